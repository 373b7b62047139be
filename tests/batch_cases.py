"""Graphs, source sets and the oracle check shared by the concurrent multi-source
BFS tests (test_batch_bfs.py on the CPU backend, test_batch_bfs_gpu.py on the
GPU).  Every check is element-wise equality with the sequential oracle."""
import os

import numpy as np

import distributed_cuda_bfs_amd as dbfs

UNIT = 4096
DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")
DIRECTIONS = ("auto", "push", "pull", "alternate")
SOURCE_SETS = ("k1", "k63", "k64", "k64dup", "k130")


def _csr(n, u, v):
    return dbfs.build_csr(n, np.asarray(u, dtype=np.uint32), np.asarray(v, dtype=np.uint32))


def _rmat(scale):
    return lambda: dbfs.host_csr_from_params(dbfs.rmat_params(scale, 16, 31 + scale))


def _n4097():
    """n is not a multiple of 64, and there is a second unit of one vertex."""
    return dbfs.host_csr_from_params(dbfs.uniform_params(4097, 10000, 5))


def _star():
    """A star with 5000 leaves (a row longer than any per-lane limit) and a
    3-vertex tail behind the last leaf."""
    k = 5000
    u = np.concatenate([np.zeros(k, dtype=np.int64), np.arange(k, k + 3)])
    v = np.concatenate([np.arange(1, k + 1), np.arange(k + 1, k + 4)])
    return _csr(k + 4, u, v)


def _two_components():
    """Two units, a random graph in each and no edge between them."""
    rng = np.random.default_rng(6)
    m = 20000
    u = np.concatenate([rng.integers(0, UNIT, m), rng.integers(UNIT, 2 * UNIT, m)])
    v = np.concatenate([rng.integers(0, UNIT, m), rng.integers(UNIT, 2 * UNIT, m)])
    return _csr(2 * UNIT, u, v)


def _path():
    """300 vertices in a row: depth 299 from an end, past the one-byte levels."""
    return _csr(300, np.arange(0, 299), np.arange(1, 300))


FAN_SIZES = (1, 7, 8, 9, 63, 64, 65, 71, 72, 73, 128, 129)
FAN_MIDS = 129


def fan_vertex(d):
    """The vertex of the fans graphs whose row is exactly the first d mids."""
    return 1 + FAN_MIDS + FAN_SIZES.index(d)


def _fans(path):
    """Rows built around the row walk's boundaries (64 column ids per step, 8
    level lines per group): source 0, 129 mids (1 .. 129) adjacent to it, and
    for every d of FAN_SIZES one fan vertex adjacent to exactly the first d
    mids -- a row of d entries, all predecessors with one shortest path each,
    so the source's path count there is d.  path > 0: that many vertices in a
    row hang off the source (300: the pass reruns with 16-bit levels)."""
    def build():
        u = [np.zeros(FAN_MIDS, dtype=np.int64)]
        v = [np.arange(1, FAN_MIDS + 1)]
        for d in FAN_SIZES:
            u.append(np.full(d, fan_vertex(d)))
            v.append(np.arange(1, d + 1))
        n = 1 + FAN_MIDS + len(FAN_SIZES)
        if path:
            u.append(np.concatenate([[0], np.arange(n, n + path - 1)]))
            v.append(np.arange(n, n + path))
        return _csr(n + path, np.concatenate(u), np.concatenate(v))
    return build


# name -> builder of a HostCSR, or a file path (read by the BFS itself)
GRAPHS = {
    "rmat10": _rmat(10),
    "rmat13": _rmat(13),
    "n4097": _n4097,
    "star5000": _star,
    "two_components": _two_components,
    "path300": _path,
    "fans": _fans(0),
    "fans300": _fans(300),
    "file_two_components": os.path.join(DATA, "two_components.txt"),
    "file_chain8": os.path.join(DATA, "chain8.txt"),
}
_csr_cache = {}
_oracle_cache = {}


def host_csr(name):
    if name not in _csr_cache:
        g = GRAPHS[name]
        _csr_cache[name] = dbfs.read_graph(g) if isinstance(g, str) else g()
    return _csr_cache[name]


def bfs_input(name):
    """What the BFS is built from: the file path itself for the file graphs."""
    g = GRAPHS[name]
    return g if isinstance(g, str) else host_csr(name)


def degrees(name):
    return np.diff(np.asarray(host_csr(name).row_off))


def oracle(name, src):
    """cpu_bfs levels of one source, computed once and never written to."""
    key = (name, int(src))
    if key not in _oracle_cache:
        lv, _ = dbfs.cpu_bfs(host_csr(name), int(src))
        lv = np.asarray(lv).copy()
        lv.setflags(write=False)
        _oracle_cache[key] = lv
    return _oracle_cache[key]


def sources(name, kind):
    """The source set `kind` of graph `name` (deterministic).  Drawn with
    replacement, so small graphs repeat sources; the structured graphs' special
    vertices come first."""
    deg = degrees(name)
    n = deg.size
    k = {"k1": 1, "k63": 63, "k64": 64, "k64dup": 64, "k130": 130}[kind]
    rng = np.random.default_rng(1000 + k + (7 if kind == "k64dup" else 0))
    src = [int(x) for x in rng.integers(0, n, k)]
    special = []
    if name == "star5000":
        special = [0, 17, n - 1]  # the centre, a leaf, the tail's end
    elif name == "path300":
        special = [0, n - 1, 150]
    elif name in ("fans", "fans300"):
        special = [0, fan_vertex(129), 1, n - 1]  # the source of the d paths, the longest fan, a mid, the path's end
    elif name in ("two_components", "file_two_components"):
        special = [0, n - 1]  # one source in each component
    if k > 1:
        src[:len(special)] = special
    elif special:
        src = special[:1]
    if kind == "k64dup":
        src[9] = src[5]  # two bits on one vertex
        iso = np.nonzero(deg == 0)[0]
        if iso.size:
            src[63] = int(iso[0])  # a source of degree 0 on bit 63
    return src


def check_batch(name, src, res, levels):
    """`res` / `levels` of run_batch(src) against the oracle, per source."""
    deg = degrees(name)
    n = deg.size
    assert list(res.sources) == list(src)
    assert res.passes == (len(src) + 63) // 64
    assert levels.shape == (len(src), n) and levels.dtype == np.int32
    for i, s in enumerate(src):
        exp = oracle(name, s)
        got = levels[i]
        bad = np.nonzero(got != exp)[0]
        assert bad.size == 0, (f"source {i} (vertex {s}): {bad.size} vertices differ, first " +
                               ", ".join(f"{int(v)}: {int(got[v])} vs {int(exp[v])}" for v in bad[:8]))
        check_totals(name, src, res, i)


def check_totals(name, src, res, i):
    deg = degrees(name)
    exp = oracle(name, src[i])
    hit = exp != dbfs.UNREACHED
    assert res.reached[i] == int(np.count_nonzero(hit)), f"source {i}: reached"
    assert res.edges[i] == int(deg[hit].sum()) // 2, f"source {i}: edges"
    assert res.depth[i] == int(exp[hit].max()) + 1, f"source {i}: depth"
    assert res.dist_sum[i] == int(exp[hit].astype(np.int64).sum()), f"source {i}: dist_sum"
    assert list(res.discovered[i]) == [int(c) for c in np.bincount(exp[hit])], f"source {i}: discovered"


def check_dup_iso(name, src, res, levels):
    """k64dup: the duplicate's two rows are equal; an isolated source reaches itself only."""
    assert src[9] == src[5]
    assert np.array_equal(levels[9], levels[5])
    if degrees(name)[src[63]] == 0:
        assert (res.reached[63], res.edges[63], res.depth[63]) == (1, 0, 1)


def forms(res):
    return "".join(l[2] for l in res.levels)
