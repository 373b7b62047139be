"""Graphs, source sets and checks shared by the directed tests: the in-edge shard
(test_in_edges.py on the CPU backend, test_in_edges_gpu.py on the GPU) and the
directed batch traversal, its device validation and parent trees, the
single-source validation and the CLI (test_directed_batch.py,
test_directed_batch_gpu.py).  Every graph is a directed CSR (out-edges only,
build_csr(directed=True)); every level check is element-wise equality with the
sequential oracle on that CSR, every in-edge check equality with the numpy
transpose."""
import os
import subprocess

import numpy as np

import distributed_cuda_bfs_amd as dbfs
from distributed_cuda_bfs_amd.parallel.runtime import init_runtime, run_virtual_ranks
from distributed_cuda_bfs_amd.utils.validate import directed_first_parents, directed_levels_violations

import batch_cases as bc

N = dbfs.native
UNIT = 4096
DIRECTIONS = bc.DIRECTIONS
SOURCE_SETS = bc.SOURCE_SETS
FILE_D6 = "6 5\n0 1\n1 2\n3 2\n2 4\n4 0\n"  # the list of test_directed_stdin_reader_and_engine


def _csr(n, u, v):
    return dbfs.build_csr(n, np.asarray(u, dtype=np.uint32), np.asarray(v, dtype=np.uint32), directed=True)


def _levels(csr, src):
    return np.asarray(dbfs.cpu_bfs(csr, int(src))[0])


def _d_rmat(scale):
    def build():
        p = dbfs.rmat_params(scale, 16, 31 + scale)
        u, v = dbfs.generate_edges(p)
        g = _csr(p.n, u, v)
        # a symmetrising implementation cannot pass: some source's levels differ
        sym = dbfs.build_csr(p.n, u, v)
        some = np.nonzero(np.diff(np.asarray(g.row_off)))[0][:8]
        assert any(not np.array_equal(_levels(g, s), _levels(sym, s)) for s in some)
        return g
    return build


def _d_n4097():
    """n is not a multiple of 64, and a second 4096-vertex unit holds one vertex."""
    p = dbfs.uniform_params(4097, 10000, 5)
    u, v = dbfs.generate_edges(p)
    g = _csr(p.n, u, v)
    assert g.n == 4097 and g.n % 64 != 0
    return g


def _star_out():
    """0 -> 1..5000 and a tail 5000 -> 5001 -> 5002 -> 5003: an out-row past the
    1024 entries a wave pushes; the leaves reach only themselves."""
    k = 5000
    g = _csr(k + 4, np.concatenate([np.zeros(k, dtype=np.int64), np.arange(k, k + 3)]),
             np.concatenate([np.arange(1, k + 1), np.arange(k + 1, k + 4)]))
    assert np.diff(np.asarray(g.row_off))[0] == k > 1024
    assert np.count_nonzero(_levels(g, 17) != dbfs.UNREACHED) == 1
    return g


def _star_in():
    """1..5000 -> 0 and 0 -> 5001 -> 5002 -> 5003: an in-row of 5000.  From 0
    every leaf is unreached yet has an edge into a reached vertex: legal under
    the directed rule, a cross under the undirected one."""
    k = 5000
    g = _csr(k + 4, np.concatenate([np.arange(1, k + 1), [0, k + 1, k + 2]]),
             np.concatenate([np.zeros(k, dtype=np.int64), [k + 1, k + 2, k + 3]]))
    assert np.count_nonzero(np.asarray(g.col) == 0) == k
    lv = _levels(g, 0)
    assert np.all(lv[1:k + 1] == dbfs.UNREACHED) and lv[k + 3] == 3
    return g


def _one_way_bridge():
    """Two units of 20000 random directed pairs each and the single edge
    17 -> 4101: unit 0 reaches unit 1, never the reverse."""
    rng = np.random.default_rng(6)
    m = 20000
    u = np.concatenate([rng.integers(0, UNIT, m), rng.integers(UNIT, 2 * UNIT, m), [17]])
    v = np.concatenate([rng.integers(0, UNIT, m), rng.integers(UNIT, 2 * UNIT, m), [UNIT + 5]])
    g = _csr(2 * UNIT, u, v)
    assert np.any(_levels(g, 17)[UNIT:] != dbfs.UNREACHED)
    assert not np.any((u >= UNIT) & (v < UNIT))  # no source of unit 1 reaches unit 0
    assert np.all(_levels(g, 2 * UNIT - 1)[:UNIT] == dbfs.UNREACHED)
    return g


def _d_path():
    """i -> i + 1: depth 300 from vertex 0 (past the one-byte levels); 299 reaches only itself."""
    g = _csr(300, np.arange(0, 299), np.arange(1, 300))
    assert _levels(g, 0)[299] == 299 and np.count_nonzero(_levels(g, 299) != dbfs.UNREACHED) == 1
    return g


def _back_edge():
    """0 -> 1 -> ... -> 9 -> 0: the undirected rule would call 9 -> 0 a gap."""
    g = _csr(10, np.arange(10), (np.arange(10) + 1) % 10)
    assert _levels(g, 0)[9] == 9
    return g


def _tiny5():
    return _csr(5, [0, 4, 1, 2], [4, 0, 4, 2])


def _empty3():
    g = _csr(3, [], [])
    assert g.directed_edges == 0
    return g


def _dup_in():
    """An in-row of 6000 entries drawn from 700 sources: a long row full of duplicates."""
    rng = np.random.default_rng(9)
    return _csr(701, rng.integers(1, 701, 6000), np.zeros(6000, dtype=np.int64))


GRAPHS = {
    "d_rmat10": _d_rmat(10),
    "d_rmat13": _d_rmat(13),
    "d_n4097": _d_n4097,
    "star_out5000": _star_out,
    "star_in5000": _star_in,
    "one_way_bridge": _one_way_bridge,
    "d_path300": _d_path,
    "back_edge10": _back_edge,
    "tiny5": _tiny5,
    "empty3": _empty3,
    "file_d6": FILE_D6,
}
EXTRA_GRAPHS = {"dup_in6000": _dup_in}  # the in-edge tests only
_csr_cache = {}
_oracle_cache = {}


def file_path(name, tmp_dir):
    """The edge-list file of a file graph, written once under tmp_dir."""
    path = os.path.join(str(tmp_dir), name + ".txt")
    if not os.path.exists(path):
        with open(path, "w") as f:
            f.write(GRAPHS[name])
    return path


def host_csr(name, tmp_dir=None):
    if name not in _csr_cache:
        g = GRAPHS.get(name) or EXTRA_GRAPHS[name]
        if isinstance(g, str):
            _csr_cache[name] = dbfs.read_graph(file_path(name, tmp_dir), directed=True)
        else:
            _csr_cache[name] = g()
    return _csr_cache[name]


def make_bfs(name, rt, tmp_dir, **kw):
    """A directed BFS in mode td; the file graph is read by the BFS itself."""
    csr = host_csr(name, tmp_dir)
    g = GRAPHS.get(name)
    return dbfs.BFS(file_path(name, tmp_dir) if isinstance(g, str) else csr, rt, mode="td", directed=True, **kw)


def degrees(name):
    return np.diff(np.asarray(host_csr(name).row_off))


def oracle(name, src):
    key = (name, int(src))
    if key not in _oracle_cache:
        lv = _levels(host_csr(name), src).copy()
        lv.setflags(write=False)
        _oracle_cache[key] = lv
    return _oracle_cache[key]


SPECIAL = {
    "star_out5000": [0, 17, 5003, 5000],    # the centre, a leaf, the tail's end, the leaf the tail hangs on
    "star_in5000": [0, 17, 5001],           # the hub, a leaf, the tail
    "one_way_bridge": [17, 0, 2 * UNIT - 1, UNIT + 5],
    "d_path300": [0, 299, 150],
    "back_edge10": [0, 9, 5],
    "tiny5": [0, 1, 2, 3],
    "file_d6": [0, 3, 5],
}


def sources(name, kind):
    """batch_cases.sources on the directed graphs: the same draws, each
    structured graph's special vertices first."""
    deg = degrees(name)
    n = deg.size
    k = {"k1": 1, "k63": 63, "k64": 64, "k64dup": 64, "k130": 130}[kind]
    rng = np.random.default_rng(1000 + k + (7 if kind == "k64dup" else 0))
    src = [int(x) for x in rng.integers(0, n, k)]
    special = SPECIAL.get(name, [])
    if k > 1:
        src[:len(special)] = special
    elif special:
        src = special[:1]
    if kind == "k64dup":
        src[9] = src[5]  # two bits on one vertex
        iso = np.nonzero(deg == 0)[0]
        if iso.size:
            src[63] = int(iso[0])  # a source without out-edges on bit 63
    return src


def check_totals(name, src, res, i):
    deg = degrees(name)
    exp = oracle(name, src[i])
    hit = exp != dbfs.UNREACHED
    assert res.reached[i] == int(np.count_nonzero(hit)), f"source {i}: reached"
    assert res.edges[i] == int(deg[hit].sum()), f"source {i}: edges (out-degree sum, not halved)"
    assert res.depth[i] == int(exp[hit].max()) + 1, f"source {i}: depth"
    assert res.dist_sum[i] == int(exp[hit].astype(np.int64).sum()), f"source {i}: dist_sum"
    assert list(res.discovered[i]) == [int(c) for c in np.bincount(exp[hit])], f"source {i}: discovered"


def check_batch(name, src, res, levels):
    n = degrees(name).size
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


def batch_matches_oracle(bfs, name, kind, direction):
    src = sources(name, kind)
    res = bfs.run_batch(src, direction=direction)
    levels = bfs.batch_levels()
    check_batch(name, src, res, levels)
    if kind == "k64dup":
        assert np.array_equal(levels[9], levels[5])
    forced = {"push": "P", "pull": "L"}.get(direction)
    if forced:
        assert set(bc.forms(res)) <= {forced}
    if direction == "alternate":
        assert all(l[2] == ("P" if l[1] % 2 == 0 else "L") for l in res.levels)
    assert res.wide_levels == (name == "d_path300")
    assert bfs.graph.has_in_edges


def levels_off(bfs, name, kind="k130"):
    src = sources(name, kind)
    res = bfs.run_batch(src, levels=False)
    for i in range(len(src)):
        check_totals(name, src, res, i)


def batch_ranks(name, P, device):
    """With several ranks every level is a pull over the in-edge shards."""
    src = sources(name, "k130")
    csr = host_csr(name)

    def body(rt):
        bfs = dbfs.BFS(csr, rt, mode="td", directed=True)
        res = bfs.run_batch(src, validate=True, parents=True)
        return res, bfs.batch_levels(), bfs.batch_parents()

    for res, levels, par in run_virtual_ranks(P, body, device=device):
        check_batch(name, src, res, levels)
        assert set(bc.forms(res)) == {"L"}
        check_clean(name, src, res, levels, par)


# ---- validation and parent trees ------------------------------------------------

def as_tuples(a):
    return [tuple(int(x) for x in row) for row in np.asarray(a)]


def check_clean(name, src, res, levels, par):
    csr = host_csr(name)
    assert res.validated is True
    assert res.violations == [(0, 0, 0)] * len(src)
    k, n = levels.shape
    assert par.shape == (k, n) and par.dtype == np.int64
    for i, s in enumerate(src):
        assert directed_levels_violations(csr, levels[i], s) == (0, 0, 0)
        exp = directed_first_parents(csr, levels[i], s)
        bad = np.nonzero(par[i] != exp)[0]
        assert bad.size == 0, f"source {i}: parent of {int(bad[0])} is {int(par[i][bad[0]])}, expected {int(exp[bad[0]])}"


def validates_clean(bfs, name, kind):
    src = sources(name, kind)
    res = bfs.run_batch(src, validate=True, parents=True)
    levels = bfs.batch_levels()
    check_batch(name, src, res, levels)
    check_clean(name, src, res, levels, bfs.batch_parents())


def _planting_sources(name):
    """k64 with, on slots 3 and 63, a source that reaches a vertex of level >= 2
    and misses some vertex."""
    src = sources(name, "k64")
    if name == "d_path300":
        src[3], src[63] = 100, 200
    else:
        deg = degrees(name)
        good = [int(v) for v in np.nonzero(deg)[0][:64]
                if oracle(name, v).max() == dbfs.UNREACHED and np.any((oracle(name, v) >= 2) & (oracle(name, v) != dbfs.UNREACHED))]
        src[3], src[63] = good[0], good[-1]
    return src


def plantings(levels_row):
    """(vertex, level) to plant in one source's row: a reached vertex of level
    >= 2 two levels deeper, a reached vertex unreached, an unreached vertex reached."""
    reached = levels_row != dbfs.UNREACHED
    deep = np.nonzero(reached & (levels_row >= 2))[0]
    lost = np.nonzero(~reached)[0]
    v = int(deep[len(deep) // 2])
    return [(v, int(levels_row[v]) + 2), (v, -1), (int(lost[len(lost) // 2]), 3)]


def planted_violations(bfs, name):
    csr = host_csr(name)
    src = _planting_sources(name)
    res = bfs.run_batch(src)
    assert res.wide_levels == (name == "d_path300")
    levels = bfs.batch_levels().copy()
    assert as_tuples(bfs.engine.validate_batch_pass(src)) == [(0, 0, 0)] * 64
    seen = set()
    for slot in (3, 63):
        for v, level in plantings(levels[slot]):
            was = int(levels[slot, v])
            bfs.engine.debug_set_batch_level(slot, v, level)
            got = as_tuples(bfs.engine.validate_batch_pass(src))
            mod = levels[slot].copy()
            mod[v] = dbfs.UNREACHED if level < 0 else level
            exp = directed_levels_violations(csr, mod, src[slot])
            assert got[slot] == exp, (slot, v, level, got[slot], exp)
            assert exp != (0, 0, 0)
            assert [g for i, g in enumerate(got) if i != slot] == [(0, 0, 0)] * 63
            seen.add(tuple(x > 0 for x in exp))
            bfs.engine.debug_set_batch_level(slot, v, -1 if was == dbfs.UNREACHED else was)
    assert as_tuples(bfs.engine.validate_batch_pass(src)) == [(0, 0, 0)] * 64
    assert len(seen) > 1  # the plantings trip different rules


def planted_ranks(name, P, device):
    csr = host_csr(name)
    src = _planting_sources(name)
    slot = 63
    v, level = plantings(oracle(name, src[slot]))[0]

    def body(rt):
        bfs = dbfs.BFS(csr, rt, mode="td", directed=True)
        bfs.run_batch(src)
        bfs.engine.debug_set_batch_level(slot, v, level)
        return as_tuples(bfs.engine.validate_batch_pass(src))

    mod = oracle(name, src[slot]).copy()
    mod[v] = level
    exp = directed_levels_violations(csr, mod, src[slot])
    assert exp != (0, 0, 0)
    for got in run_virtual_ranks(P, body, device=device):
        assert got[slot] == exp and [g for i, g in enumerate(got) if i != slot] == [(0, 0, 0)] * 63


def single_source(bfs, name):
    """Mode td: validate and parents of run() by the directed rules."""
    csr = host_csr(name)
    src = sources(name, "k64")[:3]
    for s in src:
        bfs.run(s)
        levels = bfs.levels()
        assert np.array_equal(levels, oracle(name, s))
        assert bfs.validate(s) is True
        assert np.array_equal(bfs.parents(s), directed_first_parents(csr, levels, s))
    a, b = src[0], src[1]
    assert a != b
    bfs.run(b)
    assert bfs.validate(a) is False


# ---- the in-edge shard ----------------------------------------------------------

def transpose(csr):
    """(row_off, col) of the in-edges: row v holds every u with a stored entry
    u -> v, ascending, duplicates kept."""
    ro = np.asarray(csr.row_off)
    w = np.asarray(csr.col).astype(np.int64)
    u = np.repeat(np.arange(csr.n, dtype=np.int64), np.diff(ro))
    order = np.lexsort((u, w))
    t_off = np.concatenate([[0], np.cumsum(np.bincount(w, minlength=csr.n))]).astype(np.int64)
    return t_off, u[order].astype(np.uint32)


def in_edges(name, P, device, hub_sort, sort_after=False, rt=None):
    """The rank shards of in_edges_to_host(), concatenated in rank order, are
    the numpy transpose; a second build is a no-op."""
    csr = host_csr(name)

    def body(rt):
        g = N.DeviceGraph.from_host(rt.backend, csr, N.Partition(csr.n, rt.world), rt.rank)
        assert not g.has_in_edges
        if hub_sort and not sort_after:
            g.sort_neighbors_by_degree(rt.comm, True, N.MAX_HUBS, True)
        g.build_in_edges(rt.comm)
        assert g.has_in_edges
        h = g.in_edges_to_host()
        first = (np.asarray(h.row_off).copy(), np.asarray(h.col).copy())
        if hub_sort and sort_after:
            g.sort_neighbors_by_degree(rt.comm, True, N.MAX_HUBS, True)
        g.build_in_edges(rt.comm)
        h = g.in_edges_to_host()
        assert np.array_equal(first[0], np.asarray(h.row_off)) and np.array_equal(first[1], np.asarray(h.col))
        assert (h.row_lo, h.rows, h.n) == (g.lo, g.rows, csr.n)
        return first

    if P == 1:
        shards = [body(rt or init_runtime(device))]
    else:
        shards = run_virtual_ranks(P, body, device=device)
    in_edge_shards_are_the_transpose(csr, shards)


def in_edge_shards_are_the_transpose(csr, shards):
    """The (row_off, col) in-edge shards of all ranks, in rank order, against
    the numpy transpose of the host CSR."""
    t_off, t_col = transpose(csr)
    deg = np.concatenate([np.diff(ro) for ro, _ in shards])
    col = np.concatenate([c for _, c in shards])
    assert all(ro[0] == 0 for ro, _ in shards)
    assert np.array_equal(deg, np.diff(t_off))
    assert col.dtype == np.uint32 and np.array_equal(col, t_col)


def undirected_allocates_nothing(rt):
    bfs = dbfs.BFS(bc.host_csr("rmat10"), rt)
    bfs.run_batch(bc.sources("rmat10", "k64"), validate=True, parents=True)
    assert not bfs.graph.has_in_edges
    bfs.build_in_edges()
    assert not bfs.graph.has_in_edges


def build_up_front(rt, tmp_dir):
    bfs = make_bfs("d_rmat10", rt, tmp_dir)
    assert not bfs.graph.has_in_edges
    bfs.run(sources("d_rmat10", "k1")[0])  # a top-down run needs no in-edges
    assert not bfs.graph.has_in_edges
    bfs.build_in_edges()
    assert bfs.graph.has_in_edges


# ---- the checked build's word is read where the new kernels run ---------------------

def injected_violations_fail(rt, monkeypatch, pytest):
    """DBFS_FAULT_INJECT kinds in_edges_device / batch_device record violation
    99 in the in-edge build / at a level of a batch pass: the call that ran
    the kernels fails, the next clean one passes."""
    csr = host_csr("d_rmat10")
    src = sources("d_rmat10", "k64")
    monkeypatch.setenv("DBFS_FAULT_INJECT", "rank=0,kind=in_edges_device")
    bfs = dbfs.BFS(csr, rt, mode="td", directed=True)
    bfs.run(src[0])  # a traversal is not the build's
    with pytest.raises(Exception, match="device check failed on rank 0: code 99"):
        bfs.build_in_edges()
    monkeypatch.setenv("DBFS_FAULT_INJECT", "rank=0,level=1,kind=batch_device")
    bfs = dbfs.BFS(csr, rt, mode="td", directed=True)
    bfs.run(src[0])
    bfs.build_in_edges()
    with pytest.raises(Exception, match="device check failed on rank 0: code 99"):
        bfs.run_batch(src)
    monkeypatch.delenv("DBFS_FAULT_INJECT")
    bfs = dbfs.BFS(csr, rt, mode="td", directed=True)
    check_batch("d_rmat10", src, bfs.run_batch(src, validate=True), bfs.batch_levels())


def cli_checked_reports(bfs_checked, path):
    """bin/bfs_checked: the batch (which builds the in-edge shard) fails on the
    recorded violation, which the single run from <src> before it does not see."""
    flags = ["0", path, "--directed", "--roots", "70", "--batch", "--validate"]
    for inject, file in (("rank=0,kind=in_edges_device", "graph_kernels"),
                         ("rank=0,level=1,kind=batch_device", "ms_kernels")):
        env = dict(os.environ, DBFS_FAULT_INJECT=inject)
        out = subprocess.run([bfs_checked] + flags, capture_output=True, text=True, timeout=120, env=env)
        assert out.returncode != 0, out.stdout
        assert "device check failed on rank 0: code 99" in out.stderr, out.stderr[-2000:]
        assert "file " + file in out.stderr, out.stderr[-2000:]  # (the word of the file whose kernels ran)
        assert "batch validation" not in out.stdout
    out = run_cli(bfs_checked, flags)
    assert out.returncode == 0, out.stdout + out.stderr
    assert CLEAN + " gap 0 cross 0 orphan 0" in out.stdout and "Wrong output!" not in out.stdout


# ---- CLI ------------------------------------------------------------------------

CLEAN = "batch validation 70/70 sources clean"


def cli_file(tmp_dir):
    path = os.path.join(str(tmp_dir), "cli_uniform5000.txt")
    if not os.path.exists(path):
        N.write_generated_edge_list(path, dbfs.uniform_params(5000, 12000, 3))
    return path


def run_cli(bfs_bin, flags):
    return subprocess.run([bfs_bin] + flags, capture_output=True, text=True, timeout=120)


def cli_batch(bfs_bin, path, flags):
    for extra in ([], ["--no-oracle"]):
        out = run_cli(bfs_bin, ["0", path, "--directed", "--roots", "70", "--batch", "--validate"] + flags + extra)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "Wrong output!" not in out.stdout
        lines = [l for l in out.stdout.splitlines() if l.startswith("batch validation")]
        assert len(lines) == 1 and lines[0].startswith(CLEAN + " gap 0 cross 0 orphan 0"), out.stdout
    out = run_cli(bfs_bin, ["0", path, "--directed", "--roots", "70", "--batch"] + flags)
    assert out.returncode == 0 and "Output OK!" in out.stdout and "batch validation" not in out.stdout


def cli_single(bfs_bin, path, flags):
    out = run_cli(bfs_bin, ["0", path, "--directed", "--mode", "td", "--validate"] + flags)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "Wrong output!" not in out.stdout
    for mode in ("do", "bu"):
        out = run_cli(bfs_bin, ["0", path, "--directed", "--mode", mode] + flags)
        assert out.returncode == 2 and "--directed needs a top-down mode" in out.stderr
