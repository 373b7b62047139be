"""The bottom-up kernels' record-order walk and the array it needs.

ShardView::nz_loc (the position of every non-empty row's vertex inside its
4096-vertex unit) is checked against its definition on both backends; the
walk itself (whole 64-word units per wave, csrc/kernels/bu_kernels.hip) is
checked through the engine, element-wise against the sequential CPU oracle,
on the smallest graphs at which it can go wrong: a partial unit, exactly one
and two units, a unit without rows between two with rows, units of exactly
64 / 65 / 1 non-empty rows (a step boundary; the last record's end is the
unit's span), a row longer than kSortedRowMax, and a component that is never
reached (its units stay on the record-order walk at every level while the
reached component's units drop to the compaction walk: both walks in one
launch).
"""
import numpy as np
import pytest

import distributed_cuda_bfs_amd as dbfs
from distributed_cuda_bfs_amd.parallel.runtime import init_runtime

UNIT = 4096


def _csr(n, u, v):
    return dbfs.build_csr(n, np.asarray(u, dtype=np.uint32), np.asarray(v, dtype=np.uint32))


def _rmat(scale):
    return lambda: dbfs.host_csr_from_params(dbfs.rmat_params(scale, 16, 31 + scale))


def _uniform():
    return dbfs.host_csr_from_params(dbfs.uniform_params(5000, 12000, 9))


def _n4097():
    return dbfs.host_csr_from_params(dbfs.uniform_params(4097, 10000, 5))


def _empty_middle_unit():
    """Three units; every vertex of the middle one is isolated."""
    rng = np.random.default_rng(3)
    pool = np.concatenate([np.arange(0, UNIT), np.arange(2 * UNIT, 3 * UNIT)])
    m = 12000
    return _csr(3 * UNIT, pool[rng.integers(0, pool.size, m)], pool[rng.integers(0, pool.size, m)])


def _rows_64_65_1():
    """Units with exactly 64, 65 and 1 non-empty rows (the last one's only row
    is its last vertex), joined by a shuffled path plus a few chords."""
    rng = np.random.default_rng(4)
    a = np.sort(rng.choice(UNIT, 64, replace=False))
    b = UNIT + np.sort(rng.choice(UNIT, 65, replace=False))
    c = np.array([3 * UNIT - 1])
    verts = np.concatenate([a, b, c])
    order = rng.permutation(verts)
    u, v = order[:-1], order[1:]
    cu, cv = verts[rng.integers(0, verts.size, 40)], verts[rng.integers(0, verts.size, 40)]
    return _csr(3 * UNIT, np.concatenate([u, cu]), np.concatenate([v, cv]))


def _star():
    """A star with 5000 leaves (the centre's row is longer than kSortedRowMax =
    4096) and a short tail behind the last leaf."""
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


GRAPHS = {
    "rmat10": _rmat(10),
    "rmat12": _rmat(12),
    "rmat13": _rmat(13),
    "uniform5000": _uniform,
    "empty_middle_unit": _empty_middle_unit,
    "rows_64_65_1": _rows_64_65_1,
    "star5000": _star,
    "two_components": _two_components,
}
_cache = {}


def _graph(name):
    if name not in _cache:
        _cache[name] = GRAPHS[name]()
    return _cache[name]


def _roots(csr):
    """The highest-degree vertex, vertex 0 and a vertex of the lowest non-zero degree."""
    deg = np.diff(np.asarray(csr.row_off))
    low = int(np.nonzero(deg == deg[deg > 0].min())[0][0])
    return [int(np.argmax(deg)), 0, low]


def _check(bfs, csr, src):
    res = bfs.run(src)
    exp, _ = dbfs.cpu_bfs(csr, src)
    got = bfs.levels()
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, (f"root {src}: {bad.size} vertices differ, first " +
                           ", ".join(f"{int(v)}: {int(got[v])} vs {int(exp[v])}" for v in bad[:8]))
    assert res.reached == int(np.count_nonzero(exp != dbfs.UNREACHED))
    deg = np.diff(np.asarray(csr.row_off))
    assert res.edges == int(deg[exp != dbfs.UNREACHED].sum()) // 2
    return res


# ---- nz_loc against its definition -------------------------------------------------


def _expected_loc(csr):
    deg = np.diff(np.asarray(csr.row_off))
    return (np.nonzero(deg > 0)[0] % UNIT).astype(np.uint16)


@pytest.mark.parametrize("graph", ["uniform5000", "rmat13", "n4097"])
@pytest.mark.parametrize("backend", ["cpu", pytest.param("hip", marks=pytest.mark.gpu)])
def test_nz_loc_definition(backend, graph, request):
    """4096 U + nz_loc[k] is the k-th vertex of degree >= 1 (U its unit):
    isolated vertices and a partial last unit, two full units, and 4097
    vertices (a second unit of one vertex)."""
    rt = request.getfixturevalue("gpu_runtime") if backend == "hip" else init_runtime("cpu")
    csr = _n4097() if graph == "n4097" else _graph(graph)
    exp = _expected_loc(csr)
    for hub_sort in (False, True):
        bfs = dbfs.BFS(csr, rt, hub_sort=hub_sort)
        got = np.asarray(bfs.graph.debug_nz_loc())
        assert got.dtype == np.uint16 and got.shape == exp.shape
        assert np.array_equal(got, exp)
        # (the definition, spelled out: the vertices recovered from the records' order)
        deg = np.diff(np.asarray(csr.row_off))
        nz = np.nonzero(deg > 0)[0]
        assert np.array_equal((nz // UNIT) * UNIT + got.astype(np.int64), nz)


# ---- the walk through the engine ------------------------------------------------------


def _bfs(csr, rt, mode, narrow, cut):
    bfs = dbfs.BFS(csr, rt, mode=mode)
    assert bfs.graph.nhubs > 0  # the hub kernels (the record variants are theirs)
    bfs.engine.set_option("bu_whole_units", 1)  # a whole unit per wave: the variants with the walk
    bfs.engine.set_option("narrow_levels", narrow)
    if cut:  # the hub-cut level forced on every first bottom-up level
        bfs.engine.set_option("bu_cut_edges", 1 << 40)
        bfs.engine.set_option("bu_cut_mf_frac", 1.0)
    return bfs


@pytest.mark.gpu
@pytest.mark.parametrize("graph", list(GRAPHS))
def test_record_walk_levels_gpu(gpu_runtime, graph):
    """Exact levels, reached vertices and edges in bottom-up-only and
    direction-optimising runs, one-byte and 32-bit levels."""
    csr = _graph(graph)
    for mode in ("bu", "do"):
        for narrow in (1, 0):
            bfs = _bfs(csr, gpu_runtime, mode, narrow, cut=False)
            for src in _roots(csr):
                _check(bfs, csr, src)


@pytest.mark.gpu
@pytest.mark.parametrize("graph", list(GRAPHS))
def test_record_walk_hub_cut_gpu(gpu_runtime, graph):
    """The same with the hub-cut level forced (claims in the level bytes, or
    with 32-bit levels in their own bytes), the long-row graph included."""
    csr = _graph(graph)
    for mode in ("bu", "do"):
        for narrow in (1, 0):
            bfs = _bfs(csr, gpu_runtime, mode, narrow, cut=True)
            for src in _roots(csr):
                _check(bfs, csr, src)


@pytest.mark.gpu
@pytest.mark.parametrize("graph", ["rmat10", "rmat12", "rmat13"])
def test_record_walk_validates_gpu(gpu_runtime, graph):
    """The device-side Graph500 validation accepts the levels."""
    csr = _graph(graph)
    for mode in ("bu", "do"):
        for cut in (False, True):
            bfs = _bfs(csr, gpu_runtime, mode, 1, cut)
            for src in _roots(csr):
                bfs.run(src)
                assert bfs.validate(src)
