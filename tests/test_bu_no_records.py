"""Bottom-up on a shard without packed row records.

DeviceGraph builds the records (ShardView::nz_rec) unless a 4096-vertex unit
spans 2^32 edges, so no graph a test can hold takes the other path by itself:
debug_drop_records() releases them.  The hub kernels then run their one
no-record form (units split at 16 words per wave, deferred row scans, rows
from the non-empty-row view) whatever bu_whole_units and bu_small_waves say,
and no level is hub-cut.  Checked element-wise against the sequential CPU
oracle on the graphs of test_bu_record_walk.py.
"""
import numpy as np
import pytest

import distributed_cuda_bfs_amd as dbfs
from distributed_cuda_bfs_amd.parallel.runtime import init_runtime, run_virtual_ranks

from test_bu_record_walk import _check, _graph, _roots

GRAPHS = ["rmat12", "rmat13", "uniform5000", "empty_middle_unit", "rows_64_65_1", "star5000"]
BACKENDS = ["cpu", pytest.param("hip", marks=pytest.mark.gpu)]


def _runtime(backend, request):
    return request.getfixturevalue("gpu_runtime") if backend == "hip" else init_runtime("cpu")


def _bfs(csr, rt, mode, drop=True, cut=False, **kw):
    bfs = dbfs.BFS(csr, rt, mode=mode, **kw)
    assert bfs.graph.nhubs > 0  # the hub kernels
    assert np.asarray(bfs.graph.debug_nz_loc()).size > 0
    if drop:
        bfs.graph.debug_drop_records()
        assert np.asarray(bfs.graph.debug_nz_loc()).size == 0
    if cut:  # the hub-cut level asked for on every first bottom-up level
        bfs.engine.set_option("bu_cut_edges", 1 << 40)
        bfs.engine.set_option("bu_cut_mf_frac", 1.0)
    return bfs


@pytest.mark.gpu
@pytest.mark.parametrize("graph", GRAPHS)
def test_no_records_levels_gpu(gpu_runtime, graph):
    """Exact levels, reached vertices and edges, bottom-up-only and
    direction-optimising, one-byte and 32-bit levels, device loop and host
    loop; the shape options change nothing and nothing fails."""
    csr = _graph(graph)
    roots = _roots(csr)
    for mode in ("bu", "do"):
        for narrow in (1, 0):
            bfs = _bfs(csr, gpu_runtime, mode)
            bfs.engine.set_option("narrow_levels", narrow)
            for whole in (1, -1):
                for small in (-1, 1):
                    bfs.engine.set_option("bu_whole_units", whole)
                    bfs.engine.set_option("bu_small_waves", small)
                    for src in roots:
                        _check(bfs, csr, src)
            bfs.engine.set_option("device_loop", 0)
            _check(bfs, csr, roots[0])


@pytest.mark.gpu
@pytest.mark.parametrize("graph", GRAPHS)
def test_no_records_same_as_records_gpu(gpu_runtime, graph):
    """The same engine and roots with and without records: per-vertex levels
    and the per-level discovered counts are identical."""
    csr = _graph(graph)
    for mode in ("bu", "do"):
        with_rec = _bfs(csr, gpu_runtime, mode, drop=False)
        without = _bfs(csr, gpu_runtime, mode)
        for src in _roots(csr):
            ra = with_rec.run(src)
            la = with_rec.levels()
            rb = without.run(src)
            assert np.array_equal(la, without.levels())
            assert [l["discovered"] for l in ra.levels] == [l["discovered"] for l in rb.levels]


@pytest.mark.parametrize("graph", GRAPHS)
@pytest.mark.parametrize("backend", BACKENDS)
def test_no_records_no_hub_cut(backend, graph, request):
    """The hub cut forced, records dropped: the cut needs the records, so no
    chain is enqueued as a hub-cut level (host logic, the same on both
    backends), and the levels are exact."""
    rt = _runtime(backend, request)
    csr = _graph(graph)
    for mode in ("bu", "do"):
        for narrow in (1, 0):
            bfs = _bfs(csr, rt, mode, cut=True)
            bfs.engine.set_option("narrow_levels", narrow)
            for src in _roots(csr):
                res = _check(bfs, csr, src)
                assert not any(c[7] for c in res.chains)


@pytest.mark.gpu
def test_no_records_virtual_ranks_gpu():
    """Three virtual ranks, records dropped on every rank, the cut forced:
    exact levels on every rank and no hub-cut chain."""
    csr = _graph("rmat13")
    srcs = _roots(csr)
    exp = [dbfs.cpu_bfs(csr, s)[0] for s in srcs]

    def body(rt):
        bfs = _bfs(csr, rt, "do", cut=True, max_hubs=2000)
        out = []
        for s in srcs:
            res = bfs.run(s)
            out.append((bfs.levels(), sum(1 for c in res.chains if c[7])))
        return out

    for rank_out in run_virtual_ranks(3, body, device="hip"):
        for (lv, ncut), e in zip(rank_out, exp):
            assert np.array_equal(lv, e)
            assert ncut == 0
