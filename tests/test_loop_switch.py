"""One engine switched between the device loop and the host loop.

The device loop remembers that a traversal left its frontier slices zero (a
run that ends on a top-down level that discovers nothing: Engine's
frontier_clean_), and the next device-loop traversal then writes only the
seed word instead of clearing them.  A host-loop traversal in between leaves
bits in both slices (a bottom-up level keeps its input, the last level's
output stays) and must therefore end that promise: the sequence device loop,
host loop, device loop, device loop on one engine, every run element-wise
against the sequential CPU oracle.  The CPU backend checks the promise
itself (init_run: "a frontier claimed clean holds a stale bit"); the HIP
kernel trusts it and would expand the stale bits.
"""
import numpy as np
import pytest

import distributed_cuda_bfs_amd as dbfs
from distributed_cuda_bfs_amd.parallel.runtime import init_runtime

SEQUENCE = (1, 0, 1, 1)  # device_loop for each pass over the roots


def _uniform():
    return dbfs.uniform_params(5000, 12000, 9), 4


def _rmat12():
    return dbfs.rmat_params(12, 16, 5), 7


def _check(bfs, csr, src, what):
    res = bfs.run(src)
    exp, _ = dbfs.cpu_bfs(csr, src)
    got = bfs.levels()
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, (f"{what}, root {src}: {bad.size} vertices differ, first " +
                           ", ".join(f"{int(v)}: {int(got[v])} vs {int(exp[v])}" for v in bad[:8]))
    assert res.reached == int(np.count_nonzero(exp != dbfs.UNREACHED))
    assert res.depth == int(exp[exp != dbfs.UNREACHED].max()) + 1
    return res


@pytest.mark.parametrize("graph", [_uniform, _rmat12], ids=["uniform5000", "rmat12"])
@pytest.mark.parametrize("mode", ["td", "do"])
@pytest.mark.parametrize("backend", ["cpu", pytest.param("hip", marks=pytest.mark.gpu)])
def test_device_host_device_loop_on_one_engine(backend, mode, graph, request):
    rt = request.getfixturevalue("gpu_runtime") if backend == "hip" else init_runtime("cpu")
    p, seed = graph()
    csr = dbfs.host_csr_from_params(p)
    bfs = dbfs.BFS(p, rt, mode=mode)
    roots = bfs.sample_roots(3, seed=seed)
    clean_ends = 0
    for i, device_loop in enumerate(SEQUENCE):
        bfs.engine.set_option("device_loop", device_loop)
        for src in roots:
            res = _check(bfs, csr, src, f"pass {i} (device_loop={device_loop})")
            last = res.levels[-1]
            clean_ends += device_loop and last["dir"] == "T" and last["discovered"] == 0
    if mode == "td":
        # (the case under test: device-loop runs that end on an empty top-down level)
        assert clean_ends > 0


@pytest.mark.parametrize("backend", ["cpu", pytest.param("hip", marks=pytest.mark.gpu)])
def test_options_between_device_loop_runs(backend, request):
    """Options set between two device-loop runs (the mode, a threshold) do not
    carry the clean-frontier promise over either: a bottom-up run after a
    top-down one that ended clean, and back."""
    rt = request.getfixturevalue("gpu_runtime") if backend == "hip" else init_runtime("cpu")
    p, seed = _uniform()
    csr = dbfs.host_csr_from_params(p)
    bfs = dbfs.BFS(p, rt, mode="td")
    roots = bfs.sample_roots(3, seed=seed)
    for i, mode in enumerate(("td", "bu", "td", "do", "td")):
        bfs.mode = mode
        bfs.engine.set_option("td_sparse_edges", 0 if i == 2 else 1 << 16)
        for src in roots:
            _check(bfs, csr, src, f"pass {i} (mode {mode})")
