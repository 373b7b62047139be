"""Binned levels that settle and finish in bin_apply_kernel, on the GPU
(binned_settle_cases.py), plus the unfolded scan: more than FOLD_SCAN_UNITS
units need 2^25 vertices, whose host oracle is too slow to compute for one
case -- that one runs on test_gpu_shard_sizes' graph C (power law, 8301
units), built once and shared with that module."""
import pytest

import binned_settle_cases as bs
import test_gpu_shard_sizes as sz

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,mode,narrow", bs.params())
def test_binned_settle_gpu(gpu_runtime, name, mode, narrow):
    bs.check_case(gpu_runtime, name, mode, narrow)


@pytest.mark.parametrize("narrow", bs.NARROW)
def test_binned_settle_unfolded_scan_gpu(gpu_runtime, narrow):
    """td mode on graph C: binned levels whose unit statistics a
    scan_units launch (no folded scan) and the compaction read back; the
    checks are test_gpu_shard_sizes.check_run's (levels, records, validate)
    and the host loop's records."""
    if "C" not in sz._shards:
        sz._shards["C"] = sz.Shard("C", gpu_runtime)  # (test_gpu_shard_sizes finds it there)
    g = sz._shards["C"]
    assert g.units > bs.N.FOLD_SCAN_UNITS
    bfs = g.bfs()
    try:
        bfs.mode = "td"
        for k, v in dict(bs.OPTIONS, narrow_levels=narrow).items():
            bfs.engine.set_option(k, v)
        src = g.roots[0]
        res = sz.check_run(g, bfs, src)
        chains = bs.forms(res)
        assert "X" in chains, chains
        bfs.engine.set_option("device_loop", 0)
        host = bfs.run(src)
        assert not host.chains
        assert bs.strip(host) == bs.strip(res), chains
        assert (host.reached, host.edges, host.depth) == (res.reached, res.edges, res.depth)
    finally:
        g.restore()
