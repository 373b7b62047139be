"""Concurrent multi-source BFS (BFS.run_batch) on the CPU backend: every graph,
source set and direction against the sequential oracle, virtual ranks, the
isolation from the single-source state, levels off, and the CLI."""
import os
import subprocess

import numpy as np
import pytest

import distributed_cuda_bfs_amd as dbfs
from distributed_cuda_bfs_amd.parallel.runtime import init_runtime, run_virtual_ranks

import batch_cases as bc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BFS_BIN = os.path.join(REPO, "bin", "bfs")
_bfs_cache = {}


def _bfs(name):
    if name not in _bfs_cache:
        _bfs_cache[name] = dbfs.BFS(bc.bfs_input(name), init_runtime("cpu"))
    return _bfs_cache[name]


@pytest.mark.parametrize("direction", bc.DIRECTIONS)
@pytest.mark.parametrize("kind", bc.SOURCE_SETS)
@pytest.mark.parametrize("graph", list(bc.GRAPHS))
def test_batch_matches_oracle(graph, kind, direction):
    bfs = _bfs(graph)
    src = bc.sources(graph, kind)
    res = bfs.run_batch(src, direction=direction)
    levels = bfs.batch_levels()
    bc.check_batch(graph, src, res, levels)
    if kind == "k64dup":
        bc.check_dup_iso(graph, src, res, levels)
    forced = {"push": "P", "pull": "L"}.get(direction)
    if forced:
        assert set(bc.forms(res)) <= {forced}
    if direction == "alternate":
        assert all(l[2] == ("P" if l[1] % 2 == 0 else "L") for l in res.levels)
    # depth 299 does not fit one-byte levels: the pass was rerun with 16-bit ones
    assert res.wide_levels == (graph in ("path300", "fans300"))


def test_auto_takes_both_forms():
    res = _bfs("rmat13").run_batch(bc.sources("rmat13", "k64"), direction="auto", levels=False)
    f = bc.forms(res)
    assert f.count("P") > 0 and f.count("L") > 0, f


@pytest.mark.parametrize("P", [2, 3])
@pytest.mark.parametrize("graph", ["rmat10", "n4097", "path300"])
def test_batch_virtual_ranks(graph, P):
    src = bc.sources(graph, "k130")

    def body(rt):
        bfs = dbfs.BFS(bc.host_csr(graph), rt)
        res = bfs.run_batch(src)
        levels = bfs.batch_levels()
        with pytest.raises(Exception, match="one rank"):
            bfs.run_batch(src[:3], direction="push")
        return res, levels

    for res, levels in run_virtual_ranks(P, body, device="cpu"):
        bc.check_batch(graph, src, res, levels)
        assert set(bc.forms(res)) == {"L"}


def test_batch_leaves_single_source_state_alone():
    graph = "rmat10"
    bfs = dbfs.BFS(bc.host_csr(graph), init_runtime("cpu"), mode="do")
    src = bc.sources(graph, "k64")
    a, b = src[0], src[1]
    bfs.run(a)
    before = bfs.levels().copy()
    res = bfs.run_batch(src)
    bc.check_batch(graph, src, res, bfs.batch_levels())
    bfs.run(a)
    after = bfs.levels().copy()
    assert np.array_equal(before, bc.oracle(graph, a)) and np.array_equal(after, before)
    many = bfs.run_many([b, a])
    assert np.array_equal(bfs.levels(), bc.oracle(graph, a))
    assert many[0].reached == int(np.count_nonzero(bc.oracle(graph, b) != dbfs.UNREACHED))


def test_batch_levels_off():
    graph = "n4097"
    bfs = dbfs.BFS(bc.host_csr(graph), init_runtime("cpu"))
    src = bc.sources(graph, "k130")
    res = bfs.run_batch(src, levels=False)
    for i in range(len(src)):
        bc.check_totals(graph, src, res, i)
    with pytest.raises(Exception, match="keep_levels"):
        bfs.batch_levels()


def test_batch_result_exported():
    assert dbfs.BatchResult is type(_bfs("file_chain8").run_batch([0]))
    with pytest.raises(ValueError):
        _bfs("file_chain8").run_batch([0], direction="sideways")
    with pytest.raises(Exception, match="out of range"):
        _bfs("file_chain8").run_batch([8])


@pytest.mark.parametrize("extra", [[], ["--virtual-ranks", "3"]])
def test_cli_batch(extra):
    out = subprocess.run([BFS_BIN, "--cpu", "--uniform", "5000:12000", "--roots", "70", "--batch"] + extra,
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "Wrong output!" not in out.stdout
    tail = out.stdout[out.stdout.index("Starting queue parallel bfs."):]
    assert tail.count("Output OK!") == 2  # the single run from <src>, then the batch
    line = [l for l in out.stdout.splitlines() if l.startswith("batch roots ")]
    assert len(line) == 1 and line[0].startswith("batch roots 70 passes 2 ms "), out.stdout
    assert " aggregate GTEPS " in line[0]
