"""Concurrent multi-source BFS on directed graphs (BFS(..., directed=True).run_batch)
on the CPU backend: a push follows out-edges, a pull searches the in-edge shard;
every graph x source set x direction element-wise against the sequential oracle
on the directed CSR, the device validation by the directed rules and the parent
trees against utils.validate.directed_levels_violations / directed_first_parents,
planted violations, the single-source validate / parents in mode td, virtual
ranks and the CLI.  The graphs and what each is for: directed_cases.py."""
import os

import pytest

from distributed_cuda_bfs_amd.parallel.runtime import init_runtime

import directed_cases as dc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BFS_BIN = os.path.join(REPO, "bin", "bfs")
_bfs_cache = {}


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return tmp_path_factory.mktemp("directed")


def _bfs(name, files):
    if name not in _bfs_cache:
        _bfs_cache[name] = dc.make_bfs(name, init_runtime("cpu"), files)
    return _bfs_cache[name]


@pytest.mark.parametrize("direction", dc.DIRECTIONS)
@pytest.mark.parametrize("kind", dc.SOURCE_SETS)
@pytest.mark.parametrize("graph", list(dc.GRAPHS))
def test_directed_batch_matches_oracle(files, graph, kind, direction):
    dc.batch_matches_oracle(_bfs(graph, files), graph, kind, direction)


def test_directed_batch_levels_off(files):
    dc.levels_off(_bfs("d_n4097", files), "d_n4097")


@pytest.mark.parametrize("P", [2, 3])
@pytest.mark.parametrize("graph", ["d_rmat10", "d_n4097", "one_way_bridge"])
def test_directed_batch_virtual_ranks(graph, P):
    dc.batch_ranks(graph, P, "cpu")


def test_directed_push_needs_one_rank():
    with pytest.raises(Exception, match="one rank"):
        dc.run_virtual_ranks(2, lambda rt: dc.dbfs.BFS(dc.host_csr("tiny5"), rt, mode="td", directed=True)
                             .run_batch([0, 1], direction="push"), device="cpu")


@pytest.mark.parametrize("graph", list(dc.GRAPHS))
def test_directed_batch_validates_clean(files, graph):
    dc.validates_clean(_bfs(graph, files), graph, "k64")


@pytest.mark.parametrize("graph,kind", [("d_n4097", "k130"), ("d_rmat13", "k63"), ("d_rmat13", "k64dup")])
def test_directed_batch_validates_clean_more_sets(files, graph, kind):
    dc.validates_clean(_bfs(graph, files), graph, kind)


@pytest.mark.parametrize("graph", ["d_rmat13", "d_path300"])
def test_directed_planted_violations(files, graph):
    dc.planted_violations(_bfs(graph, files), graph)


def test_directed_planted_violation_virtual_ranks():
    dc.planted_ranks("d_rmat13", 2, "cpu")


@pytest.mark.parametrize("graph", ["d_rmat10", "star_in5000", "back_edge10"])
def test_directed_single_source_validate_and_parents(files, graph):
    dc.single_source(_bfs(graph, files), graph)


def test_directed_bottom_up_modes_still_raise():
    for mode in ("do", "bu"):
        with pytest.raises(ValueError):
            dc.dbfs.BFS(dc.host_csr("tiny5"), init_runtime("cpu"), mode=mode, directed=True)


def test_injected_device_violations_fail_build_and_batch(monkeypatch):
    dc.injected_violations_fail(init_runtime("cpu"), monkeypatch, pytest)


@pytest.mark.parametrize("flags", [["--cpu"], ["--cpu", "--virtual-ranks", "3"]])
def test_cli_directed_batch(files, flags):
    dc.cli_batch(BFS_BIN, dc.cli_file(files), flags)


def test_cli_directed_single_source(files):
    dc.cli_single(BFS_BIN, dc.cli_file(files), ["--cpu"])
