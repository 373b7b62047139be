"""Concurrent multi-source BFS on directed graphs on the GPU: the directed
ms_pull over the in-edge shard, ms_record's out-degrees, the directed ms_check,
validate_kernel and parent_kernel -- the cases of test_directed_batch.py on the
device, virtual ranks on the one GPU, and the CLI (once on the checked build)."""
import os

import pytest

import directed_cases as dc

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BFS_BIN = os.path.join(REPO, "bin", "bfs")
BFS_CHECKED = os.path.join(REPO, "bin", "bfs_checked")
_bfs_cache = {}


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return tmp_path_factory.mktemp("directed_gpu")


def _bfs(name, rt, files):
    if name not in _bfs_cache:
        _bfs_cache[name] = dc.make_bfs(name, rt, files)
    return _bfs_cache[name]


@pytest.mark.parametrize("direction", dc.DIRECTIONS)
@pytest.mark.parametrize("kind", dc.SOURCE_SETS)
@pytest.mark.parametrize("graph", list(dc.GRAPHS))
def test_directed_batch_matches_oracle_gpu(gpu_runtime, files, graph, kind, direction):
    dc.batch_matches_oracle(_bfs(graph, gpu_runtime, files), graph, kind, direction)


def test_directed_batch_levels_off_gpu(gpu_runtime, files):
    dc.levels_off(_bfs("d_n4097", gpu_runtime, files), "d_n4097")


@pytest.mark.parametrize("P", [2, 3])
@pytest.mark.parametrize("graph", ["d_rmat10", "d_n4097", "one_way_bridge"])
def test_directed_batch_virtual_ranks_gpu(gpu_runtime, graph, P):
    dc.batch_ranks(graph, P, "hip")


@pytest.mark.parametrize("graph", list(dc.GRAPHS))
def test_directed_batch_validates_clean_gpu(gpu_runtime, files, graph):
    dc.validates_clean(_bfs(graph, gpu_runtime, files), graph, "k64")


@pytest.mark.parametrize("graph,kind", [("d_n4097", "k130"), ("d_rmat13", "k63"), ("d_rmat13", "k64dup")])
def test_directed_batch_validates_clean_more_sets_gpu(gpu_runtime, files, graph, kind):
    dc.validates_clean(_bfs(graph, gpu_runtime, files), graph, kind)


@pytest.mark.parametrize("graph", ["d_rmat13", "d_path300"])
def test_directed_planted_violations_gpu(gpu_runtime, files, graph):
    dc.planted_violations(_bfs(graph, gpu_runtime, files), graph)


def test_directed_planted_violation_virtual_ranks_gpu(gpu_runtime):
    dc.planted_ranks("d_rmat13", 2, "hip")


@pytest.mark.parametrize("graph", ["d_rmat10", "star_in5000", "back_edge10"])
def test_directed_single_source_validate_and_parents_gpu(gpu_runtime, files, graph):
    dc.single_source(_bfs(graph, gpu_runtime, files), graph)


@pytest.mark.parametrize("flags", [[], ["--virtual-ranks", "3"]])
def test_cli_directed_batch_gpu(gpu_runtime, files, flags):
    dc.cli_batch(BFS_BIN, dc.cli_file(files), flags)


def test_cli_directed_single_source_gpu(gpu_runtime, files):
    dc.cli_single(BFS_BIN, dc.cli_file(files), [])


def test_cli_directed_batch_checked_build_gpu(gpu_runtime, files):
    """The checked build runs the batch line clean, and a violation recorded in
    the in-edge build or in a batch level fails it."""
    dc.cli_checked_reports(BFS_CHECKED, dc.cli_file(files))
