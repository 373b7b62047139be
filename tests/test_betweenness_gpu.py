"""Path counts and betweenness centrality of a batch on the GPU: ms_bc_init,
ms_bc_forward and ms_bc_backward (both level types) -- the cases of
test_betweenness.py on the device, virtual ranks on the one GPU, and the CLI
(once on the checked build).  What each graph exercises: a 5000-entry row
walked both ways with a partial last column step (star5000, star_in5000
forward, star_out5000 backward), n not a multiple of 64 and three passes into
one vector with 2 live lanes in the last (n4097 k130), equal-length paths,
duplicates, k < 64, two slots on one vertex and a degree-0 source (rmat13),
the whole-graph result over 16 passes (rmat10 all), lanes that never reach
half the graph (two_components, one_way_bridge), 16-bit levels and 298
launches each way (path300), one lane (file_chain8), nnz = 0 (empty3)."""
import os

import pytest

import batch_cases as bc
import betweenness_cases as bt
import directed_cases as dc

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BFS_BIN = os.path.join(REPO, "bin", "bfs")
BFS_CHECKED = os.path.join(REPO, "bin", "bfs_checked")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return tmp_path_factory.mktemp("betweenness_gpu")


@pytest.mark.parametrize("case", list(bt.HAND))
def test_betweenness_hand_derived_gpu(gpu_runtime, case):
    bt.HAND[case](gpu_runtime)


@pytest.mark.parametrize("graph,kind,directed", bt.CASES)
def test_betweenness_matches_oracle_gpu(gpu_runtime, graph, kind, directed):
    bt.matches_oracle(gpu_runtime, graph, kind, directed)


@pytest.mark.parametrize("graph,kind,directed", bt.PATH_COUNT_CASES)
def test_path_counts_equal_oracle_gpu(gpu_runtime, graph, kind, directed):
    bt.path_counts(gpu_runtime, graph, kind, directed)


def test_betweenness_is_deterministic_gpu(gpu_runtime):
    bt.deterministic(gpu_runtime)


@pytest.mark.parametrize("P", [2, 3])
@pytest.mark.parametrize("graph,directed", bt.RANK_CASES)
def test_betweenness_virtual_ranks_gpu(gpu_runtime, graph, directed, P):
    bt.virtual_ranks(graph, directed, P, "hip")


@pytest.mark.parametrize("above", [0, 64, 65])
@pytest.mark.parametrize("graph,directed", [("rmat13", False), ("d_rmat13", True)])
def test_betweenness_long_row_split_gpu(gpu_runtime, graph, directed, above):
    bt.split_threshold(gpu_runtime, graph, directed, above)


@pytest.mark.parametrize("direction", bc.DIRECTIONS)
def test_betweenness_direction_independent_gpu(gpu_runtime, direction):
    bt.direction_independent(gpu_runtime, direction)


def test_betweenness_with_validate_and_parents_gpu(gpu_runtime):
    bt.with_validate_and_parents(gpu_runtime)


def test_betweenness_argument_errors_gpu(gpu_runtime):
    bt.argument_errors(gpu_runtime, pytest)


@pytest.mark.parametrize("flags", [[], ["--directed"], ["--virtual-ranks", "3"]])
def test_cli_betweenness_gpu(gpu_runtime, files, flags):
    bt.cli_betweenness(BFS_BIN, dc.cli_file(files), flags)


def test_cli_betweenness_out_file_gpu(gpu_runtime, files):
    bt.cli_out_file(BFS_BIN, dc.cli_file(files), files, gpu_runtime, False, False)


def test_cli_betweenness_checked_build_gpu(gpu_runtime, files):
    """The checked build runs the betweenness line clean, and a violation
    recorded during the accumulation fails it."""
    bt.cli_checked_reports(BFS_CHECKED, dc.cli_file(files))
