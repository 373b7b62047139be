"""Path counts and betweenness centrality of a batch (run_batch(betweenness /
path_counts)) on the CPU backend: hand-derived values, every case of
betweenness_cases.CASES against the sequential Brandes oracle, exact path
counts, determinism, virtual ranks, direction independence, the argument and
failure paths and the CLI."""
import os

import pytest

from distributed_cuda_bfs_amd.parallel.runtime import init_runtime

import batch_cases as bc
import betweenness_cases as bt
import directed_cases as dc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BFS_BIN = os.path.join(REPO, "bin", "bfs")


@pytest.fixture(scope="module")
def rt():
    return init_runtime("cpu")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return tmp_path_factory.mktemp("betweenness")


@pytest.mark.parametrize("case", list(bt.HAND))
def test_betweenness_hand_derived(rt, case):
    bt.HAND[case](rt)


def test_betweenness_scores():
    bt.scores()


@pytest.mark.parametrize("graph,kind,directed", bt.CASES)
def test_betweenness_matches_oracle(rt, graph, kind, directed):
    bt.matches_oracle(rt, graph, kind, directed)


@pytest.mark.parametrize("graph,kind,directed", bt.PATH_COUNT_CASES)
def test_path_counts_equal_oracle(rt, graph, kind, directed):
    bt.path_counts(rt, graph, kind, directed)


def test_betweenness_is_deterministic(rt):
    bt.deterministic(rt)


@pytest.mark.parametrize("P", [2, 3])
@pytest.mark.parametrize("graph,directed", bt.RANK_CASES)
def test_betweenness_virtual_ranks(graph, directed, P):
    bt.virtual_ranks(graph, directed, P, "cpu")


@pytest.mark.parametrize("above", [0, 64, 65])
@pytest.mark.parametrize("graph,directed", [("rmat13", False), ("d_rmat13", True)])
def test_betweenness_long_row_split(rt, graph, directed, above):
    bt.split_threshold(rt, graph, directed, above)


@pytest.mark.parametrize("direction", bc.DIRECTIONS)
def test_betweenness_direction_independent(rt, direction):
    bt.direction_independent(rt, direction)


def test_betweenness_with_validate_and_parents(rt):
    bt.with_validate_and_parents(rt)


def test_betweenness_argument_errors(rt):
    bt.argument_errors(rt, pytest)


def test_betweenness_injected_violation_fails(rt, monkeypatch):
    bt.injected_violation_fails(rt, monkeypatch, pytest)


@pytest.mark.parametrize("flags", [["--cpu"], ["--cpu", "--directed"], ["--cpu", "--virtual-ranks", "3"],
                                   ["--cpu", "--directed", "--virtual-ranks", "3"]])
def test_cli_betweenness(files, flags):
    bt.cli_betweenness(BFS_BIN, dc.cli_file(files), flags)


@pytest.mark.parametrize("directed", [False, True])
def test_cli_betweenness_out_file(rt, files, directed):
    bt.cli_out_file(BFS_BIN, dc.cli_file(files), files, rt, True, directed)


def test_cli_betweenness_needs_batch(files):
    bt.cli_usage(BFS_BIN, dc.cli_file(files))
