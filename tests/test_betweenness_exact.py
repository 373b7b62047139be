"""Path counts and dependency sums of a batch against exact arithmetic
(betweenness_exact_cases: Python integers and Fractions) on the CPU backend
and for the oracle cpu_betweenness, where the counts lie between 2^53 and
2^1024; and the range contract above that: the call raises, names the source,
leaves no result, and the CLI exits non-zero without a result line."""
import os

import pytest

from distributed_cuda_bfs_amd.parallel.runtime import init_runtime

import betweenness_exact_cases as bx

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BFS_BIN = os.path.join(REPO, "bin", "bfs")


@pytest.fixture(scope="module")
def rt():
    return init_runtime("cpu")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return tmp_path_factory.mktemp("betweenness_exact")


def test_exact_rounded_counts_8bit_levels(rt):
    bx.in_range_grid40(rt)


def test_exact_rounded_counts_16bit_levels(rt):
    bx.in_range_grid300(rt)


@pytest.mark.parametrize("directed", [False, True])
def test_exact_top_of_range_bit_for_bit(rt, directed):
    bx.exact_top(rt, directed)


@pytest.mark.parametrize("graph", [g for g, _ in bx.ROUNDED_TOP])
def test_exact_top_of_range_subnormal_coefficients(rt, graph):
    bx.rounded_top(rt, graph)


@pytest.mark.parametrize("split", [16, 0])
@pytest.mark.parametrize("graph,directed", bx.LONG_ROWS)
def test_exact_large_counts_long_rows(rt, graph, directed, split):
    bx.long_rows(rt, graph, directed, split)


@pytest.mark.parametrize("graph,directed", bx.RANK_CASES)
def test_exact_virtual_ranks(graph, directed):
    bx.virtual_ranks(graph, directed, 3, "cpu")


@pytest.mark.parametrize("split", [16, 0])
@pytest.mark.parametrize("graph", ["tail40x8", "tail70x6"])
def test_exact_large_counts_deterministic(rt, graph, split):
    bx.deterministic(rt, graph, split)


@pytest.mark.parametrize("graph,directed", bx.ORACLE_CASES)
def test_oracle_matches_exact(graph, directed):
    bx.oracle_matches_exact(graph, directed)


# ---- the range contract ----------------------------------------------------------------

@pytest.mark.parametrize("graph,directed", bx.OVERFLOWING)
def test_overflowing_counts_raise(rt, graph, directed):
    bx.overflow_raises(rt, pytest, graph, directed)


@pytest.mark.parametrize("graph,directed", bx.OVERFLOWING)
def test_oracle_overflowing_counts_raise(graph, directed):
    bx.oracle_overflow_raises(pytest, graph, directed)


def test_middle_source_of_overflowing_path_succeeds(rt):
    bx.middle_source_succeeds(rt)


def test_one_overflowing_lane_of_a_full_pass_raises(rt):
    bx.one_lane_overflows(rt, pytest)


def test_overflow_in_third_pass_leaves_no_result(rt):
    bx.third_pass_overflows(rt, pytest)


def test_overflow_in_a_long_row_raises(rt):
    bx.long_row_overflows(rt, pytest)


def test_overflow_raises_on_every_virtual_rank():
    bx.ranks_overflow(pytest, "cpu")


@pytest.mark.parametrize("flags", [["--cpu"], ["--cpu", "--directed"], ["--cpu", "--virtual-ranks", "3"]])
def test_cli_overflow_fails_loudly(files, flags):
    bx.cli_overflow(BFS_BIN, files, flags)
