"""Extended-range path counts (run_batch(wide_counts=...), dbfs/wide.hpp) on the
CPU backend and for the oracle cpu_betweenness(wide_counts=True), against
exact arithmetic where counts pass 2^1024 (betweenness_wide_cases): counts as
mantissa and exponent, finite dependency sums, the same bits as the double
path where that path is in range, "auto", three ranks and the CLI."""
import os

import pytest

from distributed_cuda_bfs_amd.parallel.runtime import init_runtime

import betweenness_wide_cases as bw

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BFS_BIN = os.path.join(REPO, "bin", "bfs")


@pytest.fixture(scope="module")
def rt():
    return init_runtime("cpu")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return tmp_path_factory.mktemp("betweenness_wide")


@pytest.mark.parametrize("graph,directed", bw.PAST)
def test_wide_counts_past_the_limit(rt, graph, directed):
    bw.past_the_limit(rt, graph, directed)


def test_wide_alignment_and_underflow(rt):
    bw.alignment_and_underflow(rt)


@pytest.mark.parametrize("split", [16, 0])
@pytest.mark.parametrize("graph,directed", bw.LONG_ROWS)
def test_wide_long_rows(rt, graph, directed, split):
    bw.long_rows(rt, graph, directed, split)


@pytest.mark.parametrize("split", [16, 0])
@pytest.mark.parametrize("graph", ["tail40x8w", "tail70x6w"])
def test_wide_deterministic(rt, graph, split):
    bw.deterministic(rt, graph, split)


def test_wide_full_pass_of_64_lanes(rt):
    bw.full_pass(rt)


@pytest.mark.parametrize("graph", bw.SAME_BITS)
def test_wide_same_bits_as_double(rt, graph):
    bw.same_bits(rt, graph)


def test_auto_redoes_only_the_overflowing_pass(rt):
    bw.auto_redoes_one_pass(rt, pytest)


def test_auto_stays_double_in_range(rt):
    bw.auto_stays_double(rt)


def test_path_counts_as_doubles_after_a_wide_batch(rt):
    bw.counts_as_doubles_after_wide(rt, pytest)


@pytest.mark.parametrize("graph,directed", bw.ORACLE_CASES)
def test_wide_oracle_matches_exact(graph, directed):
    bw.oracle_matches_exact(graph, directed)


@pytest.mark.parametrize("graph,directed,split", [("two_chains", False, None)] + [(g, d, 16) for g, d in bw.LONG_ROWS])
def test_wide_virtual_ranks(graph, directed, split):
    bw.virtual_ranks(graph, directed, 3, "cpu", split)


def test_auto_on_virtual_ranks_stays_in_step():
    bw.ranks_auto("cpu")


@pytest.mark.parametrize("form", ["wide", "auto"])
@pytest.mark.parametrize("flags", [["--cpu"], ["--cpu", "--directed"], ["--cpu", "--virtual-ranks", "3"]])
def test_cli_wide_counts(files, flags, form):
    bw.cli_wide(BFS_BIN, files, flags, form)


@pytest.mark.parametrize("flags", [["--cpu"], ["--cpu", "--directed"], ["--cpu", "--virtual-ranks", "3"]])
def test_cli_double_counts_still_fail_loudly(files, flags):
    bw.cli_double_unchanged(BFS_BIN, files, flags)


def test_cli_counts_usage_errors(files):
    bw.cli_usage(BFS_BIN, files, ["--cpu"])
