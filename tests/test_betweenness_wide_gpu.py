"""The wide forms of ms_bc_init / ms_bc_forward / ms_bc_backward and
ms_bc_long_kernel (ms_bc_kernels.hip; dbfs/wide.hpp) against exact arithmetic,
the cases of test_betweenness_wide.py on the GPU: counts past 2^1024 on both
level types, 2^1500 + 1 (the add's alignment) and a dependency below every
double, 7^800 through two and three waves of the long-row kernel with wide
partial sums in LDS, a full pass of 64 lanes, the same bits as the double
kernels where those are in range, "auto", three ranks on the one GPU, bin/bfs
-- and the 1056 x 1056 road grid from a corner, C(2110, 1055) ~ 2^2105."""
import os

import pytest

import betweenness_wide_cases as bw

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BFS_BIN = os.path.join(REPO, "bin", "bfs")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return tmp_path_factory.mktemp("betweenness_wide_gpu")


@pytest.mark.parametrize("graph,directed", bw.PAST)
def test_wide_counts_past_the_limit_gpu(gpu_runtime, graph, directed):
    bw.past_the_limit(gpu_runtime, graph, directed)


def test_wide_alignment_and_underflow_gpu(gpu_runtime):
    bw.alignment_and_underflow(gpu_runtime)


@pytest.mark.parametrize("split", [16, 0])
@pytest.mark.parametrize("graph,directed", bw.LONG_ROWS)
def test_wide_long_rows_gpu(gpu_runtime, graph, directed, split):
    bw.long_rows(gpu_runtime, graph, directed, split)


@pytest.mark.parametrize("split", [16, 0])
@pytest.mark.parametrize("graph", ["tail40x8w", "tail70x6w"])
def test_wide_deterministic_gpu(gpu_runtime, graph, split):
    bw.deterministic(gpu_runtime, graph, split)


def test_wide_full_pass_of_64_lanes_gpu(gpu_runtime):
    bw.full_pass(gpu_runtime)


@pytest.mark.parametrize("graph", bw.SAME_BITS)
def test_wide_same_bits_as_double_gpu(gpu_runtime, graph):
    bw.same_bits(gpu_runtime, graph)


def test_auto_redoes_only_the_overflowing_pass_gpu(gpu_runtime):
    bw.auto_redoes_one_pass(gpu_runtime, pytest)


def test_auto_stays_double_in_range_gpu(gpu_runtime):
    bw.auto_stays_double(gpu_runtime)


def test_path_counts_as_doubles_after_a_wide_batch_gpu(gpu_runtime):
    bw.counts_as_doubles_after_wide(gpu_runtime, pytest)


@pytest.mark.parametrize("graph,directed,split", [("two_chains", False, None)] + [(g, d, 16) for g, d in bw.LONG_ROWS])
def test_wide_virtual_ranks_gpu(gpu_runtime, graph, directed, split):
    bw.virtual_ranks(graph, directed, 3, "hip", split)


def test_auto_on_virtual_ranks_stays_in_step_gpu(gpu_runtime):
    bw.ranks_auto("hip")


@pytest.mark.parametrize("form", ["wide", "auto"])
@pytest.mark.parametrize("flags", [[], ["--directed"], ["--virtual-ranks", "3"]])
def test_cli_wide_counts_gpu(gpu_runtime, files, flags, form):
    bw.cli_wide(BFS_BIN, files, flags, form)


@pytest.mark.parametrize("flags", [[], ["--directed"], ["--virtual-ranks", "3"]])
def test_cli_double_counts_still_fail_loudly_gpu(gpu_runtime, files, flags):
    bw.cli_double_unchanged(BFS_BIN, files, flags)


def test_cli_counts_usage_errors_gpu(gpu_runtime, files):
    bw.cli_usage(BFS_BIN, files, [])


def test_wide_road_grid_from_a_corner_gpu(gpu_runtime):
    bw.road_grid(gpu_runtime)
