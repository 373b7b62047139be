"""ms_bc_forward / ms_bc_backward (ms_bc_kernels.hip) against exact arithmetic,
the cases of test_betweenness_exact.py on the GPU: rounded counts on both
level types, a full pass of 64 lanes with different level sets (grid40x40),
2^1023 bit for bit, subnormal coefficients 1 / sigma (tripled646, mult2357: a
device that flushed them would lose the deepest vertices' dependencies),
counts near 2^990 through two and three waves of ms_bc_long_kernel whose
chunk is rounded up to 64 entries (tail40x8, tail70x6; bc_split_row 16 and
0), both directed sweeps, three ranks on the one GPU -- and the overflow mask:
set by the wave-per-vertex store and by the long-row store, read by the
engine before a count leaves the device."""
import os

import pytest

import betweenness_exact_cases as bx

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BFS_BIN = os.path.join(REPO, "bin", "bfs")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return tmp_path_factory.mktemp("betweenness_exact_gpu")


def test_exact_rounded_counts_8bit_levels_gpu(gpu_runtime):
    bx.in_range_grid40(gpu_runtime)


def test_exact_rounded_counts_16bit_levels_gpu(gpu_runtime):
    bx.in_range_grid300(gpu_runtime)


@pytest.mark.parametrize("directed", [False, True])
def test_exact_top_of_range_bit_for_bit_gpu(gpu_runtime, directed):
    bx.exact_top(gpu_runtime, directed)


@pytest.mark.parametrize("graph", [g for g, _ in bx.ROUNDED_TOP])
def test_exact_top_of_range_subnormal_coefficients_gpu(gpu_runtime, graph):
    bx.rounded_top(gpu_runtime, graph)


@pytest.mark.parametrize("split", [16, 0])
@pytest.mark.parametrize("graph,directed", bx.LONG_ROWS)
def test_exact_large_counts_long_rows_gpu(gpu_runtime, graph, directed, split):
    bx.long_rows(gpu_runtime, graph, directed, split)


@pytest.mark.parametrize("graph,directed", bx.RANK_CASES)
def test_exact_virtual_ranks_gpu(gpu_runtime, graph, directed):
    bx.virtual_ranks(graph, directed, 3, "hip")


@pytest.mark.parametrize("split", [16, 0])
@pytest.mark.parametrize("graph", ["tail40x8", "tail70x6"])
def test_exact_large_counts_deterministic_gpu(gpu_runtime, graph, split):
    bx.deterministic(gpu_runtime, graph, split)


# ---- the range contract ----------------------------------------------------------------

@pytest.mark.parametrize("graph,directed", bx.OVERFLOWING)
def test_overflowing_counts_raise_gpu(gpu_runtime, graph, directed):
    bx.overflow_raises(gpu_runtime, pytest, graph, directed)


def test_middle_source_of_overflowing_path_succeeds_gpu(gpu_runtime):
    bx.middle_source_succeeds(gpu_runtime)


def test_one_overflowing_lane_of_a_full_pass_raises_gpu(gpu_runtime):
    bx.one_lane_overflows(gpu_runtime, pytest)


def test_overflow_in_third_pass_leaves_no_result_gpu(gpu_runtime):
    bx.third_pass_overflows(gpu_runtime, pytest)


def test_overflow_in_a_long_row_raises_gpu(gpu_runtime):
    bx.long_row_overflows(gpu_runtime, pytest)


def test_overflow_raises_on_every_virtual_rank_gpu(gpu_runtime):
    bx.ranks_overflow(pytest, "hip")


@pytest.mark.parametrize("flags", [[], ["--directed"], ["--virtual-ranks", "3"]])
def test_cli_overflow_fails_loudly_gpu(gpu_runtime, files, flags):
    bx.cli_overflow(BFS_BIN, files, flags)
