"""Engine.validate and parents() on the CPU backend against planted
violations; the checks are in validator_cases.py, the same as on the GPU
(test_validator_gpu.py, whose docstring lists the plantings)."""
import pytest

from distributed_cuda_bfs_amd.parallel.runtime import init_runtime, run_virtual_ranks

import validator_cases as vc


@pytest.fixture(scope="module")
def rt():
    return init_runtime("cpu")


@pytest.mark.parametrize("graph", vc.GRAPHS)
def test_validate_counts_planted_violations(rt, graph):
    vc.planted_one_rank(rt, graph)


@pytest.mark.parametrize("graph", ["rmat13", "d_rmat10"])
def test_validate_counts_planted_violations_three_ranks(graph):
    vc.check_ranks(run_virtual_ranks(3, vc.ranks_body(graph, 3), device="cpu"))


@pytest.mark.parametrize("graph", vc.GRAPHS)
def test_parents_keep_the_first_match(rt, graph):
    vc.parents_first_match(rt, graph)


def test_debug_set_level_range_errors(rt):
    vc.argument_errors(rt, pytest)
