"""Engine.validate (validate_kernel, csrc/kernels/graph_kernels.hip) and
parents() (parent_kernel) on the GPU against planted violations: after a clean
traversal single levels are overwritten (Engine.debug_set_level), one planting
at a time, and validate() must return exactly what the numpy reference counts
on the modified levels -- batch_levels_violations, on the directed graph
directed_levels_violations -- and never (0, 0, 0).  The checks are in
validator_cases.py, the same as on the CPU backend.

  1  a vertex of level >= 2, the only parent of some child, two levels deeper (gaps; the child an orphan)
  2  a reached vertex to unreached (cross edges, orphans)
  3  an unreached vertex to level 3
  4  the source to level 1
  5  the highest-degree vertex two deeper, then unreached: a row the whole wave walks
  6  the last entry of that row, in the device's order, to unreached: found past the walk's first step
  7  rmat13's vertices 0 and 1 together: two rows above 64 entries in one wave

  rmat13 (999 rows above 64 entries), star5000 from its tail's end, path300, d_rmat10 (directed:
  the in-edge rows); plantings 1, 2 and 5 also at three ranks, on vertices rank 0 does not own.
"""
import pytest

from distributed_cuda_bfs_amd.parallel.runtime import run_virtual_ranks

import validator_cases as vc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("graph", vc.GRAPHS)
def test_validate_counts_planted_violations_gpu(gpu_runtime, graph):
    vc.planted_one_rank(gpu_runtime, graph)


@pytest.mark.parametrize("graph", ["rmat13", "d_rmat10"])
def test_validate_counts_planted_violations_three_ranks_gpu(gpu_runtime, graph):
    vc.check_ranks(run_virtual_ranks(3, vc.ranks_body(graph, 3), device="hip"))


@pytest.mark.parametrize("graph", vc.GRAPHS)
def test_parents_keep_the_first_match_gpu(gpu_runtime, graph):
    vc.parents_first_match(gpu_runtime, graph)


def test_debug_set_level_range_errors_gpu(gpu_runtime):
    vc.argument_errors(gpu_runtime, pytest)
