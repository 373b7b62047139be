"""The in-edge shard of a directed graph on the GPU: the in_route_count /
in_route_fill kernels, the entry build and the row sort (rows past 4096
entries by the radix form) against the numpy transpose, on the graphs and rank
counts of test_in_edges.py (virtual ranks share the one GPU)."""
import pytest

import directed_cases as dc
from test_in_edges import ONE_RANK, RANKS

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("hub_sort", [False, True])
@pytest.mark.parametrize("graph", ONE_RANK)
def test_in_edges_are_the_transpose_gpu(gpu_runtime, graph, hub_sort):
    dc.in_edges(graph, 1, "hip", hub_sort, rt=gpu_runtime)


@pytest.mark.parametrize("hub_sort", [False, True])
@pytest.mark.parametrize("graph,P", RANKS)
def test_in_edges_virtual_ranks_gpu(gpu_runtime, graph, P, hub_sort):
    dc.in_edges(graph, P, "hip", hub_sort)


@pytest.mark.parametrize("graph,P", [("d_rmat10", 1), ("d_n4097", 3)])
def test_in_edges_survive_a_later_hub_sort_gpu(gpu_runtime, graph, P):
    dc.in_edges(graph, P, "hip", True, sort_after=True, rt=gpu_runtime if P == 1 else None)


def test_undirected_graphs_allocate_no_in_edges_gpu(gpu_runtime):
    dc.undirected_allocates_nothing(gpu_runtime)


def test_build_in_edges_up_front_gpu(gpu_runtime, tmp_path):
    dc.build_up_front(gpu_runtime, tmp_path)
