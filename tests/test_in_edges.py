"""The in-edge shard of a directed graph (DeviceGraph.build_in_edges) on the CPU
backend: the rank shards, concatenated, equal the numpy transpose of the
directed CSR -- one rank and 2, 3 (tiny5: 4) virtual ranks, out-rows hub-sorted
before the build, after it, or never.

  d_rmat10, d_n4097   mixed degrees, duplicates, self-loops; n no multiple of 64
  star_in5000         one in-row of 5000 entries (past the 4096 a row sort holds in LDS)
  dup_in6000          a long in-row full of duplicates
  star_out5000        one out-row of 5000 entries feeding 5000 in-rows of one entry
  one_way_bridge      at P = 2 the bridge's entry crosses the rank boundary
  tiny5 at P = 4      ranks with one row or none
  empty3              nnz = 0
"""
import pytest

from distributed_cuda_bfs_amd.parallel.runtime import init_runtime

import directed_cases as dc

ONE_RANK = ["d_rmat10", "d_rmat13", "d_n4097", "star_out5000", "star_in5000", "one_way_bridge", "d_path300",
            "back_edge10", "tiny5", "empty3", "dup_in6000"]
RANKS = [("d_rmat10", 2), ("d_rmat10", 3), ("d_n4097", 2), ("d_n4097", 3), ("one_way_bridge", 2), ("star_in5000", 3),
         ("star_out5000", 2), ("dup_in6000", 2), ("tiny5", 4), ("empty3", 2)]


@pytest.mark.parametrize("hub_sort", [False, True])
@pytest.mark.parametrize("graph", ONE_RANK)
def test_in_edges_are_the_transpose(graph, hub_sort):
    dc.in_edges(graph, 1, "cpu", hub_sort)


@pytest.mark.parametrize("hub_sort", [False, True])
@pytest.mark.parametrize("graph,P", RANKS)
def test_in_edges_virtual_ranks(graph, P, hub_sort):
    dc.in_edges(graph, P, "cpu", hub_sort)


@pytest.mark.parametrize("graph,P", [("d_rmat10", 1), ("d_n4097", 3)])
def test_in_edges_survive_a_later_hub_sort(graph, P):
    dc.in_edges(graph, P, "cpu", True, sort_after=True)


def test_undirected_graphs_allocate_no_in_edges():
    dc.undirected_allocates_nothing(init_runtime("cpu"))


def test_build_in_edges_up_front(tmp_path):
    dc.build_up_front(init_runtime("cpu"), tmp_path)
