"""Connected components on the GPU: cc_init, cc_link (its three row tiers and
the skip), cc_link_pairs, cc_compress, cc_sample and cc_sizes -- the cases of
test_components.py on the device.  What each graph exercises: a hub row of
7410 entries walked by the whole grid, 998 wave-walked rows and a giant
component to skip (rmat13); a row of 2075 duplicates in a 1024-vertex graph
(rmat10); no giant at all, so the skip skips almost nothing, and waves of 64
distinct labels in the size histogram (sparse20000); a partial giant
(partial20000); n = 64 * 64 + 1 (n4097); rows on every tier boundary and
isolated vertices (ladder); deep trees before the compress (grid70x60, the
paths); every hook on one root and a chain of re-roots (max_id_star);
self-loop-only vertices (edge_list); files, nnz = 0 and ranks without rows
(two_components, chain8, tiny5, empty3); weak connectivity from one stored
direction (the directed graphs).  Ten calls on rmat13 must agree: the labels
do not depend on the order of the races."""
import os

import pytest

import components_cases as cc

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BFS_BIN = os.path.join(REPO, "bin", "bfs")
BFS_CHECKED = os.path.join(REPO, "bin", "bfs_checked")


@pytest.mark.parametrize("graph,hub_sort", cc.CASES)
def test_components_match_references_gpu(gpu_runtime, graph, hub_sort):
    cc.matches_references(gpu_runtime, graph, hub_sort)


def test_components_edge_list_from_edges_gpu(gpu_runtime):
    cc.edge_list_from_edges(gpu_runtime)


@pytest.mark.parametrize("P", [2, 3])
@pytest.mark.parametrize("graph", cc.RANK_CASES)
def test_components_virtual_ranks_gpu(gpu_runtime, graph, P):
    cc.virtual_ranks(graph, P, "hip")


@pytest.mark.parametrize("graph", cc.TINY_RANK_CASES)
def test_components_four_ranks_with_empty_shards_gpu(gpu_runtime, graph):
    cc.virtual_ranks(graph, 4, "hip")


def test_components_label_exchange_in_pieces_gpu(gpu_runtime, monkeypatch):
    cc.virtual_ranks("rmat13", 3, "hip", piece=1000, monkeypatch=monkeypatch)


@pytest.mark.parametrize("graph", ["rmat13", "sparse20000"])
def test_components_tie_to_traversals_gpu(gpu_runtime, graph):
    cc.ties_to_traversals(gpu_runtime, graph)


def test_sample_roots_by_component_gpu(gpu_runtime):
    cc.sample_roots(gpu_runtime, pytest)


def test_components_are_deterministic_gpu(gpu_runtime):
    cc.deterministic(gpu_runtime, calls=10)


@pytest.mark.parametrize("flags,sampled", [([], True), (["--virtual-ranks", "3"], False)])
def test_cli_components_gpu(gpu_runtime, tmp_path, flags, sampled):
    cc.cli_components(BFS_BIN, flags, tmp_path, sampled)


def test_cli_components_generated_gpu(gpu_runtime):
    cc.cli_generated(BFS_BIN, [])


def test_cli_components_checked_build_gpu(gpu_runtime):
    """bin/bfs_checked runs --components clean (every DBFS_DCHECK of
    cc_kernels.hip live), and a violation recorded during the link fails it."""
    cc.cli_checked_reports(BFS_CHECKED)
