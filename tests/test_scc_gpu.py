"""Strongly connected components on the GPU: scc_init, scc_trim, scc_pivot,
scc_colour_init, scc_forward, scc_backward, scc_end_round and scc_relabel --
the cases of test_scc.py on the device.  What each graph exercises: a giant
SCC among thousands of trimmed singletons, wave-walked hub rows in both views
(d_rmat10, d_rmat13); n = 64 * 64 + 1 (d_n4097); two large SCCs and a bridge
the classes must cut (one_way_bridge); an out-row and an in-row of 5000 whose
walk ends at the first entry or never (the stars, dup_in6000's duplicates);
trim alone (d_path300, empty3); a colour and a closure that cross 3000 vertices
one sweep at a time, so the host's batched counter reads (cycle3000_desc,
back_edge10); one round per cycle against one round in all (the cycle chains);
wave-tier rows on both sides of one vertex and the relabel of a pivot that is
not its component's smallest id (hub_cycle5000, bowtie); an undirected graph,
whose in-view is the graph itself (rmat13).  Ten calls on d_rmat13 must agree:
the labels do not depend on the order in which a sweep's rows ran."""
import os

import pytest

import directed_cases as dc
import scc_cases as sc

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BFS_BIN = os.path.join(REPO, "bin", "bfs")
BFS_CHECKED = os.path.join(REPO, "bin", "bfs_checked")


@pytest.fixture(scope="module")
def tmp_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("scc_gpu")


@pytest.mark.parametrize("graph,hub_sort", sc.CASES)
def test_strong_components_match_references_gpu(gpu_runtime, graph, hub_sort):
    sc.matches_references(gpu_runtime, graph, hub_sort)


@pytest.mark.parametrize("graph", sc.FORCED_CASES)
def test_strong_components_forced_form_gpu(gpu_runtime, graph):
    sc.forced_form(gpu_runtime, graph)


def test_strong_components_early_trim_stop_gpu(gpu_runtime):
    sc.early_trim_stop(gpu_runtime)


@pytest.mark.parametrize("P", [2, 3])
@pytest.mark.parametrize("graph", sc.RANK_CASES)
def test_strong_components_virtual_ranks_gpu(gpu_runtime, graph, P):
    sc.virtual_ranks(graph, P, "hip")


@pytest.mark.parametrize("graph", sc.TINY_RANK_CASES)
def test_strong_components_four_ranks_with_empty_shards_gpu(gpu_runtime, graph):
    sc.virtual_ranks(graph, 4, "hip")


def test_strong_components_tie_to_traversals_gpu(gpu_runtime):
    sc.ties_to_traversals(gpu_runtime)


def test_sample_roots_by_strong_component_gpu(gpu_runtime):
    sc.sample_roots(gpu_runtime, pytest)


def test_strong_components_are_deterministic_gpu(gpu_runtime):
    sc.deterministic(gpu_runtime, calls=10)


def test_strong_component_labels_need_a_call_gpu(gpu_runtime):
    sc.needs_a_call(gpu_runtime, pytest)


@pytest.mark.parametrize("flags", [[], ["--virtual-ranks", "3"]])
def test_cli_strong_components_gpu(gpu_runtime, tmp_dir, flags):
    sc.cli_strong_components(BFS_BIN, dc.cli_file(tmp_dir), True, flags, tmp_dir)
    sc.cli_strong_components(BFS_BIN, os.path.join(sc.DATA, "two_components.txt"), False, flags, tmp_dir)


def test_cli_strong_components_checked_build_gpu(gpu_runtime, tmp_dir):
    """bin/bfs_checked runs --directed --strong-components clean (every
    DBFS_DCHECK of scc_kernels.hip live), and a violation recorded during the
    first trim fails it, naming scc_kernels."""
    sc.cli_checked_reports(BFS_CHECKED, dc.cli_file(tmp_dir))
