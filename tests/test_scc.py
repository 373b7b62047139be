"""Strongly connected components (BFS.strong_components) on the CPU backend:
the references against the graph facts, every graph of scc_cases.CASES with the
defaults, the forced form (no trim, no pivot), an early trim stop, virtual
ranks, the ties to run / run_batch / validate / components, sample_roots, the
failure path and the CLI (one process, virtual ranks, two processes over TCP)."""
import os

import pytest

from distributed_cuda_bfs_amd.parallel.runtime import init_runtime

import directed_cases as dc
import scc_cases as sc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BFS_BIN = os.path.join(REPO, "bin", "bfs")


@pytest.fixture(scope="module")
def rt():
    return init_runtime("cpu")


@pytest.fixture(scope="module")
def tmp_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("scc")


@pytest.mark.parametrize("graph", sc.GRAPHS)
def test_references_state_the_graph_facts(graph):
    sc.references_state_the_facts(graph)


@pytest.mark.parametrize("graph,hub_sort", sc.CASES)
def test_strong_components_match_references(rt, graph, hub_sort):
    sc.matches_references(rt, graph, hub_sort)


@pytest.mark.parametrize("graph", sc.FORCED_CASES)
def test_strong_components_forced_form(rt, graph):
    sc.forced_form(rt, graph)


def test_strong_components_early_trim_stop(rt):
    sc.early_trim_stop(rt)


@pytest.mark.parametrize("P", [2, 3])
@pytest.mark.parametrize("graph", sc.RANK_CASES)
def test_strong_components_virtual_ranks(graph, P):
    sc.virtual_ranks(graph, P, "cpu")


@pytest.mark.parametrize("graph", sc.TINY_RANK_CASES)
def test_strong_components_four_ranks_with_empty_shards(graph):
    sc.virtual_ranks(graph, 4, "cpu")


def test_strong_components_tie_to_traversals(rt):
    sc.ties_to_traversals(rt)


def test_sample_roots_by_strong_component(rt):
    sc.sample_roots(rt, pytest)


def test_strong_components_are_deterministic(rt):
    sc.deterministic(rt, calls=10)


def test_strong_component_labels_need_a_call(rt):
    sc.needs_a_call(rt, pytest)


def test_strong_components_injected_violation_fails(rt, monkeypatch):
    sc.injected_violation_fails(rt, monkeypatch, pytest)


@pytest.mark.parametrize("flags", [["--cpu"], ["--cpu", "--virtual-ranks", "3"]])
def test_cli_strong_components_directed_file(tmp_dir, flags):
    sc.cli_strong_components(BFS_BIN, dc.cli_file(tmp_dir), True, flags, tmp_dir)


@pytest.mark.parametrize("flags", [["--cpu"], ["--cpu", "--virtual-ranks", "3"]])
def test_cli_strong_components_two_components(tmp_dir, flags):
    path = os.path.join(sc.DATA, "two_components.txt")
    sc.cli_strong_components(BFS_BIN, path, False, flags, tmp_dir)
    sc.cli_strong_components(BFS_BIN, path, True, flags, tmp_dir)


def test_cli_strong_components_out_needs_strong_components():
    sc.cli_usage(BFS_BIN)


def test_cli_strong_components_two_processes(tmp_dir):
    sc.cli_two_processes(BFS_BIN, tmp_dir)
