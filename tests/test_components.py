"""Connected components (BFS.components) on the CPU backend: the references
against the graph facts, every graph of components_cases.CASES with both
settings of cc_sample_entries, virtual ranks (also with the label exchange in
several pieces), the ties to run / run_batch / validate, sample_roots, the
failure path and the CLI (one process, virtual ranks, two processes over TCP)."""
import os

import pytest

from distributed_cuda_bfs_amd.parallel.runtime import init_runtime

import components_cases as cc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BFS_BIN = os.path.join(REPO, "bin", "bfs")


@pytest.fixture(scope="module")
def rt():
    return init_runtime("cpu")


@pytest.mark.parametrize("graph", list(cc.GRAPHS))
def test_references_state_the_graph_facts(graph):
    cc.references_state_the_facts(graph)


@pytest.mark.parametrize("graph,hub_sort", cc.CASES)
def test_components_match_references(rt, graph, hub_sort):
    cc.matches_references(rt, graph, hub_sort)


def test_components_edge_list_from_edges(rt):
    cc.edge_list_from_edges(rt)


@pytest.mark.parametrize("P", [2, 3])
@pytest.mark.parametrize("graph", cc.RANK_CASES)
def test_components_virtual_ranks(graph, P):
    cc.virtual_ranks(graph, P, "cpu")


@pytest.mark.parametrize("graph", cc.TINY_RANK_CASES)
def test_components_four_ranks_with_empty_shards(graph):
    cc.virtual_ranks(graph, 4, "cpu")


def test_components_label_exchange_in_pieces(monkeypatch):
    cc.virtual_ranks("rmat13", 3, "cpu", piece=1000, monkeypatch=monkeypatch)


@pytest.mark.parametrize("graph", ["rmat13", "sparse20000"])
def test_components_tie_to_traversals(rt, graph):
    cc.ties_to_traversals(rt, graph)


def test_sample_roots_by_component(rt):
    cc.sample_roots(rt, pytest)


def test_components_are_deterministic(rt):
    cc.deterministic(rt, calls=4)


def test_component_labels_need_a_call(rt):
    cc.needs_a_call(rt, pytest)


def test_components_injected_violation_fails(rt, monkeypatch):
    cc.injected_violation_fails(rt, monkeypatch, pytest)


@pytest.mark.parametrize("flags,sampled", [(["--cpu"], True), (["--cpu", "--virtual-ranks", "3"], False)])
def test_cli_components(tmp_path, flags, sampled):
    cc.cli_components(BFS_BIN, flags, tmp_path, sampled)


def test_cli_components_directed(tmp_path):
    out = cc.run_cli(BFS_BIN, ["0", os.path.join(cc.DATA, "two_components.txt"), "--cpu", "--directed", "--components"])
    assert out.returncode == 0 and "Components OK!" in out.stdout, out.stdout + out.stderr


def test_cli_components_generated():
    cc.cli_generated(BFS_BIN, ["--cpu"])


def test_cli_components_out_needs_components():
    cc.cli_usage(BFS_BIN)


def test_cli_components_two_processes(tmp_path):
    cc.cli_two_processes(BFS_BIN, tmp_path)
