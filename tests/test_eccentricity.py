"""Eccentricities by bounding (BFS.eccentricities) on the CPU backend: every
graph of eccentricity_cases with scopes "largest" and "all" against the
sequential oracle and the numpy loop (values, bounds, settled set, pass
counts, sources), a label as the scope, the diameter and radius targets, the
pass cap, virtual ranks (also ranks without rows), hub sort on and off with
repeated calls, the ties to run / run_batch / components, the refusals, the
failure path and the CLI (one process, virtual ranks, the sampled check, the
checked build)."""
import os

import pytest

from distributed_cuda_bfs_amd.parallel.runtime import init_runtime

import eccentricity_cases as ec

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BFS_BIN = os.path.join(REPO, "bin", "bfs")
BFS_CHECKED = os.path.join(REPO, "bin", "bfs_checked")


@pytest.fixture(scope="module")
def rt():
    return init_runtime("cpu")


@pytest.mark.parametrize("graph,scope", ec.CASES)
def test_eccentricities_match_references(rt, graph, scope):
    ec.exact_all(rt, graph, scope)


def test_eccentricities_of_a_labelled_component(rt):
    ec.by_label(rt)


@pytest.mark.parametrize("target", ["diameter", "radius"])
@pytest.mark.parametrize("scope", ec.SCOPES)
@pytest.mark.parametrize("graph", ec.TARGET_GRAPHS)
def test_eccentricity_targets(rt, graph, scope, target):
    ec.targets(rt, graph, scope, target)


def test_eccentricities_capped_on_a_cycle(rt):
    ec.capped_cycle(rt)


@pytest.mark.parametrize("P", [2, 3])
@pytest.mark.parametrize("graph,scope", ec.RANK_CASES)
def test_eccentricities_virtual_ranks(graph, scope, P):
    ec.virtual_ranks(graph, scope, P, "cpu")


@pytest.mark.parametrize("graph", ec.TINY_RANK_CASES)
def test_eccentricities_four_ranks_with_empty_shards(graph):
    ec.virtual_ranks(graph, "all", 4, "cpu")


def test_eccentricities_hub_sort_and_repeated_calls(rt):
    ec.hub_sort_and_repeats(rt)


def test_eccentricities_tie_to_traversals(rt):
    ec.ties_to_traversals(rt)


def test_eccentricity_refusals(rt):
    ec.refusals(rt, pytest)


def test_eccentricities_injected_violation_fails(rt, monkeypatch):
    ec.injected_violation_fails(rt, monkeypatch, pytest)


@pytest.mark.parametrize("flags", [["--cpu"], ["--cpu", "--virtual-ranks", "3"]])
def test_cli_eccentricities(tmp_path, flags):
    ec.cli_eccentricities(BFS_BIN, flags, tmp_path)


def test_cli_eccentricities_generated_and_sampled_check():
    ec.cli_generated(BFS_BIN, ["--cpu"])


def test_cli_eccentricity_usage_errors():
    ec.cli_usage(BFS_BIN)


def test_cli_eccentricities_checked_build_cpu():
    ec.cli_checked_reports(BFS_CHECKED, ["--cpu"])
