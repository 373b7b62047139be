"""Eccentricities by bounding on the GPU: ecc_degrees, ecc_init, ecc_select
(its per-workgroup lists and the merge), ecc_update at both level widths and
ecc_totals -- the cases of test_eccentricity.py on the device.  What each
graph exercises is listed in eccentricity_cases; on the device in particular:
the last partial group of rows of the update (n4097: 64 * 64 + 1 vertices),
128-byte rows (path_zigzag, cycle2000), a selection whose live set shrinks to
a handful over 35, 129 and 141 passes (n4097, partial20000, sparse20000), more
than one selecting workgroup (every graph above 256 vertices) and fewer live
vertices than one pass holds (chain8, two_components, path65's second pass)."""
import os

import pytest

import eccentricity_cases as ec

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BFS_BIN = os.path.join(REPO, "bin", "bfs")
BFS_CHECKED = os.path.join(REPO, "bin", "bfs_checked")


@pytest.mark.parametrize("graph,scope", ec.CASES)
def test_eccentricities_match_references_gpu(gpu_runtime, graph, scope):
    ec.exact_all(gpu_runtime, graph, scope)


def test_eccentricities_of_a_labelled_component_gpu(gpu_runtime):
    ec.by_label(gpu_runtime)


@pytest.mark.parametrize("target", ["diameter", "radius"])
@pytest.mark.parametrize("scope", ec.SCOPES)
@pytest.mark.parametrize("graph", ec.TARGET_GRAPHS)
def test_eccentricity_targets_gpu(gpu_runtime, graph, scope, target):
    ec.targets(gpu_runtime, graph, scope, target)


def test_eccentricities_capped_on_a_cycle_gpu(gpu_runtime):
    ec.capped_cycle(gpu_runtime)


@pytest.mark.parametrize("P", [2, 3])
@pytest.mark.parametrize("graph,scope", ec.RANK_CASES)
def test_eccentricities_virtual_ranks_gpu(gpu_runtime, graph, scope, P):
    ec.virtual_ranks(graph, scope, P, "hip")


@pytest.mark.parametrize("graph", ec.TINY_RANK_CASES)
def test_eccentricities_four_ranks_with_empty_shards_gpu(gpu_runtime, graph):
    ec.virtual_ranks(graph, "all", 4, "hip")


def test_eccentricities_hub_sort_and_repeated_calls_gpu(gpu_runtime):
    ec.hub_sort_and_repeats(gpu_runtime)


def test_eccentricities_tie_to_traversals_gpu(gpu_runtime):
    ec.ties_to_traversals(gpu_runtime)


def test_eccentricity_refusals_gpu(gpu_runtime):
    ec.refusals(gpu_runtime, pytest)


def test_eccentricities_injected_violation_fails_gpu(gpu_runtime):
    """The device records a violation only where the check sites are compiled
    (the extension's kernels are the unchecked build, whose injection hook is
    empty): the failure path on the device runs through bin/bfs_checked."""
    ec.injected_violation_fails_checked(BFS_CHECKED, [])


@pytest.mark.parametrize("flags", [[], ["--virtual-ranks", "3"]])
def test_cli_eccentricities_gpu(gpu_runtime, tmp_path, flags):
    ec.cli_eccentricities(BFS_BIN, flags, tmp_path)


def test_cli_eccentricities_generated_and_sampled_check_gpu(gpu_runtime):
    ec.cli_generated(BFS_BIN, [])


def test_cli_eccentricities_checked_build_gpu(gpu_runtime):
    """bin/bfs_checked runs --eccentricities clean (every DBFS_DCHECK of
    ecc_kernels.hip live, the backend ending in +checked), and a violation
    recorded after the first bound update fails it naming ecc_kernels."""
    ec.cli_checked_reports(BFS_CHECKED, [])
