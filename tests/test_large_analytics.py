"""Components, strongly connected components and eccentricities on graphs
past the kernels' grid caps, on the CPU backend: the cases, references and
literals of large_cases.py proven without a GPU (the CPU backend has no grid
and no slots; test_large_analytics_gpu.py runs the same checks on the device),
and the caps themselves pinned against the sources.

  cc_1m           n = 4096 * 256 + 4097: a second trip of kCcGrid (cc_init, cc_link, cc_compress, cc_hist;
                  on two ranks cc_link_pairs), five of kCcSizeGrid (cc_totals' slots); the hub's row of
                  140 000 entries: a second stride of kCcLongGrid in cc_link_long; a path wholly in the
                  second trip; scoped to that path, ecc_init / ecc_degrees past kEccGrid * 256
  cc_two_largest  two largest components of one size whose labels lie in different trips and slots of
                  cc_totals: the smaller label wins across slots
  cc_star_out     directed, one out-row of 140 000 entries: cc_link_long's second stride without twin entries
  scc_528k        n = 2048 * 256 + 4097: a second trip of kSccGrid (every sweep kernel), three of
                  kSccPivotGrid; two hubs of one degree product in different trips and slots of scc_pivot:
                  the smaller id wins; two 40 000-entry rows on the wave tier; the in-edge routing
  scc_528k_high   the same with the pivot's slot past the first 256 that scc_pivot_finish reads per trip
  scc_tiers       (scc_cases) rows whose one live entry is the lane's last, the wave's first, ...
  tree270k        five trips of kEccSelGrid in ecc_select, a second of kEccGrid * 64 rows in
                  ecc_update<uint8>, of kEccTotalsGrid in ecc_totals; one-byte levels
  deep140k        a second trip of kEccGrid * 32 rows in ecc_update<uint16>; 16-bit levels

The two numpy bounding references take about 30 s of this file's minute."""
import pytest

from distributed_cuda_bfs_amd.parallel.runtime import init_runtime

import large_cases as lc


@pytest.fixture(scope="module")
def rt():
    return init_runtime("cpu")


def test_caps_are_those_of_the_sources():
    lc.caps_match_the_sources()


@pytest.mark.parametrize("graph", list(lc.CC_FACTS))
def test_large_components_references_state_the_facts(graph):
    lc.cc_references_state_the_facts(graph)


@pytest.mark.parametrize("graph", list(lc.CC_FACTS))
def test_large_components_match_references(rt, graph):
    lc.cc_matches_references(rt, graph)


def test_large_components_without_hub_sort(rt):
    lc.cc_matches_references(rt, "cc_1m", hub_sort=False)


def test_large_components_two_ranks():
    lc.cc_two_ranks("cc_1m", "cpu")


@pytest.mark.parametrize("graph", list(lc.SCC_HUBS))
def test_large_strong_components_references_state_the_facts(graph):
    lc.scc_references_state_the_facts(graph)


def test_large_strong_components_defaults_and_in_edges(rt):
    lc.scc_defaults(rt, "scc_528k", in_edges=True)


def test_large_strong_components_pivot_in_a_late_slot(rt):
    lc.scc_defaults(rt, "scc_528k_high")


def test_large_strong_components_forced_form(rt):
    lc.scc_forced(rt)


def test_large_strong_components_two_ranks():
    lc.scc_two_ranks("cpu")


def test_strong_component_tier_positions(rt):
    lc.scc_tier_positions(rt)


@pytest.mark.parametrize("graph", list(lc.TREES))
def test_tree_references_state_the_facts(graph):
    lc.tree_references_state_the_facts(graph)


@pytest.mark.parametrize("graph", list(lc.TREES))
def test_tree_eccentricities_match_references(rt, graph):
    lc.tree_all(rt, graph)


@pytest.mark.parametrize("graph", list(lc.TREES))
def test_tree_diameter_target(rt, graph):
    lc.tree_diameter(rt, graph)


def test_tree_eccentricities_two_ranks():
    lc.tree_two_ranks("tree270k", "cpu")


def test_eccentricities_scoped_to_a_path_of_a_large_graph(rt):
    lc.path_scope(rt)
