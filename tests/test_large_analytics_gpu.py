"""cc_kernels.hip, scc_kernels.hip and ecc_kernels.hip past their grid caps on
the GPU, with the shipped launch configuration: every grid-stride loop takes a
second trip, and the "slots, then one workgroup" reductions merge slots that
accumulated over more than one.  The checks are large_cases.py's, the same as
on the CPU backend; test_large_analytics.py pins the caps against the sources.

  cc_1m           n = 4096 * 256 + 4097 = 1 052 673 > kCcGrid * 256: cc_init, cc_link, cc_compress and
                  cc_hist take a second trip, cc_totals five (kCcSizeGrid * 256 = 262 144) before
                  cc_totals_finish merges its 1024 slots; the hub's 140 000-entry row, less the sampled
                  form's 2 or not, is past kCcLongGrid * 256 = 131 072: a second stride of cc_link_long;
                  a 200-vertex path wholly in the second trip; sample_entries 2 and 0, hub_sort off; on
                  two ranks cc_link_pairs hooks 1 052 673 pairs per peer
  cc_two_largest  two largest components of 5000 vertices, labels 300 000 and 600 000 in different trips
                  and slots of cc_totals: the smaller label on a size tie, across slots
  cc_star_out     directed: one out-row of 140 000 entries and no twin entries, so every hook of
                  cc_link_long's second stride is made there or nowhere (an undirected graph stores each
                  edge in both rows: a hook left out of the long row is made from the leaf's)
  scc_528k        n = 2048 * 256 + 4097 = 528 385 > kSccGrid * 256: every sweep kernel takes a second
                  trip, scc_pivot three (kSccPivotGrid * 256); hubs 1000 and 400 000 have one degree
                  product in different trips and slots: the smaller id, across slots; their 40 000-entry
                  rows on the wave tier of scc_row_any and scc_row_min; the forced form sweeps whole-row
                  minima and closures over 6 rounds; graph_kernels.hip's in-edge routing at this size
  scc_528k_high   the same with hubs 200 000 and 400 000: the pivot's slot (781) and the other's (538) are
                  both past the 256 slots scc_pivot_finish's threads read on their first trip
  scc_tiers       rows of 32, 33, 96, 97, 160 entries whose one live entry is the lane's last, the wave's
                  first, a full step's last, a partial step's first, the last: read back and asserted
  tree270k        n = 270 001: ecc_select takes five trips per workgroup (kEccSelGrid * 256 = 65 536)
                  with an LDS top-K that is full after the first; ecc_update<uint8> a second trip
                  (kEccGrid * 64 rows), ecc_totals a second (kEccTotalsGrid * 256); the passes, sources
                  and bounds must be the numpy loop's, which a wrong selection changes
  deep140k        n = 140 001, eccentricities up to 321: ecc_update<uint16> takes a second trip
                  (kEccGrid * 32 rows)
  cc_1m, scoped   to the path's label: ecc_init, ecc_degrees (kEccGrid * 256), ecc_select, ecc_update and
                  ecc_totals with 200 of 1 052 673 vertices in scope, all in the last trip
"""
import pytest

import large_cases as lc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("graph", list(lc.CC_FACTS))
def test_large_components_match_references_gpu(gpu_runtime, graph):
    lc.cc_matches_references(gpu_runtime, graph)


def test_large_components_without_hub_sort_gpu(gpu_runtime):
    lc.cc_matches_references(gpu_runtime, "cc_1m", hub_sort=False)


def test_large_components_two_ranks_gpu(gpu_runtime):
    lc.cc_two_ranks("cc_1m", "hip")


def test_large_strong_components_defaults_and_in_edges_gpu(gpu_runtime):
    lc.scc_defaults(gpu_runtime, "scc_528k", in_edges=True)


def test_large_strong_components_pivot_in_a_late_slot_gpu(gpu_runtime):
    lc.scc_defaults(gpu_runtime, "scc_528k_high")


def test_large_strong_components_forced_form_gpu(gpu_runtime):
    lc.scc_forced(gpu_runtime)


def test_large_strong_components_two_ranks_gpu(gpu_runtime):
    lc.scc_two_ranks("hip")


def test_strong_component_tier_positions_gpu(gpu_runtime):
    lc.scc_tier_positions(gpu_runtime)


@pytest.mark.parametrize("graph", list(lc.TREES))
def test_tree_eccentricities_match_references_gpu(gpu_runtime, graph):
    lc.tree_all(gpu_runtime, graph)


@pytest.mark.parametrize("graph", list(lc.TREES))
def test_tree_diameter_target_gpu(gpu_runtime, graph):
    lc.tree_diameter(gpu_runtime, graph)


def test_tree_eccentricities_two_ranks_gpu(gpu_runtime):
    lc.tree_two_ranks("tree270k", "hip")


def test_eccentricities_scoped_to_a_path_of_a_large_graph_gpu(gpu_runtime):
    lc.path_scope(gpu_runtime)
