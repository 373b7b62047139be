"""The built shard on the GPU: the kernels of csrc/kernels/graph_sort.hip (row
sorts, hub selection and encoding, heads, the non-empty-row view and its
records) and the build kernels of csrc/kernels/graph_kernels.hip (generator,
edge routing, exclusive scan), each table read back from the device and
compared with its numpy definition; the checks are in shard_cases.py, the same
as on the CPU backend.

  ladder      rows of 1, 2, 3 / 63, 64, 65 / 127 .. 257 / 4095, 4096, 4097, 5000 entries: the wave
              sort, the LDS sort and its padding to a power of two, long rows; leaf degrees 0..7
              (key ties: the id tie-break); n = 6021; hub caps None, 100 (42 hubs), 7, 0 (none)
  rmat13      generated on the device; 4472 / 998 / 1 rows per sort; 1716 isolated vertices
  rmat17      more non-isolated vertices than top-down hubs: td_col and hub_col encode differently
  powerlaw    no isolated vertex, two long rows
  n4097       a second unit of one vertex
  d_rmat10    directed: neighbours without out-edges sort last
  tiny5, empty3 at 4 and 2 ranks: shards of one row or none, nnz 0 (a shard without rows once kept
              whatever its allocation held in nz_row_off[0]: the fill kernel's last word writes it)
"""
import pytest

from distributed_cuda_bfs_amd.parallel.runtime import run_virtual_ranks

import shard_cases as sc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("graph,max_hubs", sc.TABLE_CASES)
def test_tables_match_definitions_gpu(gpu_runtime, graph, max_hubs):
    sc.tables_one_rank(gpu_runtime, graph, max_hubs)


@pytest.mark.parametrize("graph,max_hubs", sc.RANK_CASES)
def test_tables_match_definitions_three_ranks_gpu(gpu_runtime, graph, max_hubs):
    sc.check_ranks(graph, max_hubs, 3, run_virtual_ranks(3, sc.ranks_body(graph, max_hubs), device="hip"))


@pytest.mark.parametrize("graph,P", sc.TINY_CASES)
def test_tables_of_tiny_shards_gpu(gpu_runtime, graph, P):
    sc.check_tiny(graph, P, run_virtual_ranks(P, sc.ranks_body(graph), device="hip"))


@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("graph", sc.GENERATED)
def test_generated_shard_matches_build_csr_gpu(gpu_runtime, graph, P):
    shots = run_virtual_ranks(P, sc.ranks_body(graph, hub_sort=False), device="hip")
    part = sc.N.Partition(sc.host_csr(graph).n, P)
    for s in shots:
        sc.check_generated(graph, part, s)


@pytest.mark.parametrize("split", ["rank0", "round_robin"])
def test_from_edges_matches_build_csr_gpu(gpu_runtime, split):
    sc.check_from_edges(3, run_virtual_ranks(3, sc.from_edges_body(split), device="hip"))


@pytest.mark.parametrize("n", sc.SCAN_SIZES)
def test_exclusive_scan_matches_cumsum_gpu(gpu_runtime, n):
    sc.check_scan(gpu_runtime.backend, n)
