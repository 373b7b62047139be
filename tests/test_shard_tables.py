"""The built shard on the CPU backend: every derived table against its numpy
definition (distributed_cuda_bfs_amd.utils.shard_reference), the generator and
from_edges against build_csr, the exclusive scan against np.cumsum.  The
checks are in shard_cases.py, the same as on the GPU
(test_shard_tables_gpu.py, whose docstring says what each graph pins)."""
import pytest

from distributed_cuda_bfs_amd.parallel.runtime import init_runtime, run_virtual_ranks

import shard_cases as sc


@pytest.fixture(scope="module")
def rt():
    return init_runtime("cpu")


@pytest.mark.parametrize("graph,max_hubs", sc.TABLE_CASES)
def test_tables_match_definitions(rt, graph, max_hubs):
    sc.tables_one_rank(rt, graph, max_hubs)


@pytest.mark.parametrize("graph,max_hubs", sc.RANK_CASES)
def test_tables_match_definitions_three_ranks(graph, max_hubs):
    sc.check_ranks(graph, max_hubs, 3, run_virtual_ranks(3, sc.ranks_body(graph, max_hubs), device="cpu"))


@pytest.mark.parametrize("graph,P", sc.TINY_CASES)
def test_tables_of_tiny_shards(graph, P):
    sc.check_tiny(graph, P, run_virtual_ranks(P, sc.ranks_body(graph), device="cpu"))


@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("graph", sc.GENERATED)
def test_generated_shard_matches_build_csr(graph, P):
    shots = run_virtual_ranks(P, sc.ranks_body(graph, hub_sort=False), device="cpu")
    part = sc.N.Partition(sc.host_csr(graph).n, P)
    for s in shots:
        sc.check_generated(graph, part, s)


@pytest.mark.parametrize("split", ["rank0", "round_robin"])
def test_from_edges_matches_build_csr(split):
    sc.check_from_edges(3, run_virtual_ranks(3, sc.from_edges_body(split), device="cpu"))


@pytest.mark.parametrize("n", sc.SCAN_SIZES)
def test_exclusive_scan_matches_cumsum(rt, n):
    sc.check_scan(rt.backend, n)
