"""Device validation and parent trees of a batch (run_batch(validate=True,
parents=True)) on the GPU: the ms_check kernel, count and parent form in one
walk, against the numpy reference; the checks themselves are in
batch_validate_cases.py, the same as on the CPU backend.

  star5000 k64        a row of 5000 entries: many 64-entry column steps, the partial last step, the
                      last group's repeated line; leaves of one entry
  n4097 k130          n no multiple of 64; a second unit of one vertex; 3 passes on one matrix, the
                      last with 2 sources (lanes 2..63 masked)
  rmat13 k63, k64dup  skewed rows around 64 entries; k < 64; two bits on one vertex; a degree-0
                      source on bit 63
  two_components k64  lanes for which half the graph is unreached: no cross edges between components
  path300 k64         16-bit levels, the uint16_t instantiation, after the rerun
  file_chain8 k1      one lane
  fans300 k1, k64     rows of 1, 7, 8, 9, 63, 64, 65, 71, 72, 73, 128 and 129 entries: every boundary
                      of the row walk (64 column ids per step, 8 level lines per group, the last
                      group's repeated line); 16-bit levels
  fans k64            the same rows, one-byte levels
"""
import os

import pytest

import distributed_cuda_bfs_amd as dbfs
from distributed_cuda_bfs_amd.parallel.runtime import run_virtual_ranks

import batch_cases as bc
import batch_validate_cases as vc

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BFS_BIN = os.path.join(REPO, "bin", "bfs")
_bfs_cache = {}


def _bfs(name, rt):
    if name not in _bfs_cache:
        _bfs_cache[name] = dbfs.BFS(bc.bfs_input(name), rt)
    return _bfs_cache[name]


@pytest.mark.parametrize("direction", bc.DIRECTIONS)
@pytest.mark.parametrize("graph,kind", vc.CASES)
def test_batch_validates_clean_gpu(gpu_runtime, graph, kind, direction):
    vc.positive(_bfs(graph, gpu_runtime), graph, kind, direction)


@pytest.mark.parametrize("graph,kind", vc.PARENTS_ONLY_CASES)
def test_parents_without_validate_gpu(gpu_runtime, graph, kind):
    vc.parents_only(_bfs(graph, gpu_runtime), graph, kind)


def test_parents_copied_back_in_chunks_gpu(gpu_runtime):
    vc.parents_chunked(lambda csr: dbfs.BFS(csr, gpu_runtime))


def test_swapped_sources_are_orphans_gpu(gpu_runtime):
    vc.negative_swapped(_bfs("rmat10", gpu_runtime))


@pytest.mark.parametrize("level", [10, -1])
def test_planted_violation_gpu(gpu_runtime, level):
    vc.negative_planted(_bfs("path300", gpu_runtime), level)


@pytest.mark.parametrize("P", [2, 3])
@pytest.mark.parametrize("graph", ["rmat10", "n4097"])
def test_batch_validate_virtual_ranks_gpu(gpu_runtime, graph, P):
    src, body = vc.ranks_body(graph)
    vc.check_ranks(graph, src, run_virtual_ranks(P, body, device="hip"))


def test_argument_errors_gpu(gpu_runtime):
    vc.argument_errors(_bfs("rmat10", gpu_runtime), pytest)


def test_cli_batch_validate_gpu(gpu_runtime):
    vc.check_cli(BFS_BIN, [])
