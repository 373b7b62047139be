"""Device validation and parent trees of a batch (run_batch(validate=True,
parents=True)) on the CPU backend, whose ms_check is the plain-loop form of
the kernel; the checks themselves are in batch_validate_cases.py.

  star5000 k64        a row of 5000 entries (many 64-entry steps, a partial last one), leaves of one entry
  n4097 k130          n no multiple of 64; 3 passes on one matrix, the last with 2 sources
  rmat13 k63, k64dup  skewed rows; k < 64; two bits on one vertex; a degree-0 source on bit 63
  two_components k64  lanes for which half the graph is unreached: no cross edges between components
  path300 k64         16-bit levels after the rerun
  file_chain8 k1      one lane
  fans300 k1, k64     rows of 1, 7, 8, 9, 63, 64, 65, 71, 72, 73, 128 and 129 entries, 16-bit levels
  fans k64            the same rows, one-byte levels
"""
import os

import pytest

import distributed_cuda_bfs_amd as dbfs
from distributed_cuda_bfs_amd.parallel.runtime import init_runtime, run_virtual_ranks

import batch_cases as bc
import batch_validate_cases as vc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BFS_BIN = os.path.join(REPO, "bin", "bfs")
_bfs_cache = {}


def _bfs(name):
    if name not in _bfs_cache:
        _bfs_cache[name] = dbfs.BFS(bc.bfs_input(name), init_runtime("cpu"))
    return _bfs_cache[name]


@pytest.mark.parametrize("direction", bc.DIRECTIONS)
@pytest.mark.parametrize("graph,kind", vc.CASES)
def test_batch_validates_clean(graph, kind, direction):
    vc.positive(_bfs(graph), graph, kind, direction)


@pytest.mark.parametrize("graph,kind", vc.PARENTS_ONLY_CASES)
def test_parents_without_validate(graph, kind):
    vc.parents_only(_bfs(graph), graph, kind)


def test_parents_copied_back_in_chunks():
    vc.parents_chunked(lambda csr: dbfs.BFS(csr, init_runtime("cpu")))


def test_swapped_sources_are_orphans():
    vc.negative_swapped(_bfs("rmat10"))


@pytest.mark.parametrize("level", [10, -1])
def test_planted_violation(level):
    vc.negative_planted(_bfs("path300"), level)


@pytest.mark.parametrize("P", [2, 3])
@pytest.mark.parametrize("graph", ["rmat10", "n4097"])
def test_batch_validate_virtual_ranks(graph, P):
    src, body = vc.ranks_body(graph)
    vc.check_ranks(graph, src, run_virtual_ranks(P, body, device="cpu"))


def test_argument_errors():
    vc.argument_errors(_bfs("rmat10"), pytest)


def test_cli_batch_validate():
    vc.check_cli(BFS_BIN, ["--cpu"])
