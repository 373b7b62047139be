"""No-op chains of the device loop on the CPU backend (chain_guard_cases.py): the
CPU kernels test the same ChainGuard::live as the HIP ones."""
import pytest

from distributed_cuda_bfs_amd.parallel.runtime import init_runtime

import chain_guard_cases as cg


@pytest.fixture(scope="module")
def rt():
    return init_runtime("cpu")


@pytest.mark.parametrize("name", list(cg.OPTION_SETS))
def test_noop_chains_change_nothing(rt, name):
    cg.check_option_set(rt, name)


def test_noop_chains_of_every_form(rt):
    cg.check_every_form(rt)
