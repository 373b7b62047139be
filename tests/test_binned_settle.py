"""Binned levels that settle and finish in their apply pass, on the CPU backend
(binned_settle_cases.py): CpuBackend::td_binned has the same duties as the HIP
apply kernel -- levels, unit statistics, totals, the finish, the folded scan --
and the same DeviceLoop::emit_binned drives it."""
import pytest

from distributed_cuda_bfs_amd.parallel.runtime import init_runtime

import binned_settle_cases as bs


@pytest.fixture(scope="module")
def rt():
    return init_runtime("cpu")


@pytest.mark.parametrize("name,mode,narrow", bs.params())
def test_binned_settle(rt, name, mode, narrow):
    bs.check_case(rt, name, mode, narrow)
