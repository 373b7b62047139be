"""No-op chains of the device loop on the GPU (chain_guard_cases.py): every HIP
kernel of a mispredicted, outgrown or trailing chain returns at its guard."""
import pytest

import chain_guard_cases as cg

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(cg.OPTION_SETS))
def test_noop_chains_change_nothing_gpu(gpu_runtime, name):
    cg.check_option_set(gpu_runtime, name)


def test_noop_chains_of_every_form_gpu(gpu_runtime):
    cg.check_every_form(gpu_runtime)
