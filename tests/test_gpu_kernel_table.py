"""Which pack kernel a handle launches, on the MI355X (tests/test_kernel_table.py on the host emulation, the same cases:
tests/kernel_table_cases.py): through tests/emu/libksolve_hooks.so — the gfx950 build with -DKSOLVE_TEST_HOOKS, which reports the name
of the kernel the HIP backend launched — every case names the kernel written beside it and equals the oracle. The large-plan
instantiations (u_g1*, u_g2*, p_g1*, p_g2*, g1r4, g2r4) are not reachable with a small problem: their selection is the lookup test's,
and ksolve_test_fast_cold launches g1r1 and u_g2r4 (tests/test_gpu_fast_cold.py)."""
import pytest

import kernel_table_cases as kc
import parity

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hooks():
    from karpenter_amd.scheduling import device_available
    import __graft_entry__
    __graft_entry__.build()
    assert device_available(), "GPU tests need a usable gfx950 device and karpenter_amd/libksolve.so (no CPU fallback)"
    return parity.build_hooks()


@pytest.mark.parametrize("case", kc.lone_cases(), ids=lambda c: c[0])
def test_kernel_of_a_lone_solve(oracle, hooks, case):
    kc.check_lone(oracle, hooks, case)


def test_kernels_of_the_flavour_members_alone(oracle, hooks):
    kc.check_flavour_members_alone(oracle, hooks)


def test_kernels_of_the_flavour_members_in_one_call(oracle, hooks):
    kc.check_flavour_members_many(oracle, hooks)
