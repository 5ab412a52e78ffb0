"""The static (class, node) rows (ksolve_node_dead0: a lane per node, one ballot per class, class chunks of 32, a clamped tail block)
on the MI355X against their definition (tests/node_row_cases.py): the lists of tests/test_node_rows.py through the test-only entry
point ksolve_test_node_dead0 of tests/emu/libksolve_hooks.so (the gfx950 build with -DKSOLVE_TEST_HOOKS) — the class records laid out
by ksolve_class_gather, one launch of the kernel per table. Every comparison is exact, bits past the last node included. Each table
is also computed on the host emulation, and the two must agree bit for bit."""
import numpy as np
import pytest

import node_row_cases as nr
import parity

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hooks():
    from karpenter_amd.scheduling import device_available
    import __graft_entry__
    __graft_entry__.build()
    assert device_available(), "GPU tests need a usable gfx950 device and karpenter_amd/libksolve.so (no CPU fallback)"
    return parity.build_hooks()


@pytest.fixture(scope="module")
def emu():
    return parity.build_emu()


@pytest.mark.parametrize("case", nr.GRID, ids=nr.grid_id)
def test_generated_problems(hooks, emu, case):
    assert np.array_equal(nr.run_generated(hooks, case), nr.run_generated(emu, case)), "device and emulation differ"


@pytest.mark.parametrize("e0,k0", nr.POSITIONS)
def test_single_differences(hooks, emu, e0, k0):
    dev, host = nr.run_single_differences(hooks, e0, k0), nr.run_single_differences(emu, e0, k0)
    assert len(dev) == len(host) == 1 + len(nr.CHANGES)
    for name, d, h in zip(["base"] + list(nr.CHANGES), dev, host):
        assert np.array_equal(d, h), ("device and emulation differ", name)


def test_position_independence(hooks, emu):
    assert np.array_equal(nr.run_positions(hooks), nr.run_positions(emu)), "device and emulation differ"
