"""The queue order (be_sort_pods: ksolve_iota, ksolve_sort_key, rocprim::radix_sort_pairs — its single-block, merge and Onesweep
paths) and the queue marking (be_launch_fast_queue: ksolve_fast_queue, ksolve_fast_overlap, ksolve_fast_mark) on the MI355X against
their definitions (tests/queue_cases.py): the lists of tests/test_queue_kernels.py through the test-only entry points
ksolve_test_sort_pods and ksolve_test_fast_queue of tests/emu/libksolve_hooks.so (the gfx950 build with -DKSOLVE_TEST_HOOKS), one
launch per case. Every comparison is exact. Each case also runs on the host emulation, and the two answers must agree bit for bit in
every field."""
import numpy as np
import pytest

import parity
import queue_cases as qc

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


@pytest.mark.parametrize("family,n", qc.SORT_CASES)
def test_queue_order(hooks, emu, family, n):
    case = qc.sort_case(family, n)
    dev = qc.run_sort(hooks, case)
    qc.check_sort(case, dev, what=f"device, family {family}, {n} pods")
    assert np.array_equal(dev, qc.run_sort(emu, case)), "device and emulation differ"


@pytest.mark.parametrize("swapped", [False, True])
def test_queue_order_one_criterion_decides(hooks, emu, swapped):
    for i, pair in enumerate(qc.PAIRS):
        case = qc.pair_case(i, swapped)
        dev = qc.run_sort(hooks, case)
        qc.check_sort(case, dev, what=f"device, pair {pair}, swapped {swapped}")
        assert np.array_equal(dev, qc.run_sort(emu, case)), ("device and emulation differ", pair)


@pytest.mark.parametrize("name", qc.MARKING_CASES)
def test_queue_marking(hooks, emu, name):
    """(one-class-70001: every thread's atomic min / max lands on the same two words, which the emulation's serial loop cannot lose)"""
    case = qc.marking_case(name)
    dev = qc.run_marking(hooks, case)
    assert qc.marking_mismatches(dev, case["expected"]) == [], name
    assert qc.marking_mismatches(dev, qc.run_marking(emu, case)) == [], "device and emulation differ"
