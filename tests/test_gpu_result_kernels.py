"""The finalize kernel (ksolve_finalize over go_sort.h, with ksolve_claim_gather behind a slot_of), the fast engines' effective
allocatable (ksolve_fast_eff_alloc) and the cursor engine's claim records and scatter (ksolve_fast_records, ksolve_fast_scatter) on the
MI355X against their definitions (tests/result_cases.py): the lists of tests/test_result_kernels.py through the test-only entry points
ksolve_test_finalize, ksolve_test_eff_alloc and ksolve_test_fast_records of tests/emu/libksolve_hooks.so (the gfx950 build with
-DKSOLVE_TEST_HOOKS). Every comparison is exact. Each case also runs on the host emulation, and the two answers must agree bit for bit in
every downloaded word, prices and packed records included."""
import numpy as np
import pytest

import parity
import result_cases as rc

pytestmark = pytest.mark.gpu

ALL_FIELDS = rc.FINALIZE_FIELDS + ("rec_hot", "rec_cold", "g_hot", "g_cold", "g_reserved")


@pytest.fixture(scope="module")
def hooks(oracle):
    from karpenter_amd.scheduling import device_available
    import __graft_entry__
    __graft_entry__.build()
    assert device_available(), "GPU tests need a usable gfx950 device and karpenter_amd/libksolve.so (no CPU fallback)"
    rc.use_oracle(oracle)
    return parity.build_hooks()


@pytest.fixture(scope="module")
def emu():
    return parity.build_emu()


def same(dev, host, fields=ALL_FIELDS):
    return rc.mismatches(dev, host, [f for f in fields if f in dev or f in host])


@pytest.mark.parametrize("name", list(rc.FINALIZE_CASES))
def test_finalize(oracle, hooks, emu, name):
    P, want = rc.finalize_problem(name), rc.finalize_expected(oracle, name)
    dev = rc.run_finalize(hooks, P)
    assert rc.mismatches(dev, want) == [], name
    assert same(dev, rc.run_finalize(emu, P)) == [], "device and emulation differ"
    assert rc.mismatches(rc.run_finalize(hooks, P, poison=rc.POISONS[1]), dev) == [], "the answers depend on the poison"


def test_finalize_reservation_tables_without_held_column(oracle, hooks, emu):
    import copy
    P = copy.deepcopy(rc.finalize_problem("255x51"))
    dev = rc.run_finalize(hooks, P, c_reserved=False)
    assert same(dev, rc.run_finalize(emu, P, c_reserved=False)) == [], "device and emulation differ"
    for s in P["slots"]:
        s["held"] = set()
    assert rc.mismatches(dev, rc.expected_finalize(oracle, P)) == []


@pytest.mark.parametrize("kind", ["identity", "permutation", "duplicates"])
def test_finalize_behind_slot_of(oracle, hooks, emu, kind):
    base = rc.finalize_problem("slots")
    P = rc.with_slots(base, kind)
    want = rc.expected_finalize(oracle, P)
    for poison in rc.POISONS:
        dev = rc.run_finalize(hooks, P, poison=poison)
        assert rc.mismatches(dev, want) == [], (kind, hex(poison))
        assert rc.gather_mismatches(P, dev) == [], (kind, hex(poison))
        assert same(dev, rc.run_finalize(emu, P, poison=poison)) == [], "device and emulation differ"
    if kind != "duplicates":
        assert rc.mismatches(dev, rc.run_finalize(hooks, base, poison=rc.POISONS[1])) == [], "the answers depend on where the records lie"


def test_finalize_single_differences(oracle, hooks, emu):
    base = rc.single_base()
    want0 = rc.expected_finalize(oracle, base)
    assert rc.mismatches(rc.run_finalize(hooks, base), want0) == []
    for name, Q, may, must in rc.single_changes(base):
        want = rc.expected_finalize(oracle, Q)
        diff = rc.mismatches(want, want0)
        assert diff and {c for _, c in diff} == {0} and {k for k, _ in diff} <= may and must in {k for k, _ in diff}, (name, diff)
        dev = rc.run_finalize(hooks, Q)
        assert rc.mismatches(dev, want) == [], name
        assert same(dev, rc.run_finalize(emu, Q)) == [], "device and emulation differ"


@pytest.mark.parametrize("name", list(rc.EFF_CASES))
def test_eff_alloc(hooks, emu, name):
    E = rc.eff_case(name)
    dev = rc.run_eff(hooks, E)
    assert np.array_equal(dev, rc.expected_eff(E)), name
    assert np.array_equal(dev, rc.run_eff(emu, E)), "device and emulation differ"


@pytest.mark.parametrize("name", list(rc.RECORD_CASES))
def test_fast_records(hooks, emu, name):
    R = rc.records_case(name)
    dev = rc.run_records(hooks, R)
    assert rc.record_mismatches(dev, rc.expected_records(R)) == [], name
    host = rc.run_records(emu, R)
    assert [k for k in ("c_hot", "c_cold") + rc.RECORD_COLS if not np.array_equal(dev[k], host[k])] == [], "device and emulation differ"


@pytest.mark.parametrize("name", ["63-claims-64-types", "65-claims-130-types", "no-limits"])
def test_records_feed_finalize(oracle, hooks, emu, name):
    R = rc.records_case(name)
    got = rc.run_records(hooks, R)
    P = rc.chain_problem(R, got)
    want = rc.expected_finalize(oracle, P)
    for poison in rc.POISONS:
        dev = rc.run_finalize(hooks, P, poison=poison)
        assert rc.mismatches(dev, want) == [], (name, hex(poison))
        assert same(dev, rc.run_finalize(emu, P, poison=poison)) == [], "device and emulation differ"
