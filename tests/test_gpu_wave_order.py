"""GPU tests of the device forms of the wavefront primitives (csrc/wave.h: ballots, DPP row operations, v_readlane / v_writelane
through m0, ds_bpermute), fast_umin_s, the claim orders in every form a kernel instantiates (pdq_emul.h, run_order.h: LDS with 4-byte
pointers and the 512-wide scan, HBM with sixteen elements per lane, registers, rings) and shift_right16: one wavefront per launch of
tests/emu/wave_order_probe.cpp, the cases of tests/wave_order_cases.py. Every device answer equals its definition and, bit for bit in
every output field, the answer of the host twin. The CPU run of the same cases, which also shows that they reach every path of the
sort, is tests/test_wave_order.py."""
import pytest

import parity
import wave_order_cases as wc
from gpu_support import built  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    p = wc.Probe(parity.build_wave_order("dev"))
    assert p.is_device
    return p


@pytest.fixture(scope="module")
def twin():
    return wc.Probe(parity.build_wave_order("host"))


@pytest.fixture(scope="module")
def go_sorted():
    return {}


@pytest.mark.parametrize("name", list(wc.PART_A) + list(wc.PART_B_PLAIN))
def test_against_definition_and_twin(dev, twin, name):
    run, define = {**wc.PART_A, **wc.PART_B_PLAIN}[name]
    got, want, host = run(dev), define(), run(twin)
    assert len(got) == len(want) == len(host)
    for i, (g, w, h) in enumerate(zip(got, want, host)):
        assert g == w, (name, i, "definition")
        assert g == h, (name, i, "host twin")


@pytest.mark.parametrize("form", wc.MEM_FORMS + wc.REG_FORMS)
def test_sort_single_defect(dev, twin, oracle, go_sorted, form):
    cases = wc.single_defect_cases()
    host = wc.run_sorts(twin, cases, form)
    wc.check_sorts(host, cases, form, oracle, go_sorted)       # only cases that are green on the host twin go to the device
    got = wc.run_sorts(dev, cases, form)
    wc.check_sorts(got, cases, form, oracle, go_sorted)
    assert got == host                                          # keys, claim ids, pos, slow_sorts


@pytest.mark.parametrize("form", (1, 2, 4, 5) + wc.REG_FORMS)
def test_sort_any_array(dev, twin, oracle, go_sorted, form):
    cases = wc.any_array_cases()
    host = wc.run_sorts(twin, cases, form)
    wc.check_sorts(host, cases, form, oracle, go_sorted)
    got = wc.run_sorts(dev, cases, form)
    wc.check_sorts(got, cases, form, oracle, go_sorted)
    assert got == host


def test_register_and_scratch_frame_stacks_agree(dev):
    for cases in (wc.single_defect_cases(), wc.any_array_cases()):
        assert wc.run_sorts(dev, cases, 3) == wc.run_sorts(dev, cases, 7)


@pytest.mark.parametrize("name", list(wc.trace_cases()))
def test_commit_trace(dev, twin, oracle, name):
    ops, forms, (pods, max_claims) = wc.trace_cases()[name]
    got = {}
    for form in forms:
        host = twin.trace(form, ops, pods, max_claims)
        wc.check_trace(host, ops, oracle)
        got[form] = dev.trace(form, ops, pods, max_claims)
        wc.check_trace(got[form], ops, oracle)
        assert got[form] == host, form                          # slow_sorts and the ring heads' wraps among the fields
        assert got[form][3] == got[forms[0]][3], (form, "slow_sorts")
    if name.startswith("rings-wrap"):
        assert got[6][4] > 0 and got[6][5] > 0
