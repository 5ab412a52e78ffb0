"""CPU tests of the wavefront primitives (csrc/wave.h), fast_umin_s, the claim orders in every form a kernel instantiates (pdq_emul.h,
run_order.h) and shift_right16, each alone against its definition (tests/wave_order_cases.py), on the host twins of
tests/emu/wave_order_probe.cpp with the lanes of every wave-wide call in both orders. The same cases run on the device in
tests/test_gpu_wave_order.py; this file also shows that the cases reach every path of the sort (the host twin's counters)."""
import pytest

import parity
import wave_order_cases as wc


@pytest.fixture(scope="module", params=["host", "host_reversed"], ids=["lanes", "lanes_reversed"])
def twin(request):
    return wc.Probe(parity.build_wave_order(request.param))


@pytest.fixture(scope="module")
def go_sorted():
    return {}     # keys -> the oracle's permutation, shared by the forms


@pytest.mark.parametrize("name", list(wc.PART_A) + list(wc.PART_B_PLAIN))
def test_against_definition(twin, name):
    run, define = {**wc.PART_A, **wc.PART_B_PLAIN}[name]
    got, want = run(twin), define()
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (name, i)


@pytest.mark.parametrize("form", wc.MEM_FORMS + wc.REG_FORMS)
def test_sort_single_defect(twin, oracle, go_sorted, form):
    cases = wc.single_defect_cases()
    wc.check_sorts(wc.run_sorts(twin, cases, form), cases, form, oracle, go_sorted)


@pytest.mark.parametrize("form", (1, 2, 4, 5) + wc.REG_FORMS)
def test_sort_any_array(twin, oracle, go_sorted, form):
    cases = wc.any_array_cases()
    wc.check_sorts(wc.run_sorts(twin, cases, form), cases, form, oracle, go_sorted)


def test_register_and_scratch_frame_stacks_agree(twin):
    for cases in (wc.single_defect_cases(), wc.any_array_cases()):
        assert wc.run_sorts(twin, cases, 3) == wc.run_sorts(twin, cases, 7)


def test_every_form_counts_the_same_slow_sorts(twin):
    cases = [c for c in wc.single_defect_cases() if len(c[0]) <= 64 and sum(c[0]) <= 20000]
    slow = {form: [r[3] for r in wc.run_sorts(twin, cases, form)] for form in wc.MEM_FORMS + wc.REG_FORMS}
    assert all(s == slow[1] for s in slow.values()) and sum(slow[1]) > 0


def test_cases_reach_every_path_of_the_sort(twin):
    """From the calls pdqsort makes on its accessor (probe_sort_paths): the two lists together, and the part of them RegOrder can hold,
    take heap_sort, partition_equal, partition, partialInsertionSort proper, reverse_range, break_patterns, both rotations,
    rotate_left with same_keys and the binary searches."""
    names = ["slow", "heap_sort", "partition_equal", "partition", "partial_insertion_sort", "reverse_range", "break_patterns", "rotate_right", "rotate_left", "same_keys", "binary search"]
    total, small = [0] * 11, [0] * 11
    for key, ids, defect, app, mode in wc.single_defect_cases() + wc.any_array_cases():
        c = twin.sort_paths(key, ids, defect, app, mode)
        total = [a + b for a, b in zip(total, c)]
        if len(key) <= 64:
            small = [a + b for a, b in zip(small, c)]
    assert all(total), dict(zip(names, total))
    assert all(small), dict(zip(names, small))      # (heap_sort at 64 claims: tests/golden/pdqsort_killer_64.json)


@pytest.mark.parametrize("name", list(wc.trace_cases()))
def test_commit_trace(twin, oracle, name):
    ops, forms, (pods, max_claims) = wc.trace_cases()[name]
    got = {form: twin.trace(form, ops, pods, max_claims) for form in forms}
    for form, g in got.items():
        wc.check_trace(g, ops, oracle)
        assert g[3] == got[forms[0]][3], (form, "slow_sorts")
    if name.startswith("rings-wrap"):
        assert got[6][4] > 0 and got[6][5] > 0      # ring heads stepped across the end of their ring in both directions
