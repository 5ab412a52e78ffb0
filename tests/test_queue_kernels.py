"""The queue order (be_sort_pods) and the queue marking (be_launch_fast_queue) against their definitions (tests/queue_cases.py), on
the host emulation — where the sort is sort_key_body under std::stable_sort and the marking is the three kernel bodies in a loop. This
file also holds the case lists to what they claim: the sizes, the ties, the sign and high-digit values, the queue shapes and what the
definition reports for each. The GPU run of the same lists is tests/test_gpu_queue_kernels.py. Every comparison is exact."""
import numpy as np
import pytest

import parity
import queue_cases as qc


@pytest.fixture(scope="module")
def emu():
    return parity.build_emu()


# ------------------------------------------------------------------------------------------------ what the case lists cover
def test_sort_case_list_covers_what_it_claims():
    assert qc.SORT_SIZES == (1, 2, 255, 256, 257, 1025, 4099, 201073) and (qc.SINGLE_BLOCK_LIMIT, qc.ODDEVEN_MERGE_LIMIT, qc.MERGE_SORT_LIMIT) == (1024, 201072, 1 << 20)
    # a size in each of rocprim's ranges below 300,001: one block, odd-even block merge, merge path (the headline problem's); none larger
    assert sum(n <= 1024 for n in qc.SORT_SIZES) == 5 and sum(1024 < n <= 201072 for n in qc.SORT_SIZES) == 2 and sum(201072 < n <= 300001 for n in qc.SORT_SIZES) == 1
    assert len(qc.SORT_CASES) == 7 * 6 + 2 and [f for f, n in qc.SORT_CASES if n == 201073] == ["a", "b"]
    assert 0 in qc.CPUS and 0 in qc.MEMORIES and max(qc.CPUS) > 2**40 and max(qc.MEMORIES) > 2**40 and len(set(qc.CPUS)) == len(set(qc.MEMORIES)) == 5
    assert len(set(qc.CREATIONS)) == 4 and min(qc.CREATIONS) < 0 and max(qc.CREATIONS) > 2**32 and len(set(qc.UID_HIS)) == 3
    a = qc.sort_case("a", 4099)
    assert set(a["requests"][0].tolist()) == set(qc.CPUS) and set(a["requests"][1].tolist()) == set(qc.MEMORIES) and set(a["creation"].tolist()) == set(qc.CREATIONS)
    assert 0.4 < np.mean(a["uid_hi"] >> np.uint64(63)) < 0.6 and 0.4 < np.mean(a["uid_lo"] >> np.uint64(63)) < 0.6
    assert a["expected"].tolist() != list(range(4099)) and sorted(a["expected"].tolist()) == list(range(4099))
    b = qc.sort_case("b", 4099)
    assert len(set(b["requests"][0].tolist())) == len(set(b["requests"][1].tolist())) == len(set(b["creation"].tolist())) == 1 and set(b["uid_hi"].tolist()) == set(qc.UID_HIS)
    c = qc.sort_case("c", 257)
    assert c["expected"].tolist() == list(range(257)) and len(set(c["uid_lo"].tolist())) == 1
    assert qc.sort_case("d-sorted", 257)["expected"].tolist() == list(range(257)) and qc.sort_case("d-reversed", 257)["expected"].tolist() == list(range(256, -1, -1))
    f = qc.sort_case("f", 257)
    assert f["n_rows"] == 257 + 37 and f["requests"].shape == (2, 294) and f["requests"][:, 257:].min() > f["requests"][:, :257].max()
    # every criterion decides some pair alone, in both index orders, with the values that tell a sign or a direction mistake
    assert {p[0] for p in qc.PAIRS} == {"cpu", "memory", "creation", "uid_hi", "uid_lo"}
    assert ("cpu", 2**62, 2**62 - 1) in qc.PAIRS and ("creation", -1, 0) in qc.PAIRS and ("uid_hi", 2**63 - 1, 2**63) in qc.PAIRS and ("uid_lo", 2**63 - 1, 2**63) in qc.PAIRS


def test_marking_case_list_covers_what_it_claims():
    assert set(qc.MARKING_CASES) == set(qc.MARKING_MAX_ACTIVE)
    for name in qc.MARKING_CASES:
        c = qc.marking_case(name)
        e = c["expected"]
        n, nc = len(c["sorted"]), c["n_classes"]
        if qc.MARKING_MAX_ACTIVE[name] is not None:
            assert e["max_active"] == qc.MARKING_MAX_ACTIVE[name], name
        first, last = e["cls_first"].tolist(), e["cls_last"].tolist()
        present = [k for k in range(nc) if first[k] != qc.NOT_PLACED]
        if nc <= 305:   # the counting form of max_active against the definition as it is worded
            live = qc.live_at_first(first, last)
            assert e["max_active"] == (0 if qc.count_skipped(nc, c["count_live"]) else max(live.values())), name
        assert int(np.sum(e["q_class"] >= qc.K_FAST_LAST_BIT)) == len(present), name                     # one last entry per class present
        assert sorted(c["sorted"].tolist()) != c["sorted"].tolist() or n == 1, name                      # the pods are not in row order
        if name.startswith("random-"):
            assert len(c["row_class"]) == n + 11 and nc == 305 and 5 <= nc - len(present) and all(last[k] == 0 for k in range(nc) if k not in present), name
            assert e["max_active"] > (64 if n == 4099 else 8), name       # (the long one needs four rows of class slots)
    assert [len(qc.marking_case(n)["sorted"]) for n in ("one-class-70001", "own-class-4099", "random-4099", "random-255", "random-256", "random-257")] == [70001, 4099, 4099, 255, 256, 257]
    assert qc.marking_case("own-class-4099")["n_classes"] == 4099 and qc.marking_case("nested-257-uncounted")["count_live"] == 0
    assert max(qc.marking_case(n)["n_classes"] for n in qc.MARKING_CASES if n != "classes-32769") <= 4099    # the quadratic count never sees more
    assert qc.count_skipped(64, 1) and not qc.count_skipped(65, 1) and not qc.count_skipped(32768, 1) and qc.count_skipped(32769, 1) and qc.count_skipped(300, 0)


# ------------------------------------------------------------------------------------------------ the product's kernels, emulated
@pytest.mark.parametrize("family,n", qc.SORT_CASES)
def test_queue_order(emu, family, n):
    case = qc.sort_case(family, n)
    qc.check_sort(case, qc.run_sort(emu, case), what=f"family {family}, {n} pods")


@pytest.mark.parametrize("swapped", [False, True])
def test_queue_order_one_criterion_decides(emu, swapped):
    for i, pair in enumerate(qc.PAIRS):
        case = qc.pair_case(i, swapped)
        qc.check_sort(case, qc.run_sort(emu, case), what=f"pair {pair}, swapped {swapped}")


@pytest.mark.parametrize("name", qc.MARKING_CASES)
def test_queue_marking(emu, name):
    case = qc.marking_case(name)
    assert qc.marking_mismatches(qc.run_marking(emu, case), case["expected"]) == [], name
