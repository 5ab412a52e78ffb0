"""CPU tests of the cursor engine's slow sort (karpenter_amd/csrc/pdq_emul.h, fast_engine.h FastCold::slow_sort): orders of at
most 64 claims are sorted in two vector registers (RegOrder), larger LDS-resident orders scan 512 positions per step (ClaimOrder's
wide scan). Both must leave exactly the permutation ClaimOrder::sort() leaves on arrays in memory: same comparisons, same swaps.

End to end through the host emulation against the oracle, with the lanes of every wave-wide call in both orders; and the two
pieces alone, through tests/emu/small_order_emu.cpp, against the memory form and the one-position-per-lane scans."""
import ctypes
import os
import random
import subprocess

import pytest

import parity
from karpenter_amd import fixtures as fx
from karpenter_amd.scheduling import NewScheduler
from test_device_algorithm import emu  # noqa: F401  (fixture)
from test_device_fuzz_all import emu_reversed  # noqa: F401  (fixture)

HERE = os.path.dirname(os.path.abspath(__file__))

# (pods, types, NodeClaims, at least this many slow sorts): the first solve never has more than 57 claims in flight, the second
# crosses the hand-over from registers to LDS at 64 / 65 with most of its sorts still at 13..49, the third crosses one 512-wide step
SHAPES = [(20000, 500, 57, 3000), (26000, 500, 73, 3000), (3000, 16, 525, 0)]


@pytest.fixture(scope="module")
def wanted(oracle):
    """Per shape, once and on first use: the problem, the oracle's digest and evaluation count, the general engine's slowSorts."""
    cache = {}

    def get(pods, types, claims, lib):
        if pods not in cache:
            prob = fx.config2(pods=pods, n_types=types, seed=42)
            want = oracle.solve(prob)
            assert len(want["newNodeClaims"]) == claims          # the fixture still is the case it is here for
            general = NewScheduler(with_engine(prob, "general"), solver_lib=lib).Solve()
            assert general["counters"]["engine"] == "general" and parity.results_digest(general)[0] == parity.results_digest(want)[0]
            cache[pods] = {"prob": prob, "digest": parity.results_digest(want)[0], "evals": want["counters"]["binEvaluations"], "slow": general["counters"]["slowSorts"]}
        return cache[pods]
    return get


def with_engine(prob, engine):
    return dict(prob, options=dict(prob["options"], engine=engine))


def check_shape(lib, wanted, pods, types, claims, min_slow):
    w = wanted(pods, types, claims, lib)
    assert w["slow"] >= min_slow
    for plan, engine in ((0, "cursor"), (1, "cursor-wide"), (2, "cursor-hbm")):   # every memory plan loads and stores the registers its own way
        got = NewScheduler(with_engine(w["prob"], engine), solver_lib=lib).Solve()
        c = got["counters"]
        assert c["engine"] == "cursor" and c["cursorMemoryPlan"] == plan
        assert len(got["newNodeClaims"]) == claims
        assert parity.results_digest(got)[0] == w["digest"]
        assert c["referenceBinEvaluations"] == w["evals"]
        assert c["slowSorts"] == w["slow"]


@pytest.mark.parametrize("pods,types,claims,min_slow", SHAPES)
def test_small_orders_end_to_end(wanted, emu, pods, types, claims, min_slow):
    check_shape(emu, wanted, pods, types, claims, min_slow)


@pytest.mark.parametrize("pods,types,claims,min_slow", SHAPES)
def test_small_orders_end_to_end_lanes_reversed(wanted, emu_reversed, pods, types, claims, min_slow):
    check_shape(emu_reversed, wanted, pods, types, claims, min_slow)


# ---- the two pieces alone ----
@pytest.fixture(scope="module", params=[False, True], ids=["lanes", "lanes_reversed"])
def small(request, tmp_path_factory):
    src = os.path.join(HERE, "emu", "small_order_emu.cpp")
    lib = str(tmp_path_factory.mktemp("small_order") / "libsmall_order.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared"] + (["-DKS_EMU_REVERSE_LANES"] if request.param else []) + ["-o", lib, src])
    return ctypes.CDLL(lib)


SIZES = [2, 12, 13, 24, 49, 50, 51, 63, 64]


def sort_both(lib, key, ord_, defect, append, mode):
    n = len(key)
    A = ctypes.c_uint32 * n
    km, om, kr, orr = A(), A(), A(), A()
    slow = (ctypes.c_ulonglong * 2)()
    lib.small_order_sort(A(*key), A(*ord_), n, defect, int(append), mode, km, om, kr, orr, slow)
    assert list(kr) == list(km) and list(orr) == list(om), (n, defect, append, mode, key, ord_)
    assert slow[0] == slow[1]
    assert sorted(km) == sorted(key) and sorted(om) == sorted(ord_)
    return list(km), slow[0]


def sorted_patterns(rng, n):
    yield "all equal", [3] * n
    yield "two values", sorted(rng.choice([2, 5]) for _ in range(n))
    yield "two values, split", [2] * (n // 2) + [5] * (n - n // 2)
    yield "staircase", [1 + i // 4 for i in range(n)]
    yield "steep staircase", [1 + 2 * (i // 3) for i in range(n)]
    yield "distinct", [1 + i for i in range(n)]


def test_register_sort_single_defect(small):
    """sort() on "sorted except the claim the last step touched", every defect position of both kinds: the registers end as memory does."""
    rng = random.Random(5)
    slow_total = 0
    for n in SIZES:
        for name, base in sorted_patterns(rng, n):
            ids = list(range(n)); rng.shuffle(ids)
            for p in range(n):                       # a pod added to the claim at p
                key = list(base); key[p] += 1
                out, slow = sort_both(small, key, ids, p, False, 0)
                assert out == sorted(key), (name, n, p)
                slow_total += slow
            key = sorted(base[:n - 1]) + [1]         # a claim appended with its first pod
            out, slow = sort_both(small, key, ids, n - 1, True, 0)
            assert out == sorted(key), (name, n)
            slow_total += slow
    # pdqsort proper ran, not only the single-move shortcuts: with 12 < n < 50 every defect that leaves a descent does, and in the
    # all-equal pattern alone that is every p < n - 1 at n = 13, 24 and 49
    assert slow_total >= 12 + 23 + 48


def test_register_sort_any_permutation(small):
    """pdqsort() itself on arrays that are not one move from sorted (the single-move shortcuts of sort() assume they are): every piece of
    the algorithm — ninther, reversal, partialInsertionSort proper, partitionEqual, breakPatterns, heapsort — compares and swaps alike."""
    rng = random.Random(6)
    for n in SIZES:
        ids = list(range(n))
        cases = [list(range(n, 0, -1)), [i % 5 for i in range(n)], [min(i, n - 1 - i) for i in range(n)], [(i * 7919) % 3 for i in range(n)],
                 [n - i if i % 2 else i for i in range(n)], [1] * (n - 1) + [0], sorted(range(n), key=lambda i: (i % 8, i))]
        for _ in range(40):
            hi = rng.choice([2, 4, n, 1000])
            cases.append([rng.randrange(hi) for _ in range(n)])
        for key in cases:
            rng.shuffle(ids)
            for defect in (-1, rng.randrange(n)):
                out, _ = sort_both(small, key, ids, defect, False, 1)
                if n <= 12:
                    assert out == sorted(key)   # (above 12 the outermost call believes its caller's `defect`: only the sameness is the point)


def test_wide_scans(small):
    """ClaimOrder's 512-wide scans against the scans of one position per lane: every predicate pdqsort uses, answers at the first and last
    element, at piece (8) and step (512) boundaries and nowhere, ranges that start and end anywhere."""
    rng = random.Random(7)
    out = (ctypes.c_int * 2)()
    checked = 0
    for n in (65, 511, 512, 513, 1031):
        pad = (n + 7) // 8 * 8
        K = ctypes.c_uint16 * (pad + 8)
        raw = K()
        off = (-ctypes.addressof(raw) % 16) // 2      # 16-byte aligned start inside the buffer
        keys = (ctypes.c_uint16 * pad).from_buffer(raw, off * 2)
        assert ctypes.addressof(keys) % 16 == 0
        marks = sorted({0, 1, 7, 8, 9, 63, 64, 65, 255, 256, 504, 511, 512, 513, 519, 520, 1023, 1024, 1025, n - 2, n - 1} & set(range(n)))
        ranges = [(0, n), (1, n), (0, n - 1), (3, n - 3), (8, n), (0, 8), (7, 9), (5, 5), (n, n), (n // 2, n // 2 + 1)]
        ranges += [(512, n), (0, 512), (511, 513), (513, n)] if n > 513 else []
        ranges += [tuple(sorted((rng.randrange(n + 1), rng.randrange(n + 1)))) for _ in range(6)]

        def check(op, v):
            nonlocal checked
            for lo, hi in ranges:
                if op == 4 and lo < 1:
                    lo = 1                             # a descent needs a position below
                    if hi < lo:
                        continue
                small.small_order_scan(keys, n, op, lo, hi, v, out)
                assert out[0] == out[1], (n, op, lo, hi, v, out[0], out[1])
                checked += 1

        for j in range(pad):
            keys[j] = 0xFFFF if j >= n else 10         # (past n: whatever the array holds there, it is masked)
        for op in (0, 1, 2, 3):                        # none / all
            for v in (0, 10, 11, 20):
                check(op, v)
        check(4, 0)
        for m in marks:                                # exactly one answer, at m
            for j in range(n):
                keys[j] = 10
            keys[m] = 20
            check(0, 15); check(1, 10); check(0, 20)
            keys[m] = 5
            check(2, 5); check(3, 10); check(2, 7)
            if m >= 1:
                check(4, 0)                            # the one descent is at m
            for j in range(n):                         # a step at m: answers on both sides of it
                keys[j] = 10 if j < m else 20
            for op in (0, 1, 2, 3):
                for v in (10, 15, 20):
                    check(op, v)
        for _ in range(20):                            # arbitrary keys
            top = rng.choice([2, 3, 50, 60000])
            for j in range(n):
                keys[j] = rng.randrange(top)
            for op in (0, 1, 2, 3):
                check(op, rng.randrange(top + 1))
            check(4, 0)
    assert checked > 10000
