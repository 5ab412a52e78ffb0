"""Cases and definitions for the direct tests of the wavefront primitives (karpenter_amd/csrc/wave.h), fast_umin_s, the claim orders
(pdq_emul.h, run_order.h) and shift_right16, through tests/emu/wave_order_probe.cpp (TEST INFRASTRUCTURE). Used by
tests/test_wave_order.py (the host twins, both lane orders), tests/test_gpu_wave_order.py (one wavefront on the device) and
tests/tools/order_mutations.py.

The definitions below work on plain Python ints and lists (numpy only carries arrays to the library and, for the scans, finds the
first / last true entry of a slice); they share nothing with the product. The definition of a sort is the oracle's restatement of
Go's sort.Slice (`sort_by_key`, `order_trace`).

The contract every case keeps, as the engines do: all 64 lanes of the one wavefront are active at every call; arguments the
signature takes as wave-uniform (ranges, lanes to write or broadcast, counts, keys to compare with) are wave-uniform; a predicate may
be evaluated for any position of [lo, hi) and for none outside; `first_descent` is asked with lo >= 1; claim ids are 0 .. n-1; the
16-bit orders hold counts below 65,536; RegOrder holds at most 64 claims; RunOrder's rings are laid out for (pods, max claims) that
cover the case. Every array a predicate of Part A reads has 512 readable entries of padding on both sides that hold "true": a
predicate evaluated outside its range shows as a wrong answer, never as a fault.

Each group is (cases, run(probe) -> answers, define(oracle) -> answers); answers are plain lists / tuples compared with ==."""
import ctypes
import functools
import json
import os
import random

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
M32, M64 = (1 << 32) - 1, (1 << 64) - 1
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
POISON64 = 0xA5A5A5A5A5A5A5A5
KCAP = 4104


def _p(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t))


def _i32(x): return np.ascontiguousarray(x, dtype=np.int32)
def _u32(x): return np.ascontiguousarray(x, dtype=np.uint32)
def _u64(x): return np.ascontiguousarray(x, dtype=np.uint64)
def _u16(x): return np.ascontiguousarray(x, dtype=np.uint16)


def signed64(x):
    x &= M64
    return x - (1 << 64) if x >> 63 else x


class Probe:
    """ctypes driver of one build of the probe. Every call asserts the entry point's status: 0, nothing refused, no runtime error."""

    def __init__(self, path):
        self.lib = ctypes.CDLL(path)
        self.is_device = bool(self.lib.probe_is_device())

    def call(self, name, *args):
        st = getattr(self.lib, name)(*args)
        assert st == 0, f"{name}: status {st} (-1: the case was refused before any launch; > 0: runtime error)"

    def ballots(self, pats):
        w = self.lib.probe_ballot_out_words()
        out = np.full(len(pats) * w, POISON64, dtype=np.uint64)
        self.call("probe_ballots", _p(_u32(pats), ctypes.c_uint32), len(pats), _p(out, ctypes.c_ulonglong))
        return [[int(x) for x in out[c * w:(c + 1) * w]] for c in range(len(pats))]

    def find(self, cases):
        cs = _i32(cases)
        out = np.full(len(cases), -99, dtype=np.int32)
        self.call("probe_find", _p(cs, ctypes.c_int), len(cases), _p(out, ctypes.c_int))
        return [int(x) for x in out]

    def reduce(self, cases, vals):
        cs, v = _i32(cases), _u64(vals)
        out = np.full(len(cases) * 3, POISON64, dtype=np.uint64)
        self.call("probe_reduce", _p(cs, ctypes.c_int), len(cases), _p(v, ctypes.c_ulonglong), len(v), _p(out, ctypes.c_ulonglong))
        return [tuple(int(x) for x in out[3 * c:3 * c + 3]) for c in range(len(cases))]

    def for_n(self, ns):
        stride = self.lib.probe_for_n_stride()
        cnt = np.zeros(len(ns) * stride, dtype=np.uint32)
        self.call("probe_for_n", _p(_i32(ns), ctypes.c_int), len(ns), _p(cnt, ctypes.c_uint32))
        return [[int(x) for x in cnt[c * stride:(c + 1) * stride]] for c in range(len(ns))]

    def copy8(self, src, n):
        a, b = np.full(1536, 0xEEEE, dtype=np.uint16), np.full(1536, 0xEEEE, dtype=np.uint16)
        self.call("probe_copy8", _p(_u16(src), ctypes.c_uint16), _p(a, ctypes.c_uint16), _p(b, ctypes.c_uint16), n)
        return [int(x) for x in a], [int(x) for x in b]

    def store_leader(self, g):
        gg, out = _u32(g), np.full(192, 0xA5A5A5A5, dtype=np.uint32)
        self.call("probe_store_leader", _p(gg, ctypes.c_uint32), _p(out, ctypes.c_uint32))
        return [int(x) for x in gg], [int(x) for x in out]

    def lane_set(self, idx, val, g):
        gg = _u32(g)
        a, b, lds = (np.full(64, 0xA5A5A5A5, dtype=np.uint32) for _ in range(3))
        v = np.full(64, POISON64, dtype=np.uint64)
        self.call("probe_lane_set", _p(_i32(idx), ctypes.c_int), _p(_u64(val), ctypes.c_ulonglong), _p(gg, ctypes.c_uint32), _p(a, ctypes.c_uint32), _p(b, ctypes.c_uint32),
                  _p(v, ctypes.c_ulonglong), _p(lds, ctypes.c_uint32))
        return tuple([int(x) for x in t] for t in (a, b, v, lds, gg))

    def bcast(self, val):
        a, b = np.full(64, 0xA5A5A5A5, dtype=np.uint32), np.full(64, POISON64, dtype=np.uint64)
        self.call("probe_bcast", _p(_u64(val), ctypes.c_ulonglong), _p(a, ctypes.c_uint32), _p(b, ctypes.c_ulonglong))
        return [int(x) for x in a], [int(x) for x in b]

    def shuffle(self, pats, val):
        n = len(pats)
        a, b = np.full(64 * n, 0xA5A5A5A5, dtype=np.uint32), np.full(64 * n, POISON64, dtype=np.uint64)
        self.call("probe_shuffle", _p(_i32(pats), ctypes.c_int), n, _p(_u64(val), ctypes.c_ulonglong), _p(a, ctypes.c_uint32), _p(b, ctypes.c_ulonglong))
        return [([int(x) for x in a[64 * i:64 * i + 64]], [int(x) for x in b[64 * i:64 * i + 64]]) for i in range(n)]

    def sort(self, form, cases, n_pods=0, max_claims=0):
        """cases: (key, ord, defect, append, mode) -> per case (key, ord, pos or None, slow_sorts), one launch for all of them"""
        keys = [k for c in cases for k in c[0]]
        ords = [o for c in cases for o in c[1]]
        table, off = [], 0
        for key, _, defect, app, mode in cases:
            table.append((off, len(key), defect, int(app), mode)); off += len(key)
        ko, oo, po = (np.full(off, 0xEEEEEEEE, dtype=np.uint32) for _ in range(3))
        slow = np.full(len(cases), POISON64, dtype=np.uint64)
        self.call("probe_sort", form, _p(_u32(keys), ctypes.c_uint32), _p(_u32(ords), ctypes.c_uint32), off, _p(_i32(table), ctypes.c_int), len(cases),
                  _p(ko, ctypes.c_uint32), _p(oo, ctypes.c_uint32), _p(po, ctypes.c_uint32), _p(slow, ctypes.c_ulonglong), n_pods, max_claims)
        ko, oo, po = ko.tolist(), oo.tolist(), po.tolist()
        return [(ko[o:o + n], oo[o:o + n], po[o:o + n] if form in (4, 6) else None, int(slow[c])) for c, (o, n, _, _, _) in enumerate(table)]

    def trace(self, form, ops, n_pods=0, max_claims=0):
        """-> (keys, claim ids, pos or None, slow_sorts, ring heads wrapped upwards, downwards)"""
        ko, oo, po = (np.full(KCAP, 0xEEEEEEEE, dtype=np.uint32) for _ in range(3))
        res = np.full(4, POISON64, dtype=np.uint64)
        self.call("probe_trace", form, _p(_i32(ops), ctypes.c_int), len(ops), _p(ko, ctypes.c_uint32), _p(oo, ctypes.c_uint32), _p(po, ctypes.c_uint32), _p(res, ctypes.c_ulonglong), n_pods, max_claims)
        n = int(res[0])
        assert n == sum(1 for o in ops if o < 0)
        return (ko[:n].tolist(), oo[:n].tolist(), po[:n].tolist() if form in (4, 6) else None, int(res[1])) + ((int(res[2]), int(res[3])) if form == 6 else (0, 0))

    def scans(self, keys, n, cases):
        L = self.lib.probe_scan_len()
        k = np.full(L, 0xFFFF, dtype=np.uint16); k[:len(keys)] = keys
        out = np.full(2 * len(cases), -99, dtype=np.int32)
        self.call("probe_scans", _p(k, ctypes.c_uint16), n, _p(_i32(cases), ctypes.c_int), len(cases), _p(out, ctypes.c_int))
        return out.reshape(-1, 2).tolist()

    def shift(self, arr, cases):
        L = self.lib.probe_shift_len()
        out = np.full(L * len(cases), 0xEEEE, dtype=np.uint16)
        self.call("probe_shift", _p(_u16(arr), ctypes.c_uint16), _p(_i32(cases), ctypes.c_int), len(cases), _p(out, ctypes.c_uint16))
        return out.reshape(len(cases), L).tolist()

    def sort_paths(self, key, ord_, defect, app, mode):
        assert not self.is_device
        c = (ctypes.c_ulonglong * 11)()
        k, o = _u32(list(key)), _u32(list(ord_))
        self.call("probe_sort_paths", _p(k, ctypes.c_uint32), _p(o, ctypes.c_uint32), len(key), defect, int(app), mode, c)
        return list(c)


# ============================================================ Part A ============================================================
def lanes_mask(lanes):
    return sum(1 << l for l in lanes)


@functools.lru_cache(None)
def ballot_cases():
    rng = random.Random(101)
    sets = [[], list(range(64)), [0], [63], [31, 32]]
    pats = [[0xFF if l in s else 0 for l in range(64)] for s in sets]
    pats += [[(0x01 << (l % 8)) for l in range(64)], [(l * 37 + 5) & 0xFF for l in range(64)]]          # every predicate its own lanes
    pats += [[rng.randrange(256) for _ in range(64)] for _ in range(4)]
    pats += [[rng.choice([0, 0, 0, 0xFF, 1 << rng.randrange(8)]) for _ in range(64)] for _ in range(3)]
    return pats


def run_ballots(p): return p.ballots(ballot_cases())


def define_ballots(_oracle=None):
    out = []
    for pat in ballot_cases():
        bit = [lanes_mask(l for l in range(64) if (pat[l] >> j) & 1) for j in range(8)]
        o = [bit[0], bit[0], bit[1], bit[0], bit[1], bit[2], bit[3]]
        for n in range(9):
            o += [bit[j] if j < n else POISON64 for j in range(8)] + [n]     # g(j, .) exactly for j < n, n calls
        out.append(o)
    return out


FIND_LO = [0, 1, 63, 64, 65, 511, 512, 513]
FIND_LEN = [0, 1, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1025]


@functools.lru_cache(None)
def find_cases():
    """(fn, lo, hi, h1, h2): fn 0 find_first, 1 find_last, 2 find_first8, 3 find_last8; the predicate holds at h1 and h2 (-1: nowhere)"""
    cases = []
    for lo in FIND_LO:
        for ln in FIND_LEN:
            hi = lo + ln
            hits = [(-1, -1)]
            if ln:
                hits += [(lo, -1), (hi - 1, -1)]
            if 1 < ln <= 129:
                hits += [(x, -1) for x in range(lo + 1, hi - 1)]              # every single position
            if ln >= 2:
                hits += [(lo + ln // 5, hi - 1 - ln // 7), (lo, hi - 1)]      # two hits: first and last differ
            if ln > 129:
                hits += [(x, -1) for x in {lo + 63, lo + 64, lo + 65, hi - 64, hi - 65, hi - 66, lo + ln // 2} if lo <= x < hi]
            cases += [(fn, lo, hi, h1, h2) for h1, h2 in hits for fn in range(4)]
    return cases


def run_find(p): return p.find(find_cases())


def define_find(_oracle=None):
    out = []
    for fn, lo, hi, h1, h2 in find_cases():
        pred = lambda i: i == h1 or i == h2
        if fn in (0, 2):
            out.append(next((i for i in range(lo, hi) if pred(i)), hi))
        else:
            out.append(next((i for i in range(hi - 1, lo - 1, -1) if pred(i)), lo - 1))
    return out


REDUCE_N = [0, 1, 63, 64, 65, 128, 1000]


@functools.lru_cache(None)
def reduce_cases():
    """-> (cases (fn, off, n), vals). fn 0 reduce_min, 1 reduce_max_i64, 2 reduce_or, 3 lanes_max_i64, 4 argmin_u32, 5 uniform, 6 fast_umin_s"""
    rng = random.Random(102)
    vals, cases = [], []

    def add(fn, xs, n=None):
        cases.append((fn, len(vals), len(xs) if n is None else n)); vals.extend(x & M64 for x in xs)

    specials = [0, 1 << 63, INT64_MIN, INT64_MAX, M64, 1, (1 << 32), (1 << 32) - 1]
    for n in REDUCE_N:
        fams = [[((i * 0x9E3779B1 + 12345) & M32) << 32 | 0x12345678 for i in range(n)],          # differ in the high word only
                [0xABCDEF01 << 32 | ((i * 0x85EBCA6B + 99) & M32) for i in range(n)],             # in the low word only
                [rng.getrandbits(64) for _ in range(n)],
                [rng.choice(specials) for _ in range(n)],
                [(1 << 63) | rng.getrandbits(62) for _ in range(n)],                               # all negative as int64
                [1 << (i % 64) for i in range(n)]]
        for xs in fams:
            for fn in (0, 1, 2):
                add(fn, xs)
    base = 5 << 32 | 7
    for i in range(64):                                                                              # the extreme on each lane in turn
        for fn, extremes in ((0, [0, 5 << 32 | 6, 4 << 32 | 7]), (1, [INT64_MAX, 5 << 32 | 8, 6 << 32 | 7]), (3, [INT64_MAX, 5 << 32 | 8, 6 << 32 | 7]), (2, [1 << i])):
            for e in extremes:
                xs = [base if fn != 2 else 0] * 64; xs[i] = e
                add(fn, xs)
        xs = [INT64_MIN] * 64; xs[i] = INT64_MIN + 1                                               # max over negatives, one step above the identity
        add(1, xs); add(3, xs)
        xs = [M64] * 64; xs[i] = M64 - 1
        add(0, xs)
    for xs in ([INT64_MIN] * 64, [0] * 64, [M64] * 64, [INT64_MAX] * 64, [rng.getrandbits(64) for _ in range(64)]):
        add(3, xs)
    hi_garbage = lambda l: ((l * 0x01010101 + 0xDEAD0000) & M32) << 32                               # argmin_u32 looks at the low word only
    for i in range(64):                                                                              # the minimum on each lane in turn
        add(4, [hi_garbage(l) | (5 if l == i else 1000 + l) for l in range(64)], 64)
        add(4, [hi_garbage(l) | (0x7FFFFFFF if l == i else 0x80000000) for l in range(64)], 64)   # unsigned order
        add(4, [hi_garbage(l) | (0 if l == i else 0xFFFFFFFF) for l in range(64)], 64)            # minimum 0
        add(4, [hi_garbage(l) | (0xFFFFFFFE if l == i else 0xFFFFFFFF) for l in range(64)], 64)
    for a, b in ((0, 63), (15, 16), (31, 32), (47, 48), (16, 47), (3, 4)):                           # ties: the lowest lane wins
        add(4, [7 if l in (a, b) else 9 + l for l in range(64)], 64)
        add(4, [0x80000000 if l in (a, b) else 0x80000001 + l for l in range(64)], 64)
    add(4, [7] * 64, 64); add(4, [M32] * 64, 64); add(4, [0] * 64, 64); add(4, [0x80000000] * 64, 64)
    for _ in range(6):
        add(4, [rng.choice([rng.getrandbits(32), 3, M32]) for _ in range(64)], 64)
    for x in (0, 1, 0x00000001FFFFFFFF, 0xFFFFFFFF00000000, 0x0123456789ABCDEF, 0x8000000000000001, M64):
        add(5, [x], 1)
    for a, b in ((0, 0), (0, M32), (M32, 0), (0x80000000, 0x7FFFFFFF), (0x7FFFFFFF, 0x80000000), (5, 5), (M32, M32), (0x80000000, 0x80000000), (1, 2)):
        add(6, [a, b], 2)
    return cases, vals


def run_reduce(p): return p.reduce(*reduce_cases())


def define_reduce(_oracle=None):
    cases, vals = reduce_cases()
    out = []
    for fn, off, n in cases:
        xs = vals[off:off + (n if fn <= 2 else 64 if fn <= 4 else 2)]
        if fn == 0: r = (min(xs, default=M64), 0, 0)
        elif fn == 1: r = (max((signed64(x) for x in xs), default=INT64_MIN) & M64, 0, 0)
        elif fn == 2: r = (functools.reduce(lambda a, b: a | b, xs, 0), 0, 0)
        elif fn == 3: r = (max(signed64(x) for x in xs) & M64, 0, 0)
        elif fn == 4:
            lo = [x & M32 for x in xs]
            m = min(lo)
            r = (m, (-1 if m == M32 else lo.index(m)) & M64, m)
        elif fn == 5: r = (xs[0], 0, 0)
        else: r = (min(xs[0] & M32, xs[1] & M32), 0, 0)
        out.append(r)
    return out


FOR_N = [0, 1, 63, 64, 65, 200]
def run_for_n(p): return p.for_n(FOR_N)
def define_for_n(_oracle=None): return [[1] * n + [0] * (264 - n) for n in FOR_N]


COPY_N = [0, 1, 511, 512, 513, 1500]
COPY_SRC = [(i * 40503 + 7) & 0xFFFF for i in range(1536)]
def run_copy8(p): return [p.copy8(COPY_SRC, n) for n in COPY_N]
def define_copy8(_oracle=None): return [(COPY_SRC[:n] + [0xEEEE] * (1536 - n),) * 2 for n in COPY_N]


def run_store_leader(p): return p.store_leader([0xAAAAAAAA, 0xBBBBBBBB, 0xCCCCDDDD, 41])


def define_store_leader(_oracle=None):
    lds = [0x11110000 + i for i in range(8)]; lds[2] = 0x9ABCDEF0
    return [0xAAAAAAAA, 0x12345678, 0xCCCCBEEF, 42], [0x12345678] * 64 + [0x9ABCDEF0] * 64 + [lds[l & 7] for l in range(64)]


@functools.lru_cache(None)
def lane_set_cases():
    rng = random.Random(103)
    vals = lambda: [rng.getrandbits(64) | (1 << 63 if i % 3 == 0 else 0) for i in range(64)]
    g = lambda: [0] * 64 + [rng.getrandbits(32) for _ in range(64)]
    return [([(i * 37 + 11) % 64 for i in range(64)], vals(), g()), (list(range(64)), vals(), g()), (list(range(63, -1, -1)), vals(), g()),
            ([rng.randrange(64) for _ in range(64)], vals(), g()), ([rng.choice([0, 63, 31, 32]) for _ in range(64)], vals(), g())]


def run_lane_set(p): return [p.lane_set(*c) for c in lane_set_cases()]


def define_lane_set(_oracle=None):
    out = []
    for idx, val, g in lane_set_cases():
        a, b, v, s, g = [0xA0000000 | l for l in range(64)], [0xB0000000 | l for l in range(64)], [0] * 64, [0] * 64, list(g)
        for i in range(64):
            ln, x = idx[i] & 63, val[i]
            a[ln] = x & M32
            s[i] = ((x >> 32) + s[(i + 63) & 63]) & M32
            b[63 - ln] = (x >> 32) ^ i
            v[ln] = x
            g[i] = ((x & M32) + g[64 + i]) & M32
        out.append((a, b, v, s, g))
    return out


BCAST_VAL = [((0xC0DE0000 + l * 0x10001) & M32) << 32 | ((0x1234567 * (l + 1)) & M32) for l in range(64)]
def run_bcast(p): return p.bcast(BCAST_VAL)
def define_bcast(_oracle=None): return [((x >> 32) ^ x) & M32 for x in BCAST_VAL], list(BCAST_VAL)


def shuffle_cases():
    pats = [list(range(64)), [(l + 63) & 63 for l in range(64)], [63 - l for l in range(64)], [0] * 64, [17] * 64, [63] * 64]
    pats += [[l if l < fl else (fl - 1 if fl > 0 else 0) for l in range(64)] for fl in (0, 1, 37, 64)]     # topo_engine.h's clamp: l < fl ? l : (fl > 0 ? fl - 1 : 0)
    pats += [[(l * 29 + 3) & 63 for l in range(64)], [l ^ 1 for l in range(64)], [l ^ 32 for l in range(64)]]
    return pats


def run_shuffle(p): return p.shuffle(shuffle_cases(), BCAST_VAL)


def define_shuffle(_oracle=None):
    a, b = define_bcast()
    return [([a[s & 63] for s in pat], [b[s & 63] for s in pat]) for pat in shuffle_cases()]


# ============================================================ Part B ============================================================
MEM_FORMS = (1, 2, 4, 5, 6)            # see the typedefs in the probe: 1 / 2 cursor plans 0-1 / 2, 4 general engine, 5 HBM fallback, 6 RunOrder
REG_FORMS = (3, 7)                     # RegOrder; 7 = RegOrder with pdqsort's frame stack in scratch
SMALL = [2, 12, 13, 24, 49, 50, 51, 63, 64]
BIG = [65, 511, 512, 513, 1023, 1024, 1025, 1100]


def go_sort(oracle, keys):
    return oracle.evaluate({"fn": "sort_by_key", "keys": list(keys)})


def sorted_patterns(rng, n):
    yield "all equal", [3] * n
    yield "two values", sorted(rng.choice([2, 5]) for _ in range(n))
    yield "two values, split", [2] * (n // 2) + [5] * (n - n // 2)
    yield "staircase", [1 + i // 4 for i in range(n)]
    yield "long runs", [1 + i // 300 for i in range(n)]
    yield "distinct", [1 + i for i in range(n)]


@functools.lru_cache(None)
def single_defect_cases():
    """(key, ord, defect, append, mode 0): sorted except the claim the last step touched"""
    rng = random.Random(104)
    cases = []
    for n in SMALL + BIG:
        q = n // 4
        if n <= 64:
            where = list(range(n))
        else:
            where = sorted({0, 1, n - 2, n - 1} | {c * q + d for c in (1, 2, 3) for d in (-2, -1, 0, 1, 2)} | {rng.randrange(n), 64, n - 65})
        for _, base in sorted_patterns(rng, n):
            ids = list(range(n)); rng.shuffle(ids)
            for p in where:
                key = list(base); key[p] += 1
                cases.append((key, ids, p, False, 0))
            cases.append((sorted(base[:n - 1]) + [1], ids, n - 1, True, 0))
            cases.append(([1] * (n - 1) + [1], ids, n - 1, True, 0))             # appended behind claims of one pod: nothing moves
    return cases


def cases_for_form(cases, form):
    if form in REG_FORMS:
        return [c for c in cases if len(c[0]) <= 64]
    if form == 6:
        return [c for c in cases if sum(c[0]) <= 20000 and c[4] == 0]
    return cases


def run_sorts(p, cases, form):
    cs = cases_for_form(cases, form)
    return p.sort(form, cs, n_pods=20008 if form == 6 else 0, max_claims=KCAP if form == 6 else 0)


def check_sorts(got, cases, form, oracle, cache):
    """every case's answer against the oracle's sort of the same keys: keys and claim ids in the oracle's permutation, `pos` its inverse"""
    cs = cases_for_form(cases, form)
    assert len(got) == len(cs)
    for (key, ids, defect, app, mode), (gk, go, gp, slow) in zip(cs, got):
        t = tuple(key)
        if t not in cache:
            cache[t] = go_sort(oracle, key)
        perm = cache[t]
        assert gk == [key[i] for i in perm] and go == [ids[i] for i in perm], (form, len(key), defect, app, mode, key[:16])
        if gp is not None:
            assert all(go[gp[c]] == c for c in range(len(key))), (form, len(key), defect, app)
        assert slow < 1 << 63, "RunOrder overflowed"


def increasing_samples(keys):
    """choosePivot's verdict 'increasing' (no swap among its samples) on the whole array: the outermost pdqsort call of pdq_emul.h then
    trusts its caller that at most the one known defect is out of place, so on an arbitrary array that call is outside its contract"""
    n = len(keys)
    if n < 8:
        return True
    i, j, k = n // 4, n // 4 * 2, n // 4 * 3
    s = [keys[x] for x in ((i - 1, i, i + 1, j - 1, j, j + 1, k - 1, k, k + 1) if n >= 50 else (i, j, k))]
    if n >= 50:
        # a swap-free median of three on each triple and on the medians = every triple ascending and the middles ascending
        return all(s[t] <= s[t + 1] <= s[t + 2] for t in (0, 3, 6)) and s[1] <= s[4] <= s[7]
    return s[0] <= s[1] <= s[2]


@functools.lru_cache(None)
def any_array_cases():
    """(key, ord, -1, False, mode 1): the outermost pdqsort call on arrays of the families of test_product_go_sort_matches_oracle_go_sort"""
    rng = random.Random(105)
    killers = []
    for n in (64, 1000):        # McIlroy's adversary played against go_sort.h (tests/tools/pdqsort_killer.cpp N 2): pdqsort uses up its bad partitions
        with open(os.path.join(HERE, "golden", f"pdqsort_killer_{n}.json")) as fh:
            killers.append(json.load(fh))
    cases, dropped = [], 0
    for n in SMALL + [65, 100, 257, 511, 512, 513, 1000, 1025, 2000]:
        fams = [[rng.randrange(0, max(1, n // 8)) for _ in range(n)], sorted(rng.randrange(0, 50) for _ in range(n)),
                sorted((rng.randrange(0, 50) for _ in range(n)), reverse=True), list(range(n, 0, -1)), [rng.randrange(0, 3) for _ in range(n)], [i % 7 for i in range(n)],
                list(range(n // 2)) + list(range(n - n // 2)), [min(i, n - i) for i in range(n)], [(i * 7919) % 13 for i in range(n)], [1] * (n - 1) + [0],
                [n - i if i % 2 else i for i in range(n)]]
        fams += [[rng.randrange(hi) for _ in range(n)] for hi in (2, 4, n, 1000, 60000) for _ in range(3)]
        for key in fams:
            if len(key) > 12 and increasing_samples(key) and key != sorted(key):
                dropped += 1
                continue
            ids = list(range(n)); rng.shuffle(ids)
            cases.append((key, ids, -1, False, 1))
    for killer in killers:                                                      # heap_sort, at 64 keys (RegOrder too) and at 1,000
        assert not increasing_samples(killer)
        cases.append((killer, list(range(len(killer))), -1, False, 1))
    assert dropped < len(cases) // 4
    return cases


def random_trace(rng, length, max_claims=None):
    ops, n = [], 0
    p_new = rng.choice([0.02, 0.2, 0.7])
    for _ in range(length):
        if n == 0 or (rng.random() < p_new and (max_claims is None or n < max_claims)):
            ops.append(-1); n += 1
        else:
            ops.append(rng.randrange(n) if rng.random() < 0.5 else max(0, n - 1 - int(rng.expovariate(0.2))))
    return ops


@functools.lru_cache(None)
def trace_cases():
    """name -> (ops, forms, (pods, max claims) of RunOrder's layout)"""
    rng = random.Random(11)
    out = {}
    for length in (15, 49, 51, 130, 700, 4000):
        for t in range(3):
            ops = random_trace(rng, length)
            out[f"random-{length}-{t}"] = (ops, MEM_FORMS, (len(ops) + 4, KCAP))
        for t in range(3 if length < 4000 else 1):
            out[f"random-{length}-64claims-{t}"] = (random_trace(rng, length, max_claims=rng.choice([13, 40, 64])), MEM_FORMS + (3,), (length + 4, 64))
    # one stable move across more than one 1,024-element round (form 2) and more than two 512-wide steps (form 1)
    out["past-1099-equal-keys"] = ([-1] * 1100 + [0, 0, 1, 2, 0], MEM_FORMS, (1200, 1100))            # rotate_left with same_keys
    out["new-claim-to-the-front"] = ([-1] * 1100 + list(range(1100)) + [-1, -1], MEM_FORMS, (2300, 1102))   # rotate_right to position 0
    # RunOrder alone: rings of 16 and 64 slots whose heads wrap in both directions (n <= 12 and n >= 50: the single-move path keeps the rings)
    # Rounds over all claims, up and down in turn: a claim enters the next run at its front (the head steps down, from 0 across the ring's end)
    # and, a round later, leaves it from the front (the head steps up again, across the end the other way).
    rounds = lambda m, r: [c if t % 2 == 0 else m - 1 - c for t in range(r) for c in range(m)]
    out["rings-wrap-12"] = ([-1] * 12 + rounds(12, 9) + [rng.randrange(12) for _ in range(150)], (6, 5), (300, 12))
    out["rings-wrap-60"] = ([-1] * 60 + rounds(60, 5) + [rng.randrange(60) for _ in range(300)], (6, 5), (700, 60))
    return out


def define_trace(oracle, ops):
    return oracle.evaluate({"fn": "order_trace", "ops": list(ops)})


def check_trace(got, ops, oracle):
    keys, ids, pos, slow, up, down = got
    assert ids == define_trace(oracle, ops)
    count = {}
    claims = 0
    for o in ops:
        if o < 0: count[claims] = 1; claims += 1
        else: count[o] += 1
    assert keys == [count[c] for c in ids] and keys == sorted(keys)
    if pos is not None:
        assert all(ids[pos[c]] == c for c in range(claims))
    assert slow < 1 << 63, "RunOrder overflowed"


SCAN_N = [65, 511, 512, 513, 1100]


@functools.lru_cache(None)
def scan_cases():
    """[(keys, n, [(op, lo, hi, v)])]: op 0 first_ge, 1 first_gt, 2 last_le, 3 last_lt, 4 first_descent"""
    rng = random.Random(107)
    out = []
    for n in SCAN_N:
        ranges = [(0, n), (1, n), (0, n - 1), (3, n - 3), (5, 5), (n, n), (0, 0), (n // 2, n // 2 + 1)]
        for lo in (0, 1, 7, 8, 9, 504, 511, 512, 513, 520, 1023, 1024, 1025):       # around multiples of 8 and of 512, lo == hi among them
            ranges += [(lo, hi) for hi in (lo, lo + 1, lo + 7, lo + 8, 16, 511, 512, 513, 520, 1024, 1025, n - 1, n) if lo <= hi <= n]
        ranges += [tuple(sorted((rng.randrange(n + 1), rng.randrange(n + 1)))) for _ in range(8)]
        ranges = sorted(set(ranges))

        def table(vs, ops=(0, 1, 2, 3, 4)):
            return [(op, max(lo, 1) if op == 4 else lo, hi, v) for op in ops for v in (vs if op != 4 else [0]) for lo, hi in ranges if op != 4 or max(lo, 1) <= hi]

        out.append(([10] * n, n, table([0, 10, 11, 20])))
        marks = sorted({0, 1, 7, 8, 63, 64, 511, 512, 513, 520, 1023, 1024, n - 1} & set(range(n)))
        for m in marks:                                # exactly one answer, at m; then a step at m
            k = [10] * n; k[m] = 20
            out.append((k, n, table([15, 20], ops=(0, 1))))
            k = [10] * n; k[m] = 5
            out.append((k, n, table([5, 7], ops=(2, 3, 4))))
            out.append(([10 if j < m else 20 for j in range(n)], n, table([10, 20], ops=(0, 1, 2, 3))))
        for top in (2, 3, 50, 60000):
            k = [rng.randrange(top) for _ in range(n)]
            out.append((k, n, table([0, rng.randrange(top + 1), top])))
    return out


def run_scans(p): return [p.scans(keys, n, cases) for keys, n, cases in scan_cases()]


def define_scans(_oracle=None):
    out = []
    for keys, n, cases in scan_cases():
        k = np.asarray(keys, dtype=np.int64)
        masks = {}
        ans = []
        for op, lo, hi, v in cases:
            if (op, v) not in masks:
                if op == 4:
                    m = np.zeros(n, dtype=bool); m[1:] = k[1:] < k[:-1]
                else:
                    m = (k >= v, k > v, k <= v, k < v)[op]
                masks[op, v] = m
            hit = np.flatnonzero(masks[op, v][lo:hi])
            r = (lo + int(hit[-1]) if len(hit) else lo - 1) if op in (2, 3) else (lo + int(hit[0]) if len(hit) else hi)
            ans.append([r, r])        # form 1's 512-wide answer and form 2's one-position-per-lane answer
        out.append(ans)
    return out


SHIFT_ARR = [(i * 40503 + 7) & 0xFFFF for i in range(1536)]      # distinct (an odd multiplier is a bijection of 16-bit values)
SHIFT_MARKS = [0, 1, 7, 8, 9, 15, 16, 510, 511, 512, 513, 519, 520, 1023, 1024, 1025]
SHIFT_CASES = [(b, a) for b in SHIFT_MARKS for a in SHIFT_MARKS if b <= a]
def run_shift(p): return p.shift(SHIFT_ARR, SHIFT_CASES)
def define_shift(_oracle=None): return [SHIFT_ARR[:b + 1] + SHIFT_ARR[b:a] + SHIFT_ARR[a + 1:] for b, a in SHIFT_CASES]


# the groups whose answer is one comparable value: name -> (run, define)
PART_A = {"ballots": (run_ballots, define_ballots), "find": (run_find, define_find), "reduce": (run_reduce, define_reduce), "for_n": (run_for_n, define_for_n),
          "copy8": (run_copy8, define_copy8), "store_leader": (run_store_leader, define_store_leader), "lane_set": (run_lane_set, define_lane_set),
          "bcast": (run_bcast, define_bcast), "shuffle": (run_shuffle, define_shuffle)}
PART_B_PLAIN = {"scans": (run_scans, define_scans), "shift_right16": (run_shift, define_shift)}
