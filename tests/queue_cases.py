"""The queue order (be_sort_pods in csrc/ksolve.hip: ksolve_iota, five passes of ksolve_sort_key and rocprim::radix_sort_pairs) and
the queue marking (be_launch_fast_queue: ksolve_fast_queue, ksolve_fast_overlap, ksolve_fast_mark) against their definitions, stated
here once on plain Python ints and lists — nothing shared with the product, the emulation or tests/invariants.py.

THE QUEUE ORDER (queue.go:72-108): sorted(range(n_pods), key=(-cpu, -memory, creation, uid_hi, uid_lo)), the uid words unsigned;
Python's sort is stable, so fully equal pods stay in index order.

THE SIZES. 1, 2, 255, 256, 257 and 4,099, and one above each of the two sizes below 300,001 at which the installed rocprim's
radix_sort_pairs changes its algorithm for the keys and values of be_sort_pods (64-bit keys, 32-bit values, default_config), read
from the headers under the ROCm include directory. There are three such sizes in all:
  * 1,024 — rocprim/device/device_radix_sort.hpp, radix_sort_impl: `size <= single_sort_items_per_block` sorts in ONE block
    (radix_sort_block_sort). single_sort_items_per_block = block_size * items_per_thread of kernel_config<min(256, B), min(4, I)>,
    B and I from radix_sort_block_sort_config_base<Key, Value> in rocprim/device/detail/device_config_helper.hpp: item_scale =
    max(sizeof(Key), sizeof(Value)) = 8 -> B = merge_sort_block_size(8) * 2 = 256, I = min(4, merge_sort_items_per_thread(8)) = 4.
    SINGLE_BLOCK_LIMIT + 1 = 1,025 is the first size sorted by several blocks: block sort, then merge passes (radix_sort_merge_impl in
    rocprim/device/specialization/device_radix_merge_sort.hpp, which calls merge_sort_block_merge with the default config).
  * 201,072 — rocprim/device/device_merge_sort.hpp, merge_sort_block_merge: `use_mergepath = size > merge_oddeven_config.size_limit`.
    Up to the limit the merge passes are the odd-even block merge, above it the merge-path partition and merge kernels. size_limit is
    (1 << 17) + 70000 in merge_sort_block_merge_config_base (rocprim/device/detail/device_config_helper.hpp) and in every tuned entry
    of rocprim/device/detail/config/device_merge_sort_block_merge.hpp. ODDEVEN_MERGE_LIMIT + 1 = 201,073 is the first size on the
    merge-path kernels — the path of every solve from 201,073 to 1,048,576 pods, the headline problem (a million pods) among them.
  * 1,048,576 — radix_sort_impl again: `size <= merge_sort_limit` (radix_sort_config<>::merge_sort_limit, the default of
    MergeSortLimit in rocprim/device/device_radix_sort_config.hpp: 1024 * 1024) is the merge sort above, anything larger Onesweep.
    No case here is that large: the largest sort input of this suite is held under 300,001 keys, where the Python side of the
    comparison still takes well under a second. Onesweep is reached by the two-million-pod problems only, whose results are pinned
    end to end (tests/test_gpu_parity.py).
Every family below runs at every size but the largest, which gets (a) and (b) only.

THE INPUT FAMILIES, one launch per (family, size): (a) random with ties everywhere — cpu and memory from 5 values each, among them 0
and values above 2^40, creation from 4 values, among them a negative one and one above 2^32, random 64-bit uids; (b) cpu, memory and
creation equal, uid_hi of 3 values, uid_lo random: the last two passes carry the order through three passes that must be stable;
(c) fully equal pods: the identity; (d) already sorted and reverse sorted; (e) PAIRS: each criterion alone deciding between two pods
equal in the other four (sign and direction: cpu 2^62 against 2^62 - 1, creation -1 against 0, uid words 2^63 against 2^63 - 1);
(f) n_rows = n_pods + 37, the rows past the pods holding requests that would sort first if they were read.

THE QUEUE MARKING: q_class[i] = row_class[sorted[i]], or-ed with kFastLastBit on the last entry of its class; q_claim[i] =
0xFFFFFFFF; cls_first / cls_last = the first and last entry of every class, 0xFFFFFFFF / 0 for a class without entries; max_active =
the most, over the classes present, of the classes o with first[o] <= first[c] <= last[o] — and 0 where the launcher skips the count:
n_classes <= 64, n_classes > 32768, or count_live = 0.

run_sort() and run_marking() drive the test-only entry points ksolve_test_sort_pods and ksolve_test_fast_queue of a test build of the
solver library (tests/emu/libksolve_emu.so on the host, tests/emu/libksolve_hooks.so on the GPU). Every comparison is exact and no
output field is left out."""
import bisect
import ctypes
import functools
import os

import numpy as np

U64, I64, U32 = np.uint64, np.int64, np.uint32
SINGLE_BLOCK_LIMIT = 1024            # see the docstring: where these were read
ODDEVEN_MERGE_LIMIT = (1 << 17) + 70000
MERGE_SORT_LIMIT = 1024 * 1024       # (no case beyond it)
SORT_SIZES = (1, 2, 255, 256, 257, SINGLE_BLOCK_LIMIT + 1, 4099, ODDEVEN_MERGE_LIMIT + 1)
SORT_FAMILIES = ("a", "b", "c", "d-sorted", "d-reversed", "f")
SORT_CASES = [(f, n) for n in SORT_SIZES for f in SORT_FAMILIES if n <= 4099 or f in ("a", "b")]
K_FAST_LAST_BIT = 0x80000000
NOT_PLACED = 0xFFFFFFFF

CPUS = [0, 100, 250, (1 << 40) + 7, (1 << 40) + 8]
MEMORIES = [0, 1 << 20, (1 << 41) + 5, (1 << 41) + (1 << 33) + 5, 1 << 62]
CREATIONS = [-5, 0, 1_700_000_000, (1 << 32) + 9]
UID_HIS = [3, (1 << 63) + 1, (1 << 64) - 1]


# ------------------------------------------------------------------------------------------------ the queue order
def expected_order(cpu, memory, creation, uid_hi, uid_lo):
    """THE DEFINITION, on lists of Python ints."""
    keys = list(zip([-c for c in cpu], [-m for m in memory], creation, uid_hi, uid_lo))
    return sorted(range(len(keys)), key=keys.__getitem__)


def _finish(case):
    n = case["n"]
    req = case["requests"]
    case["expected"] = np.array(expected_order(req[0, :n].tolist(), req[1, :n].tolist(), case["creation"].tolist(), case["uid_hi"].tolist(), case["uid_lo"].tolist()), U32)
    for a in case.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return case


def _case(cpu, memory, creation, uid_hi, uid_lo, extra_rows=0):
    n = len(cpu)
    req = np.zeros((2, n + extra_rows), I64)
    req[0, :n], req[1, :n] = cpu, memory
    if extra_rows:
        req[0, n:], req[1, n:] = (1 << 62) + 1, (1 << 62) + 1        # more cpu and memory than any pod: first in the queue if read
    return dict(n=n, n_rows=n + extra_rows, requests=req, creation=np.asarray(creation, I64), uid_hi=np.asarray(uid_hi, U64), uid_lo=np.asarray(uid_lo, U64))


@functools.lru_cache(maxsize=None)
def sort_case(family, n):
    """The inputs of a (family, size) with their expected order: built once, shared by every test, read-only."""
    rng = np.random.default_rng([ord(family[0]), len(family), n])
    words = lambda: rng.integers(0, 1 << 64, n, dtype=U64)
    pick = lambda vals, dt: np.array(vals, dt)[rng.integers(0, len(vals), n)]
    if family in ("a", "d-sorted", "d-reversed", "f"):
        c = _case(pick(CPUS, I64), pick(MEMORIES, I64), pick(CREATIONS, I64), words(), words(), extra_rows=37 if family == "f" else 0)
        if family.startswith("d"):
            order = expected_order(c["requests"][0].tolist(), c["requests"][1].tolist(), c["creation"].tolist(), c["uid_hi"].tolist(), c["uid_lo"].tolist())
            if family == "d-reversed":
                order = order[::-1]
            c = _case(c["requests"][0][order], c["requests"][1][order], c["creation"][order], c["uid_hi"][order], c["uid_lo"][order])
        return _finish(c)
    if family == "b":
        return _finish(_case(np.full(n, CPUS[3], I64), np.full(n, MEMORIES[2], I64), np.full(n, CREATIONS[0], I64), pick(UID_HIS, U64), words()))
    if family == "c":
        return _finish(_case(np.full(n, CPUS[1], I64), np.full(n, MEMORIES[4], I64), np.full(n, CREATIONS[3], I64), np.full(n, UID_HIS[1], U64), np.full(n, (1 << 63) + 77, U64)))
    raise KeyError(family)


# (criterion, the value of the pod that comes first, the value of the pod that comes second); the other four criteria are equal
PAIRS = [("cpu", 1 << 62, (1 << 62) - 1), ("cpu", 1, 0), ("cpu", (1 << 40), (1 << 40) - 1), ("cpu", 1 << 32, 0xFFFFFFFF),
         ("memory", 1 << 62, (1 << 62) - 1), ("memory", 1, 0), ("memory", 1 << 32, 0xFFFFFFFF),
         ("creation", -1, 0), ("creation", -(1 << 62), 1 << 62), ("creation", 0xFFFFFFFF, 1 << 32), ("creation", -2, -1),
         ("uid_hi", (1 << 63) - 1, 1 << 63), ("uid_hi", 0, (1 << 64) - 1), ("uid_hi", 0xFFFFFFFF, 1 << 32),
         ("uid_lo", (1 << 63) - 1, 1 << 63), ("uid_lo", 0, (1 << 64) - 1), ("uid_lo", 0xFFFFFFFF, 1 << 32)]
PAIR_BASE = dict(cpu=500, memory=1 << 30, creation=1_700_000_000, uid_hi=(1 << 63) + 12345, uid_lo=(1 << 63) + 54321)


@functools.lru_cache(maxsize=None)
def pair_case(i, swapped):
    """Pair i of PAIRS; swapped: the pod that comes first in the queue is pod 1."""
    crit, first, second = PAIRS[i]
    cols = {k: [v, v] for k, v in PAIR_BASE.items()}
    cols[crit] = [second, first] if swapped else [first, second]
    c = _finish(_case(cols["cpu"], cols["memory"], cols["creation"], cols["uid_hi"], cols["uid_lo"]))
    assert c["expected"].tolist() == ([1, 0] if swapped else [0, 1])
    return c


class _SortIn(ctypes.Structure):
    _fields_ = [("n_pods", ctypes.c_uint32), ("n_rows", ctypes.c_uint32)] + [(f, ctypes.c_void_p) for f in ("requests", "creation", "uid_hi", "uid_lo")]


class _SortOut(ctypes.Structure):
    _fields_ = [("sorted", ctypes.c_void_p)]


class _QueueIn(ctypes.Structure):
    _fields_ = [("n_pods", ctypes.c_uint32), ("n_rows", ctypes.c_uint32), ("n_classes", ctypes.c_uint32), ("sorted", ctypes.c_void_p), ("row_class", ctypes.c_void_p),
                ("count_live", ctypes.c_uint32)]


class _QueueOut(ctypes.Structure):
    _fields_ = [(f, ctypes.c_void_p) for f in ("q_class", "q_claim", "cls_first", "cls_last")] + [("max_active", ctypes.c_uint32)]


_libs = {}


def _lib(path):
    if path not in _libs:
        lib = ctypes.CDLL(os.path.abspath(path))
        lib.ksolve_test_sort_pods.restype = ctypes.c_int
        lib.ksolve_test_sort_pods.argtypes = [ctypes.POINTER(_SortIn), ctypes.POINTER(_SortOut)]
        lib.ksolve_test_fast_queue.restype = ctypes.c_int
        lib.ksolve_test_fast_queue.argtypes = [ctypes.POINTER(_QueueIn), ctypes.POINTER(_QueueOut)]
        _libs[path] = lib
    return _libs[path]


def run_sort(lib_path, case):
    """ksolve_test_sort_pods on a case: one call of be_sort_pods. The output starts as a pattern no answer has."""
    n = case["n"]
    tabs = [np.ascontiguousarray(case[f]) for f in ("requests", "creation", "uid_hi", "uid_lo")]
    assert tabs[0].shape == (2, case["n_rows"]) and all(t.shape == (n,) for t in tabs[1:])
    out = np.full(n, 0xEEEEEEEE, U32)
    arg, o = _SortIn(n, case["n_rows"], *[t.ctypes.data for t in tabs]), _SortOut(out.ctypes.data)
    st = _lib(lib_path).ksolve_test_sort_pods(ctypes.byref(arg), ctypes.byref(o))
    assert st == 0, f"ksolve_test_sort_pods: status {st}"
    return out


def check_sort(case, got, what=""):
    want = case["expected"]
    if not np.array_equal(got, want):
        bad = np.nonzero(got != want)[0]
        i = int(bad[0])
        row = lambda p: None if p >= case["n"] else (int(case["requests"][0, p]), int(case["requests"][1, p]), int(case["creation"][p]), int(case["uid_hi"][p]), int(case["uid_lo"][p]))
        raise AssertionError(f"{what}: {len(bad)} of {case['n']} queue entries differ from the definition, the first at entry {i}: pod {int(got[i])} {row(int(got[i]))} "
                             f"where pod {int(want[i])} {row(int(want[i]))} belongs")


# ------------------------------------------------------------------------------------------------ the queue marking
def count_skipped(n_classes, count_live):
    """the launcher's gate: no count of the classes live at once (max_active stays 0)"""
    return n_classes <= 64 or n_classes > 32768 or not count_live


def live_at_first(first, last):
    """THE DEFINITION of max_active, class by class: for every class present, the classes o with first[o] <= first[c] <= last[o]."""
    present = [c for c in range(len(first)) if first[c] != NOT_PLACED]
    return {c: sum(1 for o in present if first[o] <= first[c] <= last[o]) for c in present}


def expected_marking(sorted_, row_class, n_classes, count_live):
    """THE DEFINITION, on lists of Python ints. (max_active by counting: the classes that began at or before first[c], less those that
    ended before it — the same number as live_at_first(), which tests/test_queue_kernels.py holds it against.)"""
    n = len(sorted_)
    q = [row_class[p] for p in sorted_]
    first, last = [NOT_PLACED] * n_classes, [0] * n_classes
    for i, c in enumerate(q):
        first[c] = min(first[c], i)
        last[c] = max(last[c], i)
    present = [c for c in range(n_classes) if first[c] != NOT_PLACED]
    q_class = [c | (K_FAST_LAST_BIT if last[c] == i else 0) for i, c in enumerate(q)]
    max_active = 0
    if not count_skipped(n_classes, count_live):
        firsts, lasts = sorted(first[c] for c in present), sorted(last[c] for c in present)
        max_active = max(bisect.bisect_right(firsts, first[c]) - bisect.bisect_left(lasts, first[c]) for c in present)
    return dict(q_class=np.array(q_class, U32), q_claim=np.full(n, NOT_PLACED, U32), cls_first=np.array(first, U32), cls_last=np.array(last, U32), max_active=max_active)


def _mark(sorted_, row_class, n_classes, count_live=1):
    c = dict(sorted=np.asarray(sorted_, U32), row_class=np.asarray(row_class, U32), n_classes=n_classes, count_live=count_live)
    c["expected"] = expected_marking(c["sorted"].tolist(), c["row_class"].tolist(), n_classes, count_live)
    for a in list(c.values()) + list(c["expected"].values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def _queue_of(classes, rng, spare_rows=0):
    """a queue whose entry i has class classes[i]: the pods are a random permutation (of more rows than pods with spare_rows)"""
    n = len(classes)
    pods = rng.permutation(n + spare_rows)
    row_class = np.zeros(n + spare_rows, U32)
    row_class[pods[:n]] = classes
    row_class[pods[n:]] = classes[0] if n else 0         # rows outside the queue: a class that exists, and never an entry
    return pods[:n], row_class


def _nested(nc):
    return [c if c < nc else 2 * nc - 1 - c for c in range(2 * nc)]


MARKING_CASES = ["one-class-70001", "own-class-4099", "disjoint-runs-65", "nested-64", "nested-65", "nested-66", "nested-257", "boundary-64-of-65", "boundary-65-of-65",
                 "random-4099", "random-255", "random-256", "random-257", "nested-257-uncounted", "classes-32769"]
# what the definition must report for max_active (None: whatever it reports, which test_queue_kernels.py bounds)
MARKING_MAX_ACTIVE = {"one-class-70001": 0, "own-class-4099": 1, "disjoint-runs-65": 1, "nested-64": 0, "nested-65": 65, "nested-66": 66, "nested-257": 257, "boundary-64-of-65": 64,
                      "boundary-65-of-65": 65, "random-4099": None, "random-255": None, "random-256": None, "random-257": None, "nested-257-uncounted": 0, "classes-32769": 0}


@functools.lru_cache(maxsize=None)
def marking_case(name):
    rng = np.random.default_rng([len(name)] + [ord(ch) for ch in name])
    if name == "one-class-70001":           # every thread contends on the same two words
        return _mark(*_queue_of(np.zeros(70001, U32), rng), 1)
    if name == "own-class-4099":
        return _mark(*_queue_of(rng.permutation(4099), rng), 4099)
    if name == "disjoint-runs-65":          # class ids in a shuffled order, runs of 1 to 9 entries
        ids = rng.permutation(65)
        return _mark(*_queue_of(np.concatenate([np.full(int(rng.integers(1, 10)), c, U32) for c in ids]), rng), 65)
    if name.startswith("nested-"):          # class c at entries c and 2 nc - 1 - c: all nc classes live at entry nc - 1
        nc = int(name.split("-")[1])
        return _mark(*_queue_of(np.array(_nested(nc), U32), rng), nc, 0 if name.endswith("uncounted") else 1)
    if name == "boundary-64-of-65":         # 64 classes nested, the 65th behind them: 64 live at once, one row of class slots
        return _mark(*_queue_of(np.array(_nested(64) + [64, 64], U32), rng), 65)
    if name == "boundary-65-of-65":         # the 65th opens inside the innermost one: 65 live at once, four rows
        return _mark(*_queue_of(np.array(_nested(64)[:64] + [64] + _nested(64)[64:] + [64], U32), rng), 65)
    if name.startswith("random-"):          # 300 classes, 5 more ids that never occur, more rows than queue entries
        n = int(name.split("-")[1])
        ids = rng.permutation(305)[:300]
        return _mark(*_queue_of(ids[rng.integers(0, 300, n)].astype(U32), rng, spare_rows=11), 305)
    if name == "classes-32769":             # beyond the count's reach: skipped, whatever the queue holds
        return _mark(*_queue_of(np.array(_nested(70), U32) * 468 + 9, rng), 32769)
    raise KeyError(name)


MARKING_FIELDS = ("q_class", "q_claim", "cls_first", "cls_last", "max_active")


def run_marking(lib_path, case):
    """ksolve_test_fast_queue on a case: the three fills and one be_launch_fast_queue. The outputs start as a pattern no answer has."""
    srt, rc = np.ascontiguousarray(case["sorted"]), np.ascontiguousarray(case["row_class"])
    n, nc = len(srt), case["n_classes"]
    out = dict(q_class=np.full(n, 0xEEEEEEEE, U32), q_claim=np.full(n, 0xEEEEEEEE, U32), cls_first=np.full(nc, 0xEEEEEEEE, U32), cls_last=np.full(nc, 0xEEEEEEEE, U32))
    arg = _QueueIn(n, len(rc), nc, srt.ctypes.data, rc.ctypes.data, case["count_live"])
    o = _QueueOut(*[out[f].ctypes.data for f in MARKING_FIELDS[:4]], 0xEEEEEEEE)
    st = _lib(lib_path).ksolve_test_fast_queue(ctypes.byref(arg), ctypes.byref(o))
    assert st == 0, f"ksolve_test_fast_queue: status {st}"
    out["max_active"] = int(o.max_active)
    return out


def marking_mismatches(got, want, limit=6):
    bad = []
    for f in MARKING_FIELDS[:4]:
        for i in np.nonzero(got[f] != want[f])[0][:limit]:
            bad.append((f, int(i), hex(int(got[f][i])), hex(int(want[f][i]))))
    if got["max_active"] != want["max_active"]:
        bad.append(("max_active", got["max_active"], want["max_active"]))
    return bad
