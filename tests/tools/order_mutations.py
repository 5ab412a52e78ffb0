#!/usr/bin/env python3
"""Do the cases of tests/wave_order_cases.py notice a wrong wavefront primitive, sort, order accessor or ring? (CPU only; a tool, not a
pytest test.)

Copies include/, karpenter_amd/, oracle/ and tests/ to a temporary directory once per mutation, applies ONE single-line textual
mutation to the copy's HOST path of wave.h, pdq_emul.h or run_order.h (the loop-over-lanes Wave, or code both builds share), and runs
tests/test_wave_order.py there, which builds the host twins of tests/emu/wave_order_probe.cpp from the mutated copy. One block per
mutation: the tests that fail. A mutation whose search text does not occur exactly once is an error of this tool (the source moved
on: mend the list), never a pass; a mutation nothing catches makes the exit status 1, unless the list marks it EQUIVALENT and says
why. Nothing mutated is ever built for or run on a GPU: this shows that the cases discriminate, the device run of the same cases
(tests/test_gpu_wave_order.py) that the device form is right.

    python tests/tools/order_mutations.py [-j N] [--out profiles/wave_order_tests/mutations.txt]
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (name, file under karpenter_amd/csrc, search text, replacement[, why no input can tell the two apart])
MUTATIONS = [
    ("find_last: stops one short of lo", "wave.h", "for (int i = hi - 1; i >= lo; --i) if (pred(i)) return i; return lo - 1;", "for (int i = hi - 1; i > lo; --i) if (pred(i)) return i; return lo - 1;"),
    ("find_first: stops one short of hi", "wave.h", "for (int i = lo; i < hi; ++i) if (pred(i)) return i; return hi;", "for (int i = lo; i < hi - 1; ++i) if (pred(i)) return i; return hi;"),
    ("argmin_u32: a tie goes to the higher lane", "wave.h", "(x == m && who >= 0 && l < who)", "(x == m && who >= 0 && l > who)"),
    ("ballot4: the fourth word tests bit 2", "wave.h", "if (v & 8) m3 |= 1ull << l; }", "if (v & 4) m3 |= 1ull << l; }"),
    ("ballots8: one predicate short", "wave.h", "for (int j = 0; j < n; ++j) { uint64_t m = 0;", "for (int j = 0; j < n - 1; ++j) { uint64_t m = 0;"),
    ("for_n: the last index left out", "wave.h", "KS_LANES(l) if (base + l < n) f(base + l);", "KS_LANES(l) if (base + l < n - 1) f(base + l);"),
    ("reduce_max_i64: identity 0", "wave.h", "{ int64_t v = INT64_MIN; for_n(n,", "{ int64_t v = 0; for_n(n,"),
    ("lanes_max_i64: identity 0", "wave.h", "{ int64_t v = INT64_MIN; KS_LANES(l)", "{ int64_t v = 0; KS_LANES(l)"),
    ("reduce_min: a 32-bit accumulator", "wave.h", "{ uint64_t v = ~0ull; for_n(n, [&](int i) { uint64_t x = f(i); if (x < v) v = x; }); return v; }",
     "{ uint64_t v = ~0ull; for_n(n, [&](int i) { uint64_t x = f(i); if ((uint32_t)x < (uint32_t)v) v = x; }); return v; }"),
    ("copy8: one element short", "wave.h", "for (int i = 0; i < n; ++i) dst[i] = src[i]; }", "for (int i = 0; i < n - 1; ++i) dst[i] = src[i]; }"),
    ("LaneVar::shuffle: the lane above the source", "wave.h", "T shuffle(int, int src) const { return v[src & 63]; }", "T shuffle(int, int src) const { return v[(src + 1) & 63]; }"),
    ("LaneVar::bcast: lane 0 always", "wave.h", "  T bcast(int lane) const { return v[lane]; }", "  T bcast(int lane) const { return v[lane & 0]; }"),
    ("pdqsort: length <= 12 -> < 12", "pdq_emul.h", "if (length <= 12) { insertion_sort(s, a, b); done = true; break; }", "if (length < 12) { insertion_sort(s, a, b); done = true; break; }"),
    ("choose_pivot: l >= 50 -> l > 50", "pdq_emul.h", "      if (l >= 50) {\n        uint32_t s0", "      if (l > 50) {\n        uint32_t s0"),
    ("break_patterns: xorshift 13 -> 12", "pdq_emul.h", "r ^= r << 13;", "r ^= r << 12;"),
    ("choose_pivot: swaps == 12 -> 11", "pdq_emul.h", "(swaps == 12 ? 2 : 0)", "(swaps == 11 ? 2 : 0)"),
    ("pdqsort: limit == 0 never true", "pdq_emul.h", "if (cur.limit == 0) { heap_sort(s, a, b); done = true; break; }", "if (false) { heap_sort(s, a, b); done = true; break; }"),
    ("rotate_left loses same_keys: the passed count is not written back", "pdq_emul.h", "if (same_keys) W::store(&key[from], passed);", "if (false) W::store(&key[from], passed);"),
    ("sort: the appended claim goes in front of its equals", "pdq_emul.h", "const int t = s.last_le_sorted(0, i, mv);   // [0, i) is sorted", "const int t = s.last_le_sorted(0, i, mv - 1);   // [0, i) is sorted"),
    ("upper_last_sorted: < for <=", "pdq_emul.h", "if (!(v < key[mid])) a = mid + 1; else b = mid; }", "if (key[mid] < v) a = mid + 1; else b = mid; }"),
    ("wide_scan: the range's upper end masked one key late", "pdq_emul.h", "(b >= 8 ? 0xFFu : b <= 0 ? 0u : (1u << b) - 1u)", "(b >= 8 ? 0xFFu : b <= 0 ? 0u : (2u << b) - 1u)"),
    ("wide_scan: lane 0 takes no key from under the step", "pdq_emul.h", "dn.at(l) = l ? up.at(l) >> 16 : under;", "dn.at(l) = l ? up.at(l) >> 16 : 0u;"),
    ("ClaimOrder::swap: pos of the second claim not updated", "pdq_emul.h", "W::store(&pos[oi], (uint32_t)j); }", "W::store(&pos[oi], (uint32_t)i); }"),
    ("RegOrder::rotate_right: the moved claim's old place keeps its claim", "pdq_emul.h", "(l > to && l <= from) ? l - 1 : l; });", "(l > to && l < from) ? l - 1 : l; });"),
    ("RegOrder::last: the lowest lane for the highest", "pdq_emul.h", "return m ? 63 - __builtin_clzll(m) : lo - 1;\n  }\n  KS_FN int first_ge", "return m ? ctz64(m) : lo - 1;\n  }\n  KS_FN int first_ge"),
    ("shift_right16: entry b itself is overwritten", "pdq_emul.h", "((elo > b && elo <= a) ? 0xFFFFu : 0u)", "((elo >= b && elo <= a) ? 0xFFFFu : 0u)"),
    ("shift_ring: the ring mask dropped from a read", "run_order.h", "else for (int i = 0; i < cntr; ++i) { const uint32_t x = r[(h + base + (uint32_t)i) & m];", "else for (int i = 0; i < cntr; ++i) { const uint32_t x = r[(h + base + (uint32_t)i)];"),
    ("RunOrder::claim_at: the ring mask dropped", "run_order.h", "return ring[off_(lo) + ((head_(lo) + ((uint32_t)p - prefix_(lo))) & mask_of(lo))];", "return ring[off_(lo) + ((head_(lo) + ((uint32_t)p - prefix_(lo))))];"),
    ("RunOrder::position: the run's prefix left out", "run_order.h", "return prefix_(k) + ((slot[c] - head_(k)) & mask_of(k));", "return ((slot[c] - head_(k)) & mask_of(k));"),
    ("RunOrder::sort: position q - 1 taken for unsampled", "run_order.h", "const bool sampled = (p >= q - 1 && p <= q + 1) || (p >= 2 * q - 1 && p <= 2 * q + 1) || (p >= 3 * q - 1 && p <= 3 * q + 1);\n      fast = !sampled;",
     "const bool sampled = (p >= q && p <= q + 1) || (p >= 2 * q - 1 && p <= 2 * q + 1) || (p >= 3 * q - 1 && p <= 3 * q + 1);\n      fast = !sampled;"),
    ("move_known: the shorter side is always the front", "run_order.h", "if (i <= sz - 1 - i) { shift_ring(k, 0, i, +1); new_head = (h + 1) & m; }", "if (true) { shift_ring(k, 0, i, +1); new_head = (h + 1) & m; }",
     "EQUIVALENT: either side may step over the hole; which one does is a matter of speed only"),
    ("move_appended: the prefixes behind run 1 stay", "run_order.h", "if (k < kRunMaxCount) tt->e[k].prefix += 1; else gp[k] += 1; });", "if (k < kRunMaxCount) tt->e[k].prefix += 0; else gp[k] += 1; });"),
]


def run_mutation(i, work):
    name, fname, old, new = MUTATIONS[i][:4]
    d = os.path.join(work, f"m{i + 1:02d}")
    for sub in ("include", "karpenter_amd", "oracle", "tests"):
        shutil.copytree(os.path.join(ROOT, sub), os.path.join(d, sub), ignore=shutil.ignore_patterns("_obj", "_ref", "libksolve*.so", "libksched.so", "libwave_order*.so", "__pycache__", "*.lock", "*.tmp"))
    shutil.copy(os.path.join(ROOT, "__graft_entry__.py"), d)
    path = os.path.join(d, "karpenter_amd", "csrc", fname)
    with open(path) as f:
        text = f.read()
    if text.count(old) != 1:
        raise SystemExit(f"mutation {i + 1} ({name}): its search text occurs {text.count(old)} times in {fname}")
    with open(path, "w") as f:
        f.write(text.replace(old, new))
    # three runs, so that a mutation under which one group of tests dies (a sort that runs off its array in the host twin) still shows
    # which tests of the other groups fail; a run that dies counts as caught and is reported as such
    failed, tail = [], ""
    for group in ("against_definition", "sort or stacks or path", "commit_trace"):
        r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_wave_order.py", "-k", group, "-q", "-p", "no:cacheprovider", "--tb=no", "-rf"], cwd=d, capture_output=True, text=True, timeout=900)
        failed += re.findall(r"^(?:FAILED|ERROR) (\S+)", r.stdout, re.M)
        if r.returncode not in (0, 1):
            failed.append(f"(the run of -k '{group}' died with status {r.returncode})")
        tail += r.stdout[-200:]
    return name, failed, tail


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-j", type=int, default=4)
    ap.add_argument("--out")
    args = ap.parse_args()
    lines, missed = [], 0
    with tempfile.TemporaryDirectory() as work, ThreadPoolExecutor(max_workers=args.j) as pool:
        for i, (name, failed, tail) in enumerate(pool.map(lambda i: run_mutation(i, work), range(len(MUTATIONS)))):
            why = MUTATIONS[i][4] if len(MUTATIONS[i]) > 4 else None
            if failed:
                lines.append(f"{i + 1:2d}. {name}: caught by {len(failed)} tests" + (" (listed as equivalent: mend the list)" if why else ""))
                lines += [f"      {t}" for t in failed[:8]] + ([f"      ... and {len(failed) - 8} more"] if len(failed) > 8 else [])
            elif why:
                lines += [f"{i + 1:2d}. {name}: not caught", f"      {why}"]
            else:
                lines += [f"{i + 1:2d}. {name}: NOT CAUGHT", "      " + tail.replace("\n", "\n      ")]
                missed += 1
    lines.append(f"{len(MUTATIONS) - missed} of {len(MUTATIONS)} mutations caught or shown equivalent")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    return 1 if missed else 0


if __name__ == "__main__":
    sys.exit(main())
