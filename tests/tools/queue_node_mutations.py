#!/usr/bin/env python3
"""Do the cases of tests/queue_cases.py and tests/node_row_cases.py notice a wrong queue order, queue marking or node row? (CPU only;
a tool, not a pytest test.)

Copies include/, karpenter_amd/ and tests/ to a temporary directory once per mutation, applies ONE textual mutation to the copy,
builds the host emulation from it and runs tests/test_queue_kernels.py and tests/test_node_rows.py there. One block per mutation:
the tests that fail. A mutation whose search text does not occur exactly once is an error of this tool (the source moved on: mend
the list), never a pass; a mutation nothing catches makes the exit status 1. Nothing mutated is ever run on a GPU.

    python tests/tools/queue_node_mutations.py [-j N] [--out profiles/queue_node_tests/mutations.txt]
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

# (name, file under karpenter_amd/csrc, search text, replacement)
MUTATIONS = [
    ("sort_key_body: pass 3 (memory) without the ~", "kernels.h",
     "case 3: k = ~((uint64_t)a.requests[(size_t)1 * a.n_rows + p] ^ 0x8000000000000000ull); break;", "case 3: k = ((uint64_t)a.requests[(size_t)1 * a.n_rows + p] ^ 0x8000000000000000ull); break;"),
    ("sort_key_body: pass 2 (creation) without the sign bias", "kernels.h",
     "case 2: k = (uint64_t)a.creation[p] ^ 0x8000000000000000ull; break;", "case 2: k = (uint64_t)a.creation[p]; break;"),
    ("sort_key_body: pass 1 reads uid_lo", "kernels.h", "case 1: k = a.uid_hi[p]; break;", "case 1: k = a.uid_lo[p]; break;"),
    ("fast_mark_body: compares with cls_first", "fast_engine.h",
     "if (a.cls_last[c] == (uint32_t)i) a.q_class[i] = c | kFastLastBit;", "if (a.cls_first[c] == (uint32_t)i) a.q_class[i] = c | kFastLastBit;"),
    ("fast_overlap_body: < for <=", "fast_engine.h",
     "live += (uint32_t)((a.cls_first[o] <= f) & (a.cls_last[o] >= f));", "live += (uint32_t)((a.cls_first[o] < f) & (a.cls_last[o] >= f));"),
    ("node_dead0_body: stores ok for ~ok", "kernels.h",
     "W::store(&a.dead0[(size_t)k * a.node_words + block], (uint64_t)~ok);", "W::store(&a.dead0[(size_t)k * a.node_words + block], (uint64_t)ok);"),
    ("node_dead0_body: l < cnt dropped from the ballot", "kernels.h", "return l < cnt && node_static_ok_pre(", "return node_static_ok_pre("),
    ("node_dead0_body: k1 = k0 + 1", "kernels.h", "k1 = k0 + kDead0Classes < a.n_classes ? k0 + kDead0Classes : a.n_classes;", "k1 = k0 + 1;"),
    ("node_static_ok_pre: rem >= 0 dropped", "nodecheck.h",
     "for (int r = 0; r < kMaxRes; ++r) if (r < ly.nr) { const int64_t rem = n.rem[r]; fit = fit && rem >= 0 && x.req[r] <= rem; }",
     "for (int r = 0; r < kMaxRes; ++r) if (r < ly.nr) { const int64_t rem = n.rem[r]; fit = fit && x.req[r] <= rem; }"),
    ("node_reqs_ok: & ~x.kneg dropped", "nodecheck.h", "if (x.kdef & ~ndef & ~x.kneg) return false;", "if (x.kdef & ~ndef) return false;"),
    ("node_preload: rem[r] for r < ly.nr - 1", "nodecheck.h", "n.rem[r] = r < ly.nr ? t.remaining", "n.rem[r] = r < ly.nr - 1 ? t.remaining"),
]


def run_mutation(i, work):
    name, fname, old, new = MUTATIONS[i]
    d = os.path.join(work, f"m{i + 1:02d}")
    for sub in ("include", "karpenter_amd", "tests"):
        shutil.copytree(os.path.join(ROOT, sub), os.path.join(d, sub), ignore=shutil.ignore_patterns("_obj", "*.so", "__pycache__", "*.lock", "*.tmp"))
    shutil.copy(os.path.join(ROOT, "__graft_entry__.py"), d)
    path = os.path.join(d, "karpenter_amd", "csrc", fname)
    with open(path) as f:
        text = f.read()
    if text.count(old) != 1:
        raise SystemExit(f"mutation {i + 1} ({name}): its search text occurs {text.count(old)} times in {fname}")
    with open(path, "w") as f:
        f.write(text.replace(old, new))
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-o", os.path.join(d, "tests", "emu", "libksolve_emu.so"), os.path.join(d, "tests", "emu", "ksolve_emu.cpp")])
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_queue_kernels.py", "tests/test_node_rows.py", "-q", "-p", "no:cacheprovider", "--tb=no", "-rf"],
                       cwd=d, capture_output=True, text=True)
    return name, re.findall(r"^FAILED (\S+)", r.stdout, re.M), r.stdout[-400:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-j", type=int, default=4)
    ap.add_argument("--out")
    args = ap.parse_args()
    lines, missed = [], 0
    with tempfile.TemporaryDirectory() as work, ThreadPoolExecutor(max_workers=args.j) as pool:
        for i, (name, failed, tail) in enumerate(pool.map(lambda i: run_mutation(i, work), range(len(MUTATIONS)))):
            lines.append(f"{i + 1:2d}. {name}: " + (f"caught by {len(failed)} tests" if failed else "NOT CAUGHT"))
            lines += [f"      {t}" for t in failed] or ["      " + tail.replace("\n", "\n      ")]
            missed += not failed
    lines.append(f"{len(MUTATIONS) - missed} of {len(MUTATIONS)} mutations caught")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    return 1 if missed else 0


if __name__ == "__main__":
    sys.exit(main())
