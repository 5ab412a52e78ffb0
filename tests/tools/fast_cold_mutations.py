#!/usr/bin/env python3
"""Do the cases of tests/fast_cold_cases.py notice a wrong FastCold — setup(), compat_word, offering_cells, create_entry, the cache's
lookup and fit test, new_slot, new_claim, filter_diag? (CPU only; a tool, not a pytest test.)

Copies include/, karpenter_amd/, oracle/ and tests/ to a temporary directory once per mutation, applies ONE textual mutation to the
copy, builds the host emulation from it and runs tests/test_fast_cold.py there (the lanes-ascending half: the other lane order runs
the same code). One block per mutation: the tests that fail. A mutation whose search text does not occur exactly once is an error of
this tool (the source moved on: mend the list), never a pass; a mutation nothing catches makes the exit status 1, unless the list marks
it EQUIVALENT and says why. Nothing mutated is ever run on a GPU.

    python tests/tools/fast_cold_mutations.py [-j N] [--out profiles/fast_cold_tests/mutations.txt] [--check] [--only N ...]
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
    ("create_entry: dominance <= -> < in the first resource", "fast_engine.h", "bool le = eff[it] <= v0;", "bool le = eff[it] < v0;"),
    ("create_entry: dominance <= -> < in the last resource", "fast_engine.h", "if (nr > 3) le = le && eff[(size_t)3 * n_its + it] <= v3;", "if (nr > 3) le = le && eff[(size_t)3 * n_its + it] < v3;"),
    ("create_entry: the Pareto loop stops one vector early", "fast_engine.h", "if (count > kFastMaxPareto || n_pool >= kFastPool) return -1;", "if (count >= kFastMaxPareto || n_pool >= kFastPool) return -1;"),
    ("create_entry: the pool's last row refused", "fast_engine.h", "if (count > kFastMaxPareto || n_pool >= kFastPool) return -1;", "if (count > kFastMaxPareto || n_pool >= kFastPool - 1) return -1;"),
    ("create_entry: it < n_its dropped in the offering ballot", "fast_engine.h",
     "return it < n_its && ((in >> l) & 1) && (Pv.it_off_avail[it] & cells) != 0; }) : 0ull;\n      W::store(&its[j], okm);",
     "return ((in >> l) & 1) && (Pv.it_off_avail[it] & cells) != 0; }) : 0ull;\n      W::store(&its[j], okm);",
     "EQUIVALENT: `in` is a word of compat_word, an AND with t_its, whose bits past n_its are clear (setup() masks them with it < n_its and tmpl_its), and && tests the bit before it reads the table"),
    ("create_entry: the cache gate off by one", "fast_engine.h", "if (n_ent * 5 >= kFastEnt * 4) return -1;", "if (n_ent * 5 > kFastEnt * 4 + 4) return -1;"),
    ("create_entry: linear probing without wrap", "fast_engine.h", "while (ent[h].info & 1u) h = (h + 1) & (kFastEnt - 1);", "while (ent[h].info & 1u) h = h + 1;"),
    ("create_entry: the unused resources' capacity", "fast_engine.h", "int64_t v0 = 0x3FFFFFFF, v1 = 0x3FFFFFFF, v2 = 0x3FFFFFFF, v3 = 0x3FFFFFFF;", "int64_t v0 = 0x3FFFFFFF, v1 = 0x3FFFFFFF, v2 = 0x3FFFFFFF, v3 = 0;"),
    ("create_entry: the pool offset taken behind the vectors", "fast_engine.h", "((uint32_t)poff << 16);", "((uint32_t)n_pool << 16);"),
    ("create_entry: kFastExtBit never set", "fast_engine.h", "e.vmask = count > 1 ? (vm | kFastExtBit) : vm;", "e.vmask = vm;"),
    ("create_entry: the allocatable without the daemon overhead", "fast_engine.h", "const int64_t* eff = eff_alloc(P, tr);   // allocatable less the template's daemon overhead (ksp.h)", "const int64_t* eff = P.it_alloc;   //"),
    ("create_entry: the candidates not narrowed to the maximum", "fast_engine.h", "return it < n_its && ((in >> l) & 1) && al[it] == mx; }) : 0ull;", "return it < n_its && ((in >> l) & 1) && al[it] <= mx; }) : 0ull;"),
    ("fast_lookup: kFastExtBit not masked", "fast_engine.h", "if ((out.vmask & ~kFastExtBit) == vm) return (int)h;", "if (out.vmask == vm) return (int)h;"),
    ("fast_lookup: linear probing without wrap", "fast_engine.h", "    h = (h + 1) & (kFastEnt - 1);\n  }\n  return -1;", "    h = h + 1;\n  }\n  return -1;"),
    ("fast_fits: the pool offset dropped", "fast_engine.h", "o2 = o2 && size[r] <= pool[(off + i) * 4 + r] - req[r];", "o2 = o2 && size[r] <= pool[i * 4 + r] - req[r];"),
    ("fast_fits: the last Pareto vector lost", "fast_engine.h", "for (int i = 0; i < extra; ++i) {\n    bool o2 = true;", "for (int i = 0; i < extra - 1; ++i) {\n    bool o2 = true;"),
    ("fast_fits_first: <= -> < in the second resource", "fast_engine.h", "(int)(size[1] <= e.cap[1] - req[1])", "(int)(size[1] < e.cap[1] - req[1])"),
    ("fast_fields_ok: some field instead of every field", "fast_engine.h", "return (((m & dmask) + dmask) & g) == g;", "return (((m & dmask) + dmask) & g) != 0 || !g;"),
    ("compat_word: the guard-bit skip inverted", "fast_engine.h", "if ((vm >> (Mm.voff[j] + Mm.vwidth[j])) & 1) continue;   // guard bit set", "if (!((vm >> (Mm.voff[j] + Mm.vwidth[j])) & 1)) continue;   // guard bit set"),
    ("compat_word: key_neg dropped for the empty set", "fast_engine.h", "if (!field) r |= Pv.key_neg[(size_t)k * iw + w];", ""),
    ("compat_word: key_undef dropped", "fast_engine.h", "uint64_t r = Pv.key_undef[(size_t)k * iw + w];\n      if (!field)", "uint64_t r = 0;\n      if (!field)"),
    ("compat_word (pod operators): key_compl dropped", "fast_engine.h", "if (!((this->dne_vars >> j) & 1u)) {\n          r |= Pv.key_compl[(size_t)k * iw + w];", "if (!((this->dne_vars >> j) & 1u)) {"),
    ("compat_word (pod operators): the phantom bit read as a value", "fast_engine.h", "for (uint64_t dv = f & (fm >> 1); dv; dv &= dv - 1)", "for (uint64_t dv = f & (fm >> 2); dv; dv &= dv - 1)"),
    ("offering_cells: the wrong shift", "fast_engine.h", "cells |= (uint64_t)cts << (__builtin_ctz(z) * 4);\n    return cells;", "cells |= (uint64_t)cts << (__builtin_ctz(z) * 3);\n    return cells;"),
    ("offering_cells: the set's capacity types ignored", "fast_engine.h", "if (Mp->vkey[j] == d.key_ct) cts &= field;", ""),
    ("setup: the prefilter's cells with the wrong shift", "fast_engine.h", "cells |= (uint64_t)cts << (__builtin_ctz(z) * 4);\n      uint64_t any = 0;", "cells |= (uint64_t)cts << (__builtin_ctz(z) * 3);\n      uint64_t any = 0;"),
    ("setup: key_neg dropped (the NotIn / DoesNotExist escape)", "fast_engine.h", "if (op_negative(req_op(d, tr, k))) r |= Pv.key_neg[(size_t)k * iw + w];", ""),
    ("setup: key_compl dropped", "fast_engine.h", "if (comp) r |= Pv.key_compl[(size_t)k * iw + w];", ""),
    ("setup: it_alloc_ok dropped", "fast_engine.h", "uint64_t acc = tin[w] & Pv.it_alloc_ok[w];", "uint64_t acc = tin[w];"),
    ("setup: it < n_its dropped in the prefilter's offering ballot", "fast_engine.h",
     "return it < n_its && ((in >> l) & 1) && (Pv.it_off_avail[it] & cells) != 0; }) : 0ull;\n        W::store(&tits[j], okm);",
     "return ((in >> l) & 1) && (Pv.it_off_avail[it] & cells) != 0; }) : 0ull;\n        W::store(&tits[j], okm);",
     "EQUIVALENT where tmpl_its has no bit past n_its, which is what create() uploads and what the cases hold: && tests the bit before it reads the table"),
    ("setup: tmplok ignores well_known_mask", "fast_engine.h", "if (!(Pv.tmpl_taints[t] & ~tol) && !(kdef & ~Mm.tdef[t] & ~wk)) ok |= 1u << t;", "if (!(Pv.tmpl_taints[t] & ~tol) && !(kdef & ~Mm.tdef[t])) ok |= 1u << t;"),
    ("setup: tmplok ignores the taints", "fast_engine.h", "if (!(Pv.tmpl_taints[t] & ~tol) && !(kdef & ~Mm.tdef[t] & ~wk)) ok |= 1u << t;", "if (!(kdef & ~Mm.tdef[t] & ~wk)) ok |= 1u << t;"),
    ("setup (pod operators): Exists against DoesNotExist passes", "fast_engine.h", "if (((kexists >> k) & 1u) ? top == OP_DNE : !op_negative(top)) v = false;", "if (((kexists >> k) & 1u) ? false : !op_negative(top)) v = false;"),
    ("setup (pod operators): a DoesNotExist class without the phantom bit", "fast_engine.h", "if (!comp) { f = ph; kdne |= 1u << k; kpos &= ~(1u << k); }", "if (!comp) { f = 0; kdne |= 1u << k; kpos &= ~(1u << k); }"),
    ("setup: an undefined key without its guard bit", "fast_engine.h", "else vm |= Mm.fmask[j] | guard;   // undefined", "else vm |= Mm.fmask[j];   // undefined"),
    ("setup: the width without the phantom bit", "fast_engine.h", "(valid ? 64 - __builtin_clzll(valid) : 1) + (pod_ops ? 1 : 0);", "(valid ? 64 - __builtin_clzll(valid) : 1);"),
    ("setup: no guard bit between the fields", "fast_engine.h", "bits += width + 1;   // + the guard bit", "bits += width;   // + the guard bit"),
    ("setup: 57 packed bits pass", "fast_engine.h", "if (bits + width + 1 > kFastVarBits) return DECLINE_KEYS_DO_NOT_PACK;", "if (bits + width > kFastVarBits) return DECLINE_KEYS_DO_NOT_PACK;"),
    ("setup: 13 variable keys pass", "fast_engine.h", "|| nv >= kFastMaxVar) return DECLINE_KEYS_DO_NOT_PACK;", "|| nv > kFastMaxVar) return DECLINE_KEYS_DO_NOT_PACK;"),
    ("setup: a request of 2^30 passes", "fast_engine.h", "return (uint64_t)((a >= (1ll << 30) || a < 0) ? 1 : 0); })) return DECLINE_QUANTITY_RANGE;", "return (uint64_t)((a > (1ll << 30) || a < 0) ? 1 : 0); })) return DECLINE_QUANTITY_RANGE;"),
    ("setup: the effective allocatable's range not tested", "fast_engine.h", "if (!((P.tmpl_ov >> t) & 1u)) continue;\n      const int64_t* eff = eff_alloc(P, t);", "continue;\n      const int64_t* eff = eff_alloc(P, t);"),
    ("setup: the class's In [] passes", "fast_engine.h", "if (!f) badc = 1;   // In [] == DoesNotExist: not positive", ""),
    ("setup: DECLINE_CLASS_DNE_MIXED ignores the NodePools' NotIn", "fast_engine.h", "if (kop[OP_DNE] & (kop[OP_NOTIN] | t_notin)) return DECLINE_CLASS_DNE_MIXED;", "if (kop[OP_DNE] & kop[OP_NOTIN]) return DECLINE_CLASS_DNE_MIXED;"),
    ("new_slot: the fullest row among equals", "fast_engine.h", "const int score = popc64(friends) * 128 + (64 - popc64(used));", "const int score = popc64(friends) * 128 + popc64(used);"),
    ("new_slot: the last free lane", "fast_engine.h", "if (fr) slot = j * 64 + ctz64(fr);", "if (fr) slot = j * 64 + 63 - __builtin_clzll(fr);"),
    ("new_slot: kFastExtBit ignored in the one-compare test", "fast_engine.h", "const uint64_t simm = W::ballot([&](int l) { return evm.at(l) == mlv.at(l); });\n      const uint64_t fitm = W::ballot([&](int l) { return (rec.size[0]",
     "const uint64_t simm = W::ballot([&](int l) { return (evm.at(l) & ~kFastExtBit) == mlv.at(l); });\n      const uint64_t fitm = W::ballot([&](int l) { return (rec.size[0]"),
    ("row_accepts: tmplok not tested", "fast_engine.h", "if (!((s.tmplok >> t) & 1u)) return 0;\n        const uint64_t m = st.vmask & s.cvmask;", "const uint64_t m = st.vmask & s.cvmask;"),
    ("new_claim: the hostname number not counted", "fast_engine.h", "      host_seq++;\n      n_ref_extra++;", "      n_ref_extra++;"),
    ("new_claim: taints and incompatibility swapped", "fast_engine.h", "? E_TAINTS : E_INCOMPATIBLE;", "? E_INCOMPATIBLE : E_TAINTS;"),
    ("new_claim: the retry's net dropped", "fast_engine.h", "if (retry) { bail_code = DECLINE_UNSCHEDULABLE_POD; return 0; }", ""),
    ("new_claim: a kept verdict without its hostname numbers", "fast_engine.h", "host_seq += tried; n_ref_extra += (unsigned long long)tried;", "n_ref_extra += (unsigned long long)tried;"),
    ("new_claim: one claim more than max_claims", "fast_engine.h", "if (n_claims >= S.max_claims) { bail_code = DECLINE_KERNEL_CAPACITY; return 0; }", "if (n_claims > S.max_claims) { bail_code = DECLINE_KERNEL_CAPACITY; return 0; }"),
    ("filter_diag: fits without requirements -> with", "fast_engine.h", "d_fo |= (itfits & ~cm) != 0;", "d_fo |= (itfits & cm) != 0;"),
    ("filter_diag: a type fits without a compatible offering", "fast_engine.h", "const uint64_t itfits = off & W::ballot([&](int l) {", "const uint64_t itfits = in & W::ballot([&](int l) {"),
    ("limit_stage_id: the stage's tvmask keeps the template's id", "fast_engine.h", "Mp->tvmask[s] = (Mp->tvmask[t] & ~(0xFFull << 56)) | ((uint64_t)s << 56);", "Mp->tvmask[s] = Mp->tvmask[t];"),
    ("limit_stage_id: first_claim overwritten", "fast_engine.h", "if (differs && W::leader() && lim->first_claim == 0xFFFFFFFFu) lim->first_claim", "if (differs && W::leader()) lim->first_claim"),
    ("limit_stage_id: the template's current stage not moved on", "fast_engine.h", "lim->real[s] = (uint8_t)t; lim->cur[t] = (uint8_t)s; lim->n_ids", "lim->real[s] = (uint8_t)t; lim->n_ids"),
    ("limit_stage_id: a capacity equal to the remaining excluded", "fast_engine.h", "v = v && Pv.it_cap[(size_t)q * n_its + it] <= rem[q];\n      return v;", "v = v && Pv.it_cap[(size_t)q * n_its + it] < rem[q];\n      return v;"),
    ("limit_stage_id: a pool with no node left goes on", "fast_engine.h", "if (((lm >> nr) & 1) && rem[nr] <= 0) return -1;", "if (((lm >> nr) & 1) && rem[nr] < 0) return -1;"),
    ("limit_stage: tmplok not copied to the stage's bit in the class records", "fast_engine.h", "fc[c].tmplok = k | (((k >> t) & 1u) << s); });", "fc[c].tmplok = k; });"),
    ("limit_stage: tmplok not copied to the stage's bit in the slots", "fast_engine.h", "as[i].tmplok = k | (((k >> t) & 1u) << s); });", "as[i].tmplok = k; });"),
    ("limits_exclude: a capacity equal to the remaining excluded", "fast_engine.h", "v = v && Pv.it_cap[(size_t)q * n_its + it] <= rem[q];\n      return !v;", "v = v && Pv.it_cap[(size_t)q * n_its + it] < rem[q];\n      return !v;"),
    ("limits_exclude: a pool with no node left goes on", "fast_engine.h", "if (((lm >> nr) & 1) && rem[nr] <= 0) return DECLINE_LIMIT_NODES;", "if (((lm >> nr) & 1) && rem[nr] < 0) return DECLINE_LIMIT_NODES;"),
    ("subtract_max: over F without the fit", "fast_engine.h", "for (int z = 0; z < nr; ++z) if (eff[(size_t)z * n_its + it] < (int64_t)size[z]) return INT64_MIN;", ""),
    ("subtract_max: the allocatable for the capacity", "fast_engine.h", "return Pv.it_cap[(size_t)q * n_its + it];\n    });\n    W::store(&rem[q], rem[q] - mx);", "return Pv.it_alloc[(size_t)q * n_its + it];\n    });\n    W::store(&rem[q], rem[q] - mx);"),
    ("new_claim: us_epoch not bumped", "fast_engine.h", "if constexpr (US) if (lm) this->us_epoch++;", ""),
    ("new_claim: a skipped template leaves no E_LIMITS", "fast_engine.h", "if (ts == -1) { if (!first_err) first_err = E_LIMITS; continue; }", "if (ts == -1) { continue; }"),
    ("new_claim: the hostname number counted for a skipped template", "fast_engine.h", "if (ts == -1) { if (!first_err) first_err = E_LIMITS; continue; }", "if (ts == -1) { if (!first_err) first_err = E_LIMITS; host_seq++; continue; }"),
    ("new_claim: the claim carries the template's id under a stage", "fast_engine.h", "const uint64_t m = Mp->tvmask[ts] & cs.cvmask;", "const uint64_t m = Mp->tvmask[t] & cs.cvmask;"),
    ("create_entry: a stage reads its own overhead row", "fast_engine.h", "const int tr = F.lim ? (int)F.lim->real[t] : t;   // t may be a limit stage (FastLimits): its row of t_its, the template's requirements and overhead", "const int tr = t < P.n_templates ? t : 0;   //"),
    ("eff_alloc: the last matching group", "kernels.h", "for (int x = g0; x < g1 && g < 0; ++x)", "for (int x = g0; x < g1; ++x)"),
]


def checked(i):
    name, fname, old, new = MUTATIONS[i][:4]
    with open(os.path.join(ROOT, "karpenter_amd", "csrc", fname)) as f:
        n = f.read().count(old)
    if n != 1:
        raise SystemExit(f"mutation {i + 1} ({name}): its search text occurs {n} times in {fname}")


def run_mutation(i, work):
    name, fname, old, new = MUTATIONS[i][:4]
    d = os.path.join(work, f"m{i + 1:02d}")
    for sub in ("include", "karpenter_amd", "oracle", "tests"):
        shutil.copytree(os.path.join(ROOT, sub), os.path.join(d, sub), ignore=shutil.ignore_patterns("_obj", "_ref", "*.so", "__pycache__", "*.lock", "*.tmp", "fullsize", "sweeps", "go_dump"))
    shutil.copy(os.path.join(ROOT, "__graft_entry__.py"), d)
    path = os.path.join(d, "karpenter_amd", "csrc", fname)
    with open(path) as f:
        text = f.read()
    with open(path, "w") as f:
        f.write(text.replace(old, new))
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-o", os.path.join(d, "tests", "emu", "libksolve_emu.so"), os.path.join(d, "tests", "emu", "ksolve_emu.cpp")])
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_fast_cold.py", "-k", "ascending", "-q", "-p", "no:cacheprovider", "--tb=no", "-rf"], cwd=d, capture_output=True, text=True)
    shutil.rmtree(d, ignore_errors=True)
    failed = re.findall(r"^FAILED (\S+.*)", r.stdout, re.M)
    if not failed and not re.search(r"\d+ passed", r.stdout):
        failed = [f"(the test process died with exit status {r.returncode} before its summary: the mutation writes past a table)"]
    return name, failed, r.stdout[-400:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-j", type=int, default=4)
    ap.add_argument("--out")
    ap.add_argument("--check", action="store_true", help="only check that every search text occurs exactly once")
    ap.add_argument("--only", type=int, nargs="*", help="run these mutations alone (numbers as the report prints them)")
    args = ap.parse_args()
    for i in range(len(MUTATIONS)):
        checked(i)
    if args.check:
        return 0
    lines, missed = [], 0
    with tempfile.TemporaryDirectory() as work, ThreadPoolExecutor(max_workers=args.j) as pool:
        picked = [n - 1 for n in args.only] if args.only else list(range(len(MUTATIONS)))
        for i, (name, failed, tail) in zip(picked, pool.map(lambda i: run_mutation(i, work), picked)):
            why = MUTATIONS[i][4] if len(MUTATIONS[i]) > 4 else None
            if failed:
                lines.append(f"{i + 1:2d}. {name}: caught by {len(failed)} tests" + (" (listed as equivalent: mend the list)" if why else ""))
                lines += [f"      {t}" for t in failed[:6]] + ([f"      ... and {len(failed) - 6} more"] if len(failed) > 6 else [])
            elif why:
                lines += [f"{i + 1:2d}. {name}: not caught", f"      {why}"]
            else:
                lines += [f"{i + 1:2d}. {name}: NOT CAUGHT", "      " + tail.replace("\n", "\n      ")]
                missed += 1
    lines.append(f"{len(picked) - missed} of {len(picked)} mutations caught or shown equivalent")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    return 1 if missed else 0


if __name__ == "__main__":
    sys.exit(main())
