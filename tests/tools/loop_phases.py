"""Phase table of the cursor engine's kernel (TEST TOOL) from a -DKSOLVE_PHASE_TIMERS build of the device library, shader-clock
cycles (or of the host emulation: the counts are the same, the cycles are the host's): where the time of the two loops and of the
driver's events goes, fast_slow_run's sections and the fast loop's exits per reason — the reader of phaseCycles slots 7 and 16..19
as FastCold::finish packs them (csrc/fast_engine.h). The shapes of profiles/loop_events.
    KSOLVE_TEST_SOLVER_LIB=1 python tests/tools/loop_phases.py LABEL LIB [LABEL LIB ...]
LIB: __graft_entry__.build_ksolve(LIB, defines=("-DKSOLVE_PHASE_TIMERS",)); with "-DKSOLVE_LOOP_TAIL=0" beside it, the engine whose
fast loop hands every pod that is not plain to fast_slow_run."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from karpenter_amd import fixtures as fx
from karpenter_amd.scheduling import NewScheduler

REASONS = ["sort-only", "no acceptor", "move past window", "class without slot", "cancel-poll boundary", "last entry / end", "pending at entry", "uncached set", "count limit"]


def table(label, lib, name, prob, solves=3):
    s = NewScheduler(prob, solver_lib=lib)
    r = s.Solve(repeat=solves, want_results=False)
    pc = r["counters"]["phaseCycles"]
    ms = [round(t["pack_kernel_ms"], 3) for t in r["timings"]]
    c = r["counters"]
    print(f"== {label} {name} pack ms {ms} pods {c['pods']} claims {c['claims']} slowSorts {c['slowSorts']} fullEvaluations {pc[21]}")
    tot = pc[6]
    nss, npl = pc[14] & 0xFFFFFFFF, pc[14] >> 32
    print(f"  total {tot}   fast loop (t_fast) {pc[8]} over {pc[9]} calls   one-pod loop (t_slow) {pc[10]} over {pc[11]} calls"
          f" ({pc[10] // max(1, pc[11])} each, {100.0 * pc[10] / tot:.2f}% of total)")
    print(f"  ev:refresh {pc[1]} ({pc[12]})  ev:slot {pc[2]} ({pc[13]}, {pc[2] // max(1, pc[13])} each)  ev:slowsort {pc[3]} ({nss}, {pc[3] // max(1, nss)} each)"
          f"  ev:place {pc[4]} ({npl}, {pc[4] // max(1, npl)} each)  ev:newclaim {pc[5]} ({pc[15]}, {pc[5] // max(1, pc[15])} each)")
    ts = [pc[16] & 0xFFFFFFFF, pc[16] >> 32, pc[17] & 0xFFFFFFFF, pc[17] >> 32]
    print(f"  one-pod loop sections: block fetch + pending move {ts[0]}  select {ts[1]}  commit {ts[2]}  refresh {ts[3]}  (entry + exit: {pc[10] - sum(ts)})")
    w = [pc[7], pc[18], pc[19]]
    print("  fast loop exits: " + ", ".join(f"{REASONS[i]} {(w[i // 3] >> (21 * (i % 3))) & 0x1FFFFF}" for i in range(9)))
    print(f"  slow_sort n<=64: calls {pc[20] >> 44} cycles {pc[20] & ((1 << 44) - 1)}", flush=True)
    s.close()


args = sys.argv[1:]
for label, lib in zip(args[0::2], args[1::2]):
    table(label, os.path.abspath(lib), "config2 20k seed42", fx.config2(pods=20000, n_types=500, seed=42))
    table(label, os.path.abspath(lib), "config2 1M seed42", fx.config2(pods=1_000_000, n_types=500, seed=42))
