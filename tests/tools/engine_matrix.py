"""The engine-option matrix (TEST TOOL; tests/test_engine_matrix.py on the emulation, tests/test_gpu_engine_matrix.py on the
device): a fixed list of small problems — the smallest shapes of the case modules — solved under EVERY value of
ksolve_options.engine, each one alone (Solve) and as a member of one SolveBatch of the whole list under that setting, always on
fresh handles. Per (problem, setting, alone / batch) one cell: ok or the exception class, the full error text, counters.engine,
engineFallbackReason, cursorMemoryPlan, cursorAttempts and parity.results_digest. Values 0-16 go in by name through the host
library; 17, a value past the table that no name stands for, goes in as a number (options.engine = 17, which the host library hands
on as it is).

The record is tests/golden/engine_matrix.json: {"emulation": {cell: {...}}, "device": {cell: {...}}}; "device" holds only the
cells that differ from the emulation's. It is taken from the commit BEFORE a change to the engine option's decoding, never from the
code under test (where that commit's host library takes names only, with the one line that hands a number on added to it: the solver
library, which decodes the value, is that commit's):
  python tests/tools/engine_matrix.py --record emulation        (host emulation, no GPU)
  python tests/tools/engine_matrix.py --record device           (on the MI355X)
  python tests/tools/engine_matrix.py --coverage                (what the recorded cells exercise)

A second, separate record pins the settings that came after that one, rows 18-27, 29, 30, 32 and 33 of csrc/engine_setting.h
(LATE_SETTINGS), over eleven small problems of the later engines' shapes (late_problems()) and in THREE ways: alone, batch, and "many" —
one SolveMany of the setting's eleven problems on fresh handles (solve_many_cases.matrix_cells). It is
tests/golden/engine_matrix_late.json, in the same layout with the same seven fields, taken from the commit BEFORE the three call
ladders of Solve, SolveBatch and SolveMany were put on one set of steps (csrc/solve_calls.h), with nothing but this tool's lines for
it added to that commit: the batch's cells that differ from the lone ones are its behaviour as it was, and stay.
  python tests/tools/engine_matrix.py --record emulation --late
  python tests/tools/engine_matrix.py --record device --late
  python tests/tools/engine_matrix.py --coverage --late"""
import argparse
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(ROOT, "tests", "golden", "engine_matrix.json")
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
os.environ.setdefault("KSOLVE_TEST_SOLVER_LIB", "1")

# value -> the name the host library accepts (include/ksolve.h, ksolve_options.engine)
SETTINGS = ["auto", "general", "cursor", "cursor-wide", "cursor-hbm", "cursor-pair", "spread", "auto-nodes", "cursor-nodes", "auto-nodes-spread", "spread-nodes",
            "auto-limits", "cursor-limits", "auto-limits-spread", "spread-limits", "auto-operators", "cursor-operators", 17]
# rows 18-27, 29, 30, 32 and 33 of csrc/engine_setting.h (28 and 31 have no row of their own)
LATE_SETTINGS = ["auto-operators-spread", "spread-operators", "auto-unschedulable", "cursor-unschedulable", "auto-unschedulable-spread", "spread-unschedulable",
                 "auto-filters-spread", "spread-filters", "auto-pod-operators", "cursor-pod-operators", "auto-pod-operators-spread", "spread-pod-operators",
                 "auto-pod-operators-nodes", "cursor-pod-operators-nodes"]
LATE_FIXTURE = os.path.join(ROOT, "tests", "golden", "engine_matrix_late.json")
WAYS = ("alone", "batch")
LATE_WAYS = ("alone", "batch", "many")
FIELDS = ("outcome", "error", "engine", "engineFallbackReason", "cursorMemoryPlan", "cursorAttempts", "digest")


def problems():
    """[(name, problem)]. fixtures.pod() numbers its uids from a process-wide counter, and uids are part of the queue order and of the
    digest: the list is built from uid 1 whatever ran before in the process, as it was when the record was taken."""
    from karpenter_amd import fixtures as fx
    before, fx._uid_counter[0] = fx._uid_counter[0], 0
    try:
        return _problems(fx)
    finally:
        fx._uid_counter[0] = max(before, fx._uid_counter[0])   # (no uid handed out twice to whoever builds problems next)


def late_problems():
    """[(name, problem)] of the late record, built from uid 1 as problems() builds its list. Eleven: "spread-mix-daemonsets" is there
    for the batch's DaemonSet condition, which no other of them meets on its own; "escalation-open", which the record of settings 0-17
    has, made room for it (with both, the record would be larger than that one)."""
    from karpenter_amd import fixtures as fx
    before, fx._uid_counter[0] = fx._uid_counter[0], 0
    try:
        return _late_problems(fx)
    finally:
        fx._uid_counter[0] = max(before, fx._uid_counter[0])


def _late_problems(fx):
    import pod_operator_cases as po
    import pod_operator_node_cases as pn
    import spread_filter_cases as sf
    import spread_limit_cases as sl
    import spread_node_cases as sn
    import spread_operator_cases as so
    import spread_pod_operator_cases as sp
    import spread_unschedulable_cases as su
    import unschedulable_cases as uc
    plain = fx.config1()
    plain = dict(plain, pods=plain["pods"][:40])
    return [("plain", plain),
            ("spread-mix", sl.mix_problem((300, 144, 1), None)),
            ("spread-mix-nodes", sn.mix_problem((300, 144, 1), 5)),
            ("spread-mix-daemonsets", sn.mix_problem((300, 144, 1), 0, daemonsets=True)),   # (no node: DaemonSets are all that sets it apart from spread-mix)
            ("spread-complement", so.counted_problem()),
            ("pinned", uc.pinned_problem()),
            ("chain-web", su.chain_web_problem()),
            ("filter-never", sf.never_problem()),
            ("zone-notin", po.zone_notin_problem()),
            ("spread-pod-notin", sp.counted_problem()),
            ("dedicated-nodes", pn.dedicated_problem())]


def _problems(fx):
    import limit_cases as lc
    import operator_cases as oc
    import spread_limit_cases as sl
    import spread_node_cases as sn
    plain = fx.config1()
    plain = dict(plain, pods=plain["pods"][:40])
    return [("plain", plain),
            ("plain-nodes", fx.with_existing_nodes(plain, 4, seed=1)),
            ("cpu-chain", lc.cpu_chain_problem(True)),
            ("stage-chain-4", lc.stage_chain_problem(4)),
            ("notin", oc.notin_problem()),
            ("bounds", oc.bounds_problem()),
            ("min-values", oc.min_values_problem()),
            ("pod-gt", oc.pod_gt_problem()),
            ("spread-mix", sl.mix_problem((300, 144, 1), None)),
            ("spread-mix-limit", sl.mix_problem((300, 144, 1), {"cpu": "100"})),
            ("spread-mix-nodes", sn.mix_problem((300, 144, 1), 5)),
            ("many-classes", lc.many_classes_problem()),
            ("escalation", lc.escalation_problem(3200)),
            ("escalation-open", _without_limits(lc.escalation_problem(3600)))]


def _without_limits(prob):
    """escalation_problem(3600) without its limit: 3,600 claims, and a lower bound of them (create()'s, from the requests alone) past
    the LDS plan's capacity — the settings that choose the first plan start on plan 1, "cursor-pair" gets there by reason 26."""
    return dict(prob, nodePools=[{k: v for k, v in p.items() if k != "limits"} for p in prob["nodePools"]])


def _cell(doc=None, exc=None):
    if exc is not None:
        return {"outcome": type(exc).__name__, "error": str(exc), "engine": None, "engineFallbackReason": None, "cursorMemoryPlan": None, "cursorAttempts": None, "digest": None}
    import parity
    c = doc["counters"]
    return {"outcome": "ok", "error": "", "engine": c["engine"], "engineFallbackReason": c["engineFallbackReason"], "cursorMemoryPlan": c["cursorMemoryPlan"],
            "cursorAttempts": c["cursorAttempts"], "digest": parity.results_digest(doc)[0]}


def _solve_batch(schedulers):
    """scheduling.SolveBatch, but every member's document on its own: one member's refusal does not hide the others' results."""
    from karpenter_amd import scheduling as sch
    lib, n = schedulers[0]._lib, len(schedulers)
    sessions = (ctypes.c_void_p * n)(*[s._session for s in schedulers])
    outs = (ctypes.c_void_p * n)()
    lib.ksched_solve_batch(sessions, n, sch._want(True), outs)
    cells = []
    for i in range(n):
        try:
            doc = json.loads(ctypes.string_at(outs[i]).decode())
        finally:
            lib.ksched_free(outs[i])
        try:
            if "error" in doc:
                sch._raise(doc.get("kind"), doc["error"])
            cells.append(_cell(sch.Results(doc)))
        except Exception as e:
            cells.append(_cell(exc=e))
    return cells


def build_matrix(solver_lib=None, progress=False, settings=None, probs=None, ways=WAYS):
    """{cell: {field: value}} for every problem (problems(), or `probs`), setting (SETTINGS, or `settings`) and way of solving ("many":
    solve_many_cases.matrix_cells). solver_lib: the emulation; None = the device library."""
    from karpenter_amd.scheduling import NewScheduler
    probs = problems() if probs is None else probs
    out = {}
    if "many" in ways:
        import solve_many_cases
        out.update(solve_many_cases.matrix_cells(solver_lib, SETTINGS if settings is None else settings, probs, way="many"))

    def open_all(setting):
        opened = []
        for name, prob in probs:
            try:
                opened.append((name, NewScheduler(dict(prob, options=dict(prob.get("options", {}), engine=setting)), solver_lib=solver_lib), None))
            except Exception as e:
                opened.append((name, None, e))
        return opened

    for setting in (SETTINGS if settings is None else settings):
        if progress:
            print(f"engine_matrix: {setting}", file=sys.stderr, flush=True)
        for name, s, err in open_all(setting):
            if s is None:
                out[f"{name}|{setting}|alone"] = _cell(exc=err)
                continue
            try:
                out[f"{name}|{setting}|alone"] = _cell(s.Solve())
            except Exception as e:
                out[f"{name}|{setting}|alone"] = _cell(exc=e)
            finally:
                s.close()
        opened = open_all(setting)
        live = [(name, s) for name, s, _ in opened if s is not None]
        for name, s, err in opened:
            if s is None:
                out[f"{name}|{setting}|batch"] = _cell(exc=err)
        try:
            for (name, _), cell in zip(live, _solve_batch([s for _, s in live])):
                out[f"{name}|{setting}|batch"] = cell
        finally:
            for _, s in live:
                s.close()
    return out


def differences(got, want):
    """[(cell, field, got, want)] over the union of the cells, field by field."""
    out = []
    for cell in sorted(set(got) | set(want)):
        g, w = got.get(cell), want.get(cell)
        if g is None or w is None:
            out.append((cell, "<cell>", g is not None, w is not None))
            continue
        out += [(cell, f, g[f], w[f]) for f in FIELDS if g[f] != w[f]]
    return out


def build_late(solver_lib=None, progress=False, settings=None):
    """The late matrix: late_problems() under LATE_SETTINGS (or `settings` of them), alone, batch and many."""
    return build_matrix(solver_lib, progress, LATE_SETTINGS if settings is None else settings, late_problems(), LATE_WAYS)


def load(key, fixture=FIXTURE):
    """The recorded matrix for "emulation" or "device" (the emulation's cells overlaid with the device's differing ones)."""
    with open(fixture) as f:
        doc = json.load(f)
    cells = {k: dict(v) for k, v in doc["emulation"].items()}
    if key == "device":
        for k, v in doc.get("device", {}).items():
            cells[k] = dict(v)
    return cells


# setting pairs that differ in ONE switch of the option (include/ksolve.h): some cell has to differ between them
SWITCH_PAIRS = {"nodes": ("auto", "auto-nodes"), "spread_nodes": ("auto-nodes", "auto-nodes-spread"), "limits": ("auto-nodes", "auto-limits"),
                "spread_limits": ("spread-nodes", "spread-limits"), "operators": ("cursor-limits", "cursor-operators")}
MESSAGES = {"cursor declined": "cursor engine declined the problem (reason ", "spread declined": "spread engine declined the problem (reason ",
            "cursor outside shape": "cursor engine requested for a problem outside its shape (topology", "spread outside shape": "spread engine requested for a problem outside its shape (no topology",
            "batch outside shape": "cursor engine requested for a problem outside its shape"}


def coverage(cells):
    """What the matrix exercises, as {claim: [cells]}: every claim needs at least one cell."""
    names = [n for n, _ in problems()]
    cov = {}
    def where(pred):
        return [k for k, v in sorted(cells.items()) if pred(k, v)]
    setting_of = lambda k: k.split("|")[1]
    cov["run Auto falls back"] = where(lambda k, v: setting_of(k) == "auto" and v["engine"] == "general" and v["engineFallbackReason"])
    cov["run General"] = where(lambda k, v: setting_of(k) == "general" and v["engine"] == "general")
    cov["run Cursor refuses"] = where(lambda k, v: setting_of(k) == "cursor" and v["outcome"] == "Unsupported")
    cov["run Cursor solves"] = where(lambda k, v: setting_of(k) == "cursor" and v["engine"] == "cursor")
    cov["run Spread refuses"] = where(lambda k, v: setting_of(k) == "spread" and v["outcome"] == "Unsupported")
    cov["run Spread solves"] = where(lambda k, v: setting_of(k) == "spread" and v["engine"] == "spread")
    # 17: the cursor engine only (solves, refuses in both texts), and it does NOT choose its first plan as "cursor" does
    cov["past the table: solves on the cursor engine"] = where(lambda k, v: setting_of(k) == "17" and v["engine"] == "cursor")
    cov["past the table: refuses, declined"] = where(lambda k, v: setting_of(k) == "17" and MESSAGES["cursor declined"] in v["error"])
    cov["past the table: refuses, outside shape"] = where(lambda k, v: setting_of(k) == "17" and MESSAGES["cursor outside shape"] in v["error"])
    cov["past the table: first plan not chosen"] = where(lambda k, v: setting_of(k) == "17" and v["cursorAttempts"] == 2 and cells[k.replace("|17|", "|cursor|")]["cursorAttempts"] == 1)
    for plan, setting in ((1, "cursor-wide"), (2, "cursor-hbm")):
        cov[f"first plan {plan}"] = where(lambda k, v: setting_of(k) == setting and v["cursorMemoryPlan"] == plan)
    cov["first plan chosen by the library"] = where(lambda k, v: setting_of(k) in ("auto", "cursor") and (v["engine"], v["cursorMemoryPlan"], v["cursorAttempts"]) == ("cursor", 1, 1))
    cov["first plan outgrown (reason 26)"] = where(lambda k, v: v["engine"] == "cursor" and v["cursorAttempts"] == 2)
    for switch, (a, b) in SWITCH_PAIRS.items():
        cov[f"switch {switch}"] = [f"{n}|{b}|{how}" for n in names for how in ("alone", "batch") if cells[f"{n}|{a}|{how}"] != cells[f"{n}|{b}|{how}"]]
    for what, text in MESSAGES.items():
        if what == "batch outside shape":
            cov[what] = where(lambda k, v: v["error"].endswith(text))
            cov["batch outside shape, spread-only handle"] = where(lambda k, v: v["error"].endswith(text) and str(setting_of(k)).startswith("spread"))
        else:
            cov[what] = where(lambda k, v: text in v["error"])
    # the batch path: a cursor handle run alone by solve() (existing-node stage, limit stages, a plan in HBM) and one the batched kernel hands back
    cov["batch: alone"] = where(lambda k, v: k.endswith("|batch") and v["engine"] == "cursor" and (setting_of(k) in ("cursor-wide", "cursor-hbm", "cursor-nodes", "cursor-limits")))
    cov["batch: handed back"] = where(lambda k, v: k.endswith("|batch") and setting_of(k) == "auto" and v["engine"] == "general" and v["engineFallbackReason"] in (23, 24))
    cov["batch: handed back, refused"] = where(lambda k, v: k.endswith("|batch") and setting_of(k) == "cursor" and MESSAGES["cursor declined"] in v["error"])
    cov["batch: out of claim slots, alone"] = where(lambda k, v: k.endswith("|batch") and v["engine"] == "cursor" and v["cursorAttempts"] == 2)
    return cov


def late_coverage(cells):
    """What the late matrix exercises, as {claim: [cells]}: every claim needs at least one cell. A cell does not say which branch of a
    driver its handle took; each claim below names the problem and the settings whose handle create() shapes so that only that branch
    can give the recorded engine."""
    cov = {}
    def where(pred):
        return [k for k, v in sorted(cells.items()) if pred(*k.split("|"), v)]
    spread_only = lambda s: s.startswith("spread-")
    solved = lambda v, engine: v["outcome"] == "ok" and v["engine"] == engine and v["engineFallbackReason"] == 0
    no_many_kernel = ("auto-pod-operators-spread", "spread-pod-operators", "auto-pod-operators-nodes")   # (the settings with spread_pod_operators)
    # SolveMany, the spread engine
    cov["many: a spread member in a shared launch"] = where(lambda n, s, w, v: w == "many" and n == "spread-mix" and solved(v, "spread"))
    cov["many: a spread member without a many-problem kernel, alone"] = where(lambda n, s, w, v: w == "many" and n == "spread-pod-notin" and s in no_many_kernel and solved(v, "spread"))
    cov["many: a spread hand-back that keeps tw.enabled (27)"] = where(lambda n, s, w, v: w == "many" and v["engine"] == "general" and v["engineFallbackReason"] == 27 and v["cursorAttempts"] == 0)
    cov["many: a spread hand-back that clears tw.enabled"] = where(lambda n, s, w, v: w == "many" and n in ("filter-never", "spread-pod-notin") and v["engine"] == "general" and v["engineFallbackReason"] in (4, 43))
    cov["many: spread-only, refused by the engine"] = where(lambda n, s, w, v: w == "many" and spread_only(s) and MESSAGES["spread declined"] in v["error"])
    cov["many: spread-only, refused by the host"] = where(lambda n, s, w, v: w == "many" and spread_only(s) and MESSAGES["spread outside shape"] in v["error"])
    # SolveMany, the cursor engine. Every cursor handle of a late setting that SolveMany does not refuse has the limit stages (create():
    # fw.lim under eng.limits) and so runs alone; the batched kernel under SolveMany is in the record of settings 0-17
    # (tests/test_solve_many.py). Here it runs for the batch, which leaves the attempts at 0: that is how a cell shows it.
    cov["a cursor member on the batched kernel"] = where(lambda n, s, w, v: w == "batch" and solved(v, "cursor") and v["cursorAttempts"] == 0)
    cov["many: a cursor member alone, the set-aside list"] = where(lambda n, s, w, v: w == "many" and n == "pinned" and solved(v, "cursor"))
    cov["many: a cursor member alone, pod operators"] = where(lambda n, s, w, v: w == "many" and n == "zone-notin" and solved(v, "cursor"))
    cov["many: a cursor member alone, the node stage"] = where(lambda n, s, w, v: w == "many" and n == "dedicated-nodes" and solved(v, "cursor"))
    # SolveBatch: a spread handle alone by each of its four conditions — under "auto-operators-spread" (no set-aside list) "spread-mix"
    # meets none and runs the general engine with reason 0; the three problems beside it meet one each
    plain_mix = where(lambda n, s, w, v: w == "batch" and n == "spread-mix" and s == "auto-operators-spread" and v["engine"] == "general" and v["engineFallbackReason"] == 0)
    cov["batch: a spread-shaped handle on the general engine, reason 0"] = plain_mix
    for what, name in (("daemon_groups", "spread-mix-daemonsets"), ("nd.dom", "spread-mix-nodes"), ("spread_complement", "spread-complement")):
        cov[f"batch: a spread handle alone, {what}"] = plain_mix and where(lambda n, s, w, v: w == "batch" and n == name and s == "auto-operators-spread" and solved(v, "spread"))
    cov["batch: a spread handle alone, unsched"] = plain_mix and where(lambda n, s, w, v: w == "batch" and n == "spread-mix" and s == "auto-unschedulable-spread" and solved(v, "spread"))
    cov["batch: the short outside-shape text, spread-only handle"] = where(lambda n, s, w, v: w == "batch" and spread_only(s) and v["error"].endswith(MESSAGES["batch outside shape"]))
    return cov


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", choices=["emulation", "device"])
    ap.add_argument("--coverage", action="store_true")
    ap.add_argument("--late", action="store_true", help="the record of LATE_SETTINGS (tests/golden/engine_matrix_late.json)")
    ap.add_argument("--out")
    args = ap.parse_args()
    args.out = args.out or (LATE_FIXTURE if args.late else FIXTURE)
    if args.coverage:
        for claim, found in (late_coverage(load("emulation", LATE_FIXTURE)) if args.late else coverage(load("emulation"))).items():
            print(f"{len(found):4d}  {claim}" + (f"   e.g. {found[0]}" if found else "   MISSING"))
        return
    if not args.record:
        ap.error("--record or --coverage")
    import parity
    cells = (build_late if args.late else build_matrix)(parity.build_emu() if args.record == "emulation" else None, progress=True)
    doc = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            doc = json.load(f)
    if args.record == "emulation":
        doc["emulation"] = cells
    else:
        base = doc.get("emulation", {})
        doc["device"] = {k: v for k, v in cells.items() if base.get(k) != v}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"engine_matrix: recorded {len(cells)} cells under '{args.record}' in {args.out}" + (f" ({len(doc['device'])} differ from the emulation)" if args.record == "device" else ""))


if __name__ == "__main__":
    main()
