"""Problems with topology groups whose NodePool limits BIND, for the spread engine's limit stages (csrc/topo_engine.h
TopoEngine::limit_stage over csrc/fast_engine.h limit_stage_id, engines "auto-limits-spread" / "spread-limits";
tests/test_spread_engine_limits.py on the emulation, tests/test_gpu_spread_limits.py on the device): the benchmark mix over a
limited and an open pool, known small shapes, the seeded fuzz and the comparison helper.

What the reference does when a limit binds (scheduler.go:706-727) stands in tests/limit_cases.py, whose problems are the cursor
engine's; the ones here carry at least one topology constraint, so engines 0-12 end on the general engine with reason 23 / 24."""
import copy

import engine_checks as ec
import limit_cases as lc
import mix_cases
import parity
from karpenter_amd import fixtures as fx
from karpenter_amd.scheduling import NewScheduler

stages, pool_of = lc.stages, lc.pool_of
# 13, 14 over "auto" ("auto-nodes-spread" with existing nodes): what engines 0-12 do is to stop with reason 23 / 24. No engine-only
# leg below the switch. declined(): plain "auto" stops earlier, at the limit.
SWITCH = ec.Switch("spread", only="spread-limits", auto="auto-limits-spread", base="auto", reasons=(23, 24), base_first=True)
check_declined = SWITCH.declined


def check_engine(oracle, lib, prob, base="auto"):
    """The limit binds in this problem: SWITCH.check under `base`."""
    return SWITCH.check(oracle, lib, prob, base=base)


# ---- 1, 2, 6: the benchmark mix over two pools --------------------------------------------------------------------------------------

def mix_problem(cfg, limits):
    """fixtures.config3(*cfg) with its single pool doubled: a copy named "limited" with weight 10 and the given limits, tried first,
    and a copy named "open"."""
    pods, n_types, seed = cfg
    prob = fx.config3(pods=pods, n_types=n_types, seed=seed)
    (pool,) = prob["nodePools"]
    limited, open_ = copy.deepcopy(pool), copy.deepcopy(pool)
    limited.update(name="limited", weight=10)
    if limits is not None:   # (None: the two pools without a limit, for tools that size one)
        limited["limits"] = dict(limits)
    open_.update(name="open")
    return dict(prob, nodePools=[limited, open_])


# (cfg, limits, the oracle's claims in "limited", in "open")
MIX = [((300, 144, 1), {"cpu": "100"}, 2, 58),
       ((1500, 144, 5), {"cpu": "600"}, 5, 295)]


def mix_nodes_problem():
    """Case 6: the first problem of MIX with five existing nodes and DaemonSets "c" — the kernel with the node path."""
    return fx.with_daemonsets(fx.with_existing_nodes(mix_problem(*MIX[0][:2]), 5, seed=3), "c")


# ---- 3: a zonal chain ---------------------------------------------------------------------------------------------------------------

def zonal_chain_problem():
    """limit_cases.cpu_chain_problem(True) with zonal spread on every pod: thirty 3-cpu pods of one label, the 1..8-cpu catalogue,
    "first" (weight 10, cpu 40) takes five claims of 8 cpu (40 -> 32 -> ... -> 0), the first exclusion — of every type — comes with
    five claims open, "second" takes the rest."""
    lab = {"app": "chain"}
    pools = [fx.node_pool("first", weight=10, limits={"cpu": "40"}), fx.node_pool("second")]
    pods = [fx.pod(labels=lab, requests={"cpu": "3"}, topology_spread=[fx.spread(fx.ZONE, lab)]) for _ in range(30)]
    return fx.problem(fx.fake_instance_types(8), pools, pods)


# ---- 4: a claim of an early stage accepts after a later stage exists ---------------------------------------------------------------

def early_stage_problem():
    """limit_cases.early_stage_problem with topology constraints: twelve 3-cpu pods with zonal + hostname (max_skew 2) spread, then
    (queue order: larger requests first) twenty 1-cpu pods with zonal spread; "first" has cpu 36. Claims of the full list, then of
    the narrowed one, then of "second"; the 1-cpu pods fill the room the early claims have left."""
    big, small = {"app": "big"}, {"app": "small"}
    pools = [fx.node_pool("first", weight=10, limits={"cpu": "36"}), fx.node_pool("second")]
    pods = [fx.pod(labels=big, requests={"cpu": "3"}, topology_spread=[fx.spread(fx.ZONE, big), fx.spread(fx.HOSTNAME, big, max_skew=2)]) for _ in range(12)]
    pods += [fx.pod(labels=small, requests={"cpu": "1"}, topology_spread=[fx.spread(fx.ZONE, small)]) for _ in range(20)]
    return fx.problem(fx.fake_instance_types(8), pools, pods)


def early_claim_holds_a_small_pod(prob, res):
    """Read off a result: some claim of "first" that still lists the 8-cpu type — opened under the full list, lists only narrow —
    holds a 1-cpu pod, and some claim of "first" lists no type above 4 cpu. Every 3-cpu pod is popped before every 1-cpu pod and
    only 3-cpu pods open claims of "first" under the full list, so the early claim took the 1-cpu pod after the narrower stage
    existed."""
    cpus = lc.cpu_of(prob)
    size = {p["uid"]: p["requests"]["cpu"] for p in prob["pods"]}
    first = [c for c in res["newNodeClaims"] if c["nodePool"] == "first"]
    early = [c for c in first if lc.max_cpu(c, cpus) == 8 and any(size[u] == "1" for u in c["pods"])]
    narrow = [c for c in first if lc.max_cpu(c, cpus) <= 4]
    return bool(early) and bool(narrow)


# ---- 5: more limit stages than template ids ---------------------------------------------------------------------------------------

def stage_chain_problem(n_limited):
    """limit_cases.stage_chain_problem with zonal spread on every pod: `n_limited` weighted pools of cpu 127 over the power
    catalogue (three pods to a claim) and a catch-all pool. A pool's remaining cpu goes 127 -> 63 -> 31 -> 15 -> 7 -> 3 -> 1 -> 0:
    its list narrows seven times, one stage each; three pools need 21 of the 28 free ids, four pools 28 of 27 (reason 29)."""
    lab = {"app": "chain"}
    pools = [fx.node_pool(f"pool-{i}", weight=50 - 10 * i, limits={"cpu": "127"}) for i in range(n_limited)] + [fx.node_pool("catch-all")]
    pods = [fx.pod(labels=lab, requests={"cpu": "100m", "memory": "64Mi"}, topology_spread=[fx.spread(fx.ZONE, lab)]) for _ in range(3 * 7 * n_limited + 12)]
    return fx.problem(lc.power_catalogue(), pools, pods)


# ---- 7: repeated solves -------------------------------------------------------------------------------------------------------------

def repeated_solves(lib, prob, engine, n):
    """n solves on one handle -> (the set of digests, the set of stage words, the last result); every solve on the spread engine."""
    s = NewScheduler(dict(prob, options=dict(prob.get("options", {}), engine=engine)), solver_lib=lib)
    try:
        digests, words = set(), set()
        for _ in range(n):
            r = s.Solve()
            assert r["counters"]["engine"] == "spread" and r["counters"]["engineFallbackReason"] == 0, r["counters"]
            digests.add(parity.results_digest(r)[0])
            words.add(stages(r))
        return digests, words, r
    finally:
        s.close()


# ---- 8: seeded fuzz -----------------------------------------------------------------------------------------------------------------

FUZZ_SEEDS = [s for s in range(96) if s % 5 == 2]     # mix_cases.fuzz_problem: pools "few" (cpu 20, weight 5) + "rest"
FUZZ_ON_SPREAD = [2, 12, 17, 22, 32, 37, 42, 52, 57, 62, 67, 72, 77, 82, 92]   # no pod errors in the oracle; engines 0-12 stop with 24
FUZZ_UNSCHEDULABLE = [27]                              # the oracle leaves one pod unschedulable: reason 27 under every setting
FUZZ_NODE_FILTER = [7, 47, 87]                         # a pod with a nodeSelector AND a spread constraint: reason 43, as before
assert sorted(FUZZ_ON_SPREAD + FUZZ_UNSCHEDULABLE + FUZZ_NODE_FILTER) == FUZZ_SEEDS


def run_fuzz(oracle, lib, seeds):
    """Whatever "auto-limits-spread" runs equals the oracle; a seed of FUZZ_ON_SPREAD runs on the spread engine with reason 0 (and
    stops with 24 under "auto"), seed 27 ends with reason 27 and has pod errors in the oracle, seeds 7 / 47 / 87 end with 43.
    Returns the limit stages created, summed over the seeds."""
    made = 0
    for seed, prob, want, got, on, reason in ec.fuzz_cases(oracle, lib, ((seed, mix_cases.fuzz_problem(seed)) for seed in seeds), SWITCH.auto, pops=False):
        if seed in FUZZ_ON_SPREAD:
            assert not want["podErrors"] and (on, reason) == ("spread", 0), (seed, got["counters"])
            assert ec.solve(prob, "auto", lib)["counters"]["engineFallbackReason"] == 24, seed
            made += stages(got)[0]
        elif seed in FUZZ_UNSCHEDULABLE:
            assert len(want["podErrors"]) == 1 and (on, reason) == ("general", 27), (seed, got["counters"])
        else:
            assert seed in FUZZ_NODE_FILTER and (on, reason) == ("general", 43), (seed, got["counters"])
    return made
