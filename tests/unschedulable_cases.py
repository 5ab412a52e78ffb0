"""Problems that leave pods UNSCHEDULABLE, for the cursor engine's set-aside list (csrc/fast_engine.h, "Unschedulable pods"; engines
"auto-unschedulable" / "cursor-unschedulable"; tests/test_cursor_engine_unschedulable.py on the emulation,
tests/test_gpu_cursor_unschedulable.py on the device): known shapes, the comparison helper and the fuzz runner.

What the reference does with such a pod (scheduler.go:440-519, queue.go:31-108): its error is the FIRST template's, in template
order — Limits (7) for a template skipped before NewNodeClaim, else CanAdd's first failing check: Taints (1), Incompatible (2),
InstanceTypes (4, with the filter's flags: requirementsMet 1, fits 2, hasOffering 4, requirements + offering without fit 16, fit +
offering without requirements 32), NoTemplates (6) when no template survived the prefilter. The pod goes to the back of the queue with
lastLen = the queue's length after the push, is popped again behind everything that stood in front of it, and the loop stops at the
first pop whose lastLen equals the queue's length — so `pops` = pods + failed pods - the run of failed pods at the queue's tail (at
least pods), and a pod's reported error is that of its last attempt."""
import os
import sys
from collections import Counter

import engine_checks as ec
import limit_cases as lc
import operator_cases as oc
from karpenter_amd import fixtures as fx

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import engine_matrix  # noqa: E402

# 20, 21 over 18 / 16 (every switch but the one under test): what every setting up to 19 does is to decline with reason 27. The
# oracle leaves pods unschedulable; queue pops are compared.
SWITCH = ec.Switch("cursor", only="cursor-unschedulable", auto="auto-unschedulable", base="auto-operators-spread", base_only="cursor-operators",
                   reasons=(27,), errors=True, pops=True)
BASE = SWITCH.base
ABSENT = "test-zone-9"


def n_pods(prob):
    return len(prob.get("pods", [])) + sum(g["count"] for g in prob.get("podGroups", []))


def errors_of(res):
    """{(code, diag): pods} of a Results document."""
    return dict(Counter((e["code"], e["diag"]) for e in res["podErrors"].values()))


def check_engine(oracle, lib, prob, base=BASE):
    """One problem five ways (SWITCH.check), in claims and their order, hostnames, pod errors with their flags, the
    reference-equivalent evaluation count and queue pops."""
    return SWITCH.check(oracle, lib, prob, base=base)


def check_declined(oracle, lib, prob, reason):
    """SWITCH.declined (reason 0: the batch is not offered to a fast engine at all) for a problem that leaves pods unschedulable."""
    auto = SWITCH.declined(oracle, lib, prob, reason)
    assert auto["podErrors"]   # (the oracle's: declined() held the two equal)
    return auto


# ---- 1-3: one plain batch, pods that fit nowhere --------------------------------------------------------------------------------------

def big_pod():
    """10,000 cpu: the first pod of any queue (queue.go:72-108: larger requests first). Every type meets its requirements and has an
    offering, none holds it: InstanceTypes with requirementsMet | hasOffering | their pair = 21."""
    return fx.pod(requests={"cpu": "10000"})


def absent_zone_pod(cpu="1m"):
    """Selects a zone no type offers; 1m cpu and no memory: the last pod of the queue. No flag is set: 0."""
    return fx.pod(requests={"cpu": cpu}, node_selector={fx.ZONE: ABSENT})


def plain_batch(n_big, n_absent, pods=24):
    """fx.config1 at `pods` pods (pod groups) plus n_big pods no type holds and n_absent pods selecting an absent zone."""
    prob = fx.config1(pods=pods)
    return dict(prob, pods=list(prob.get("pods", [])) + [big_pod() for _ in range(n_big)] + [absent_zone_pod() for _ in range(n_absent)])


# ---- 4-6: which template's error ------------------------------------------------------------------------------------------------------

def pinned_pool():
    return fx.node_pool("zone-1", requirements=[fx.req(fx.ZONE, "In", "test-zone-1")])


def pinned_pods():
    return [fx.pod(requests={"cpu": "1"}) for _ in range(8)] + [fx.pod(requests={"cpu": "500m"}, node_selector={fx.ZONE: "test-zone-2"}) for _ in range(2)]


def pinned_problem():
    """A pool pinned to test-zone-1 and pods selecting test-zone-2: Requirements.Compatible fails, Incompatible (2)."""
    return fx.problem(fx.fake_instance_types(8), [pinned_pool()], pinned_pods())


def tainted_first_problem():
    """A heavier tainted pool in front of case 4's: the pods tolerate nothing, so the FIRST template's error is Taints (1) — for the
    zone-2 pods, whose second template says Incompatible, and for a 100-cpu pod, whose second template says InstanceTypes."""
    pools = [fx.node_pool("tainted", weight=10, taints=oc.taint("tainted")), pinned_pool()]
    return fx.problem(fx.fake_instance_types(8), pools, pinned_pods() + [fx.pod(requests={"cpu": "100"})])


def no_template_problem():
    """The only pool asks for a zone no type offers: NewScheduler's prefilter leaves no template, every pod gets NoTemplates (6) and
    the first pop of the second round ends the loop."""
    pools = [fx.node_pool("nowhere", requirements=[fx.req(fx.ZONE, "In", ABSENT)])]
    return fx.problem(fx.fake_instance_types(8), pools, [fx.pod(requests={"cpu": c}) for c in ["2", "1", "500m"] * 4])


def inactive_first_problem():
    """Case 6's pool (weight 10: no template survives for it) in front of an open pool: the FIRST surviving template is the second
    one, and the flags of the 100-cpu pod's InstanceTypes error are that template's (21; the first template's list is empty: 0)."""
    pools = [fx.node_pool("nowhere", weight=10, requirements=[fx.req(fx.ZONE, "In", ABSENT)]), fx.node_pool("open")]
    pods = [fx.pod(requests={"cpu": "100"})] + [fx.pod(requests={"cpu": c}) for c in ["2", "1", "500m"] * 3] + [absent_zone_pod()]
    return fx.problem(fx.fake_instance_types(8), pools, pods)


def sort_at_retry_problem():
    """A failing attempt sorts the claims (scheduler.go:598) before it scans them. Queue: a 100-cpu pod (fails), four 3-cpu pods
    (two claims of two pods on the 1..8-cpu catalogue), one 1-cpu pod, which joins the claim at the front of the order: three pods against two, so the
    next sort moves that claim behind the other. No pod follows; the sort that moves it is the one of the first pod's second attempt."""
    pods = [fx.pod(requests={"cpu": "100"})] + [fx.pod(requests={"cpu": "3"}) for _ in range(4)] + [fx.pod(requests={"cpu": "1"})]
    return fx.problem(fx.fake_instance_types(8), [fx.node_pool()], pods)


# ---- 8: failing pods inside the queue and at its tail ---------------------------------------------------------------------------------

def tail_run_problem():
    """Eleven pods in queue order: four of 2 cpu, one of 1 cpu and 100,000Gi (21, in the MIDDLE of the queue: cpu sorts first), three
    of 500m, three of 1m that select an absent zone (0, the queue's tail). Four pods fail, three of them at the tail: twelve pops."""
    pods = [fx.pod(requests={"cpu": "2"}) for _ in range(4)] + [fx.pod(requests={"cpu": "1", "memory": "100000Gi"})]
    pods += [fx.pod(requests={"cpu": "500m"}) for _ in range(3)] + [absent_zone_pod() for _ in range(3)]
    return fx.problem(fx.fake_instance_types(8), [fx.node_pool()], pods)


# ---- 9: an error that changes at the retry --------------------------------------------------------------------------------------------

def error_changes_problem():
    """limits.cpu = 16 on the only pool of the 1..8-cpu catalogue. The queue's first pod (100 cpu) fails with InstanceTypes; the 3-cpu
    pods open two claims of two pods each (16 -> 8 -> 0) and the other four find the template skipped: Limits (7). The first pod comes back behind them —
    pods that followed it were placed — and its second attempt finds the template skipped too: its error is 7 now, not 4."""
    pods = [fx.pod(requests={"cpu": "100"})] + [fx.pod(requests={"cpu": "3"}) for _ in range(8)]
    return fx.problem(fx.fake_instance_types(8), [fx.node_pool(limits={"cpu": "16"})], pods)


# ---- 10-12: limit stages, DaemonSet overhead, a complement template -------------------------------------------------------------------

def stage_chain_alone():
    """lc.stage_chain_problem(3) without its catch-all pool: three pools whose lists narrow seven times each, then nothing."""
    prob = lc.stage_chain_problem(3)
    return dict(prob, nodePools=[p for p in prob["nodePools"] if p["name"] != "catch-all"])


def daemonset_problem():
    """7800m pods fit the 8-cpu type alone but not beside the 500m DaemonSet: the overhead alone makes them unschedulable."""
    ds = [fx.pod(requests={"cpu": "500m", "memory": "100Mi"})]
    pods = [fx.pod(requests={"cpu": "7800m"}) for _ in range(3)] + [fx.pod(requests={"cpu": "1"}) for _ in range(9)]
    return fx.problem(fx.fake_instance_types(8), [fx.node_pool()], pods, daemonset_pods=ds)


def complement_problem():
    """oc.notin_problem() without its open pool: the pods pinned to test-zone-1 meet the pool's NotIn [test-zone-1]."""
    return fx.problem(fx.fake_instance_types(8), [oc.notin_zone_pool()], oc.notin_zone_pods())


# ---- 13, 14: four rows of class slots; the next memory plan ----------------------------------------------------------------------------

def many_classes_problem():
    """lc.many_classes_problem() (1,490 pods, more than 64 classes live at once: the kernels with four rows of class slots) plus
    failing pods of three kinds: at the head of the queue, inside it (2 cpu like every other pod, an absent zone) and at its tail."""
    prob = lc.many_classes_problem()
    extra = [fx.pod(requests={"cpu": "10000"})] + [fx.pod(requests={"cpu": "2", "memory": "1Gi"}, node_selector={fx.ZONE: ABSENT}) for _ in range(5)] + [absent_zone_pod()]
    return dict(prob, pods=prob["pods"] + extra)


def escalation_problem():
    """3,600 claims: more than the LDS plan holds, so the solve either starts on plan 1 or gets there by reason 26 — a second run of the
    kernel, whose setup() starts from an empty set-aside list — plus a failing pod at each end of the queue."""
    prob = engine_matrix._without_limits(lc.escalation_problem(3600))
    return dict(prob, pods=prob["pods"] + [big_pod(), absent_zone_pod()])


def hand_problems(with_escalation=True):
    """(name, problem, what the oracle must report or None): every known shape. The expectations are facts about the reference, read
    off the oracle when the cases were written."""
    nodes = fx.with_existing_nodes(tail_run_problem(), 4, seed=1)
    out = [("big-first", plain_batch(1, 0), dict(errors={(4, 21): 1}, extra_pops=1)),
           ("absent-last", plain_batch(1, 1), dict(errors={(4, 21): 1, (4, 0): 1}, extra_pops=1)),
           ("absent-last-alone", plain_batch(0, 1), dict(errors={(4, 0): 1}, extra_pops=0)),
           ("two-big", plain_batch(2, 1), dict(errors={(4, 21): 2, (4, 0): 1}, extra_pops=2)),
           ("pinned", pinned_problem(), dict(errors={(2, 0): 2}, extra_pops=0)),
           ("tainted-first", tainted_first_problem(), dict(errors={(1, 0): 3})),
           ("no-template", no_template_problem(), dict(errors={(6, 0): 12}, extra_pops=0)),
           ("inactive-first", inactive_first_problem(), dict(errors={(4, 21): 1, (4, 0): 1}, extra_pops=1)),
           ("sort-at-retry", sort_at_retry_problem(), dict(errors={(4, 21): 1}, claims=2, extra_pops=1)),
           ("cpu-chain", lc.cpu_chain_problem(False), dict(errors={(7, 0): 20}, claims=5, extra_pops=0)),
           ("tail-run", tail_run_problem(), dict(errors={(4, 0): 3, (4, 21): 1}, extra_pops=1)),
           ("tail-run-nodes", nodes, None),
           ("error-changes", error_changes_problem(), dict(errors={(7, 0): 5}, claims=2, extra_pops=1)),
           ("stage-chain", stage_chain_alone(), None),
           ("daemonset", daemonset_problem(), None),
           ("complement", complement_problem(), None),
           ("many-classes", many_classes_problem(), None)]
    if with_escalation:
        out.append(("escalation", escalation_problem(), None))
    return out


def check_expectation(prob, want, expect):
    if not expect:
        return
    assert errors_of(want) == expect["errors"], errors_of(want)
    if "claims" in expect:
        assert len(want["newNodeClaims"]) == expect["claims"]
    if "extra_pops" in expect:
        assert want["counters"]["pops"] == n_pods(prob) + expect["extra_pops"], (want["counters"]["pops"], n_pods(prob))


# ---- still declined --------------------------------------------------------------------------------------------------------------------

def spread_problem():
    """A zonal spread plus a pod that fits nowhere: the spread engine still declines with 27 (there a retry CAN succeed: domain counts move)."""
    pods = [fx.pod(requests={"cpu": "1"}, labels={"app": "web"}, topology_spread=[fx.spread(fx.ZONE, {"app": "web"})]) for _ in range(12)]
    return fx.problem(fx.fake_instance_types(8), [fx.node_pool()], pods + [fx.pod(requests={"cpu": "100"})])


def preference_problem():
    """A failing pod with a node-affinity preference: the reference's push-back relaxes it (preferences.go:38-57), a relaxation row."""
    prob = tail_run_problem()
    pref = fx.pod(requests={"cpu": "100"}, node_preferences=[fx.req(fx.ZONE, "In", "test-zone-1")])
    return dict(prob, pods=prob["pods"] + [pref])


def pod_operator_problems():
    """(name, problem, reason): the tail-run batch plus one pod whose own requirement is not an In set — NotIn makes its class "not
    positive" (4), Gt / Lt are bounds, which the host finds (1) — and the batch under a NodePool with minValues (1; minValues is a
    NodePool field: pods cannot carry it)."""
    prob = tail_run_problem()
    reqs = [("notin", fx.req(fx.ZONE, "NotIn", "test-zone-3"), 4), ("gt", fx.req(fx.FAKE_INTEGER_LABEL, "Gt", 4), 1), ("lt", fx.req(fx.FAKE_INTEGER_LABEL, "Lt", 3), 1)]
    out = [(name, dict(prob, pods=prob["pods"] + [fx.pod(requests={"cpu": "1"}, node_requirements=[r])]), reason) for name, r, reason in reqs]
    pool = fx.node_pool(requirements=[fx.req(fx.INSTANCE_TYPE, "Exists", min_values=2)])
    return out + [("min-values", dict(prob, nodePools=[pool]), 1)]


# ---- fuzz ------------------------------------------------------------------------------------------------------------------------------

FUZZ_SEEDS = list(range(48))
GPU_FUZZ_SEEDS = list(range(0, 48, 4))


def run_fuzz(oracle, lib, seeds):
    """lc.fuzz_problem(seed) — a cpu limit on EVERY pool, existing nodes one time in two, DaemonSets two times in three — under
    "auto-unschedulable": every seed equals the oracle, pops included; a seed that leaves the cursor engine does so with 29 or a shape
    reason, never 27. Returns (seeds with pod errors in the oracle, seeds that stayed on the cursor engine, {seed: reason} of the rest)."""
    with_errors, on_cursor, rest = 0, 0, {}
    for seed, _, want, got, on, r in ec.fuzz_cases(oracle, lib, ((seed, lc.fuzz_problem(seed)) for seed in seeds), SWITCH.auto, pops=True, mode=SWITCH.mode):
        with_errors += bool(want["podErrors"])
        if on == "cursor":
            on_cursor += 1
        else:
            assert r != 27 and (r == 29 or r in lc.SHAPE_REASONS), (seed, got["counters"])
            rest[seed] = r
    print(f"auto-unschedulable kept {on_cursor} of {len(seeds)} seeds on the cursor engine ({with_errors} with pod errors in the oracle); reasons of the rest {rest}")
    return with_errors, on_cursor, rest
