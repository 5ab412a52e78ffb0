"""Problems whose PODS carry requirements that are not In sets — NotIn, Exists, DoesNotExist — for the cursor engine's pod operators
(csrc/fast_engine.h, "The cursor engine's pod operators"; engines "auto-pod-operators" / "cursor-pod-operators";
tests/test_cursor_engine_pod_operators.py on the emulation, tests/test_gpu_cursor_pod_operators.py on the device): known shapes, the
seeded fuzz generator and the comparison helpers.

What the reference does with such a pod (requirements.go:181-197, 254-274; requirement.go:181-254): a NotIn / DoesNotExist requirement
may name a key the NodeClaim does not define; against a concrete In set it needs a common value and leaves a concrete set; against a
complement set (NotIn, Exists, Gt, Lt) a NotIn always intersects and grows the excluded values; two sides that are both NotIn /
DoesNotExist pass without an intersection (:260-265), and what is left is DoesNotExist when one of them is."""
import random

import engine_checks as ec
import operator_cases as oc
from karpenter_amd import fixtures as fx

claims_of, req_of = oc.claims_of, oc.req_of
ZONES = oc.ZONES
K = "example.com/k"
# 26, 27 over 24 / 21 (every switch but the one under test): what every setting up to 25 does is to decline with the reason given per
# call — 4 for NotIn / Exists pods, 8 for DoesNotExist. The oracle's result has no pod errors.
SWITCH = ec.Switch("cursor", only="cursor-pod-operators", auto="auto-pod-operators", base="auto-filters-spread", base_only="cursor-unschedulable", errors=False)
ENGINE, AUTO, BASE, BASE_CURSOR = SWITCH.only, SWITCH.auto, SWITCH.base, SWITCH.base_only
# ... and for a problem that leaves pods unschedulable: pod errors required, queue pops compared, no engine-only leg below the switch
UNSCHEDULABLE = SWITCH._replace(errors=True, pops=True, base_only=None)
check_declined = SWITCH.declined


def check_engine(oracle, lib, prob, reason=4):
    """One problem five ways (SWITCH.check): the claims' requirements are compared by operator, values and bounds (parity.canon_req)."""
    return SWITCH.check(oracle, lib, prob, reason=reason)


def check_unschedulable(oracle, lib, prob, reason=4):
    """A problem that leaves pods unschedulable: 24 falls back with `reason`, 26 / 27 end on the cursor engine and equal the oracle in
    claims, pod errors with their flags, evaluation count and queue pops."""
    return UNSCHEDULABLE.check(oracle, lib, prob, reason=reason)


def kinds(res, key, pool=None):
    """{(operator, values)} of the claims' requirement on `key` (None for a claim without one)."""
    return {req_of(c, key) and (req_of(c, key)[0], tuple(req_of(c, key)[1])) for c in res["newNodeClaims"] if pool is None or c["nodePool"] == pool}


def pod_reqs(pod):
    """The requirements of the pod's (one) required node-affinity term."""
    return list((pod.get("nodeAffinity") or {}).get("required", [[]])[0])


def notin(key, *values):
    return [fx.req(key, "NotIn", *values)]


# ---- 1: zone NotIn over an open pool ----------------------------------------------------------------------------------------------

def zone_notin_problem():
    """Queue order is by size. Three 7-cpu pods with zone NotIn [test-zone-1]: a claim each, nothing fits beside them — NotIn
    [test-zone-1]. Two 5-cpu pods with the same requirement; two 4-cpu pods with it; two 3-cpu pods that admit test-zone-2 and
    test-zone-3 join the 4-cpu claims, which become the concrete In [test-zone-2, test-zone-3]; two 2-cpu pods with zone NotIn
    [test-zone-2] join the 5-cpu claims, which print the union NotIn [test-zone-1, test-zone-2]."""
    pods = [fx.pod(requests={"cpu": c}, node_requirements=notin(fx.ZONE, "test-zone-1")) for c in ["7"] * 3 + ["5"] * 2 + ["4"] * 2]
    pods += [fx.pod(requests={"cpu": "3"}, node_requirements=[fx.req(fx.ZONE, "In", "test-zone-2", "test-zone-3")]) for _ in range(2)]
    pods += [fx.pod(requests={"cpu": "2"}, node_requirements=notin(fx.ZONE, "test-zone-2")) for _ in range(2)]
    return fx.problem(fx.fake_instance_types(8), [fx.node_pool("open")], pods)


ZONE_NOTIN_KINDS = {("NotIn", ("test-zone-1",)), ("NotIn", ("test-zone-1", "test-zone-2")), ("In", ("test-zone-2", "test-zone-3"))}


# ---- 2: capacity-type NotIn [spot] over a pool with In [spot, on-demand] --------------------------------------------------------------

def capacity_type_problem():
    pools = [fx.node_pool("both", weight=10, requirements=[fx.req(fx.CAPACITY_TYPE, "In", "spot", "on-demand")]), fx.node_pool("open")]
    pods = [fx.pod(requests={"cpu": c}, node_requirements=notin(fx.CAPACITY_TYPE, "spot")) for c in ["3", "1", "500m"] * 4]
    pods += [fx.pod(requests={"cpu": "7500m"}) for _ in range(2)]   # (a claim each, nothing fits beside them: the pool's own In [on-demand, spot])
    return fx.problem(fx.fake_instance_types(8), pools, pods)


# ---- 3: complement meets complement, the dictionary exhausted --------------------------------------------------------------------------

def exhausted_problem():
    """example.com/k (well-known here, so that a pod's In may name it on the open pool) has the values a and b alone. Pool `not-a`: k
    NotIn [a]. Four 3-cpu pods with k NotIn [b] are accepted — two complements always intersect — and leave NotIn [a, b]: no dictionary
    value. The 1-cpu pods with k In [a] are refused by those claims and by the pool, and open claims of the open pool."""
    pools = [fx.node_pool("not-a", weight=10, requirements=[fx.req(K, "NotIn", "a")]), fx.node_pool("open")]
    pods = [fx.pod(requests={"cpu": "3"}, node_requirements=notin(K, "b")) for _ in range(4)]
    pods += [fx.pod(requests={"cpu": "1"}, node_requirements=[fx.req(K, "In", "a")]) for _ in range(3)]
    return fx.problem(fx.fake_instance_types(8), pools, pods, well_known=fx.FAKE_WELL_KNOWN + [K])


# ---- 4: special DoesNotExist -------------------------------------------------------------------------------------------------------

def dne_problem():
    """Pool `with` (weight 30): special Exists — refuses a DoesNotExist pod. Pool `without` (weight 20, tainted): special DoesNotExist
    — takes those that tolerate it. Pool `open`: the claim prints DoesNotExist and loses the large types (special In [optional])."""
    pools = [fx.node_pool("with", weight=30, requirements=[fx.req(fx.FAKE_EXOTIC_LABEL, "Exists")]),
             fx.node_pool("without", weight=20, requirements=[fx.req(fx.FAKE_EXOTIC_LABEL, "DoesNotExist")], taints=oc.taint("without")), fx.node_pool("open")]
    dne = [fx.req(fx.FAKE_EXOTIC_LABEL, "DoesNotExist")]
    pods = [fx.pod(requests={"cpu": c}, node_requirements=dne) for c in ["2", "1", "500m"] * 3]
    pods += [fx.pod(requests={"cpu": c}, node_requirements=dne, tolerations=oc.tolerate("without")) for c in ["1500m", "700m"] * 3]
    pods += [fx.pod(requests={"cpu": "1"}) for _ in range(4)]
    return fx.problem(fx.fake_instance_types(8), pools, pods)


def static_verdict_problem():
    """What the packed word cannot tell, on a custom key no instance type defines (so no type list can hide a wrong verdict). Pool
    `exists-first` (weight 40, tainted): k Exists; pool `absent` (weight 30): k DoesNotExist; pool `exists` (weight 20): k Exists. Pods with
    k DoesNotExist that tolerate the taint are refused by `exists-first` and land on `absent`; pods with k Exists are refused by `absent`
    and land on `exists`; pods without a requirement land on `absent`."""
    pools = [fx.node_pool("exists-first", weight=40, requirements=[fx.req(K, "Exists")], taints=oc.taint("exists-first")),
             fx.node_pool("absent", weight=30, requirements=[fx.req(K, "DoesNotExist")]), fx.node_pool("exists", weight=20, requirements=[fx.req(K, "Exists")])]
    pods = [fx.pod(requests={"cpu": c}, node_requirements=[fx.req(K, "DoesNotExist")], tolerations=oc.tolerate("exists-first")) for c in ["2", "1"] * 3]
    pods += [fx.pod(requests={"cpu": c}, node_requirements=[fx.req(K, "Exists")]) for c in ["1500m", "700m"] * 3]
    pods += [fx.pod(requests={"cpu": "500m"}) for _ in range(4)]
    return fx.problem(fx.fake_instance_types(8), pools, pods)


# ---- 5: integer NotIn ------------------------------------------------------------------------------------------------------------

def integer_problem():
    """Open pool. Two 5500m pods with integer NotIn [7, 8]: of the three types that hold them (6, 7 and 8 cpu) their claims lose exactly
    the 7- and the 8-cpu type. One 3-cpu pod with integer NotIn [8] — complement —, then a
    2-cpu pod with integer In [2, 4, 6, 8] joins it — the concrete In [2, 4, 6] —, then a 500m pod with integer In [4, 6] — In [4, 6], of
    which only the 6-cpu type holds the three."""
    pods = [fx.pod(requests={"cpu": "5500m"}, node_requirements=notin(fx.FAKE_INTEGER_LABEL, 7, 8)) for _ in range(2)]
    pods += [fx.pod(requests={"cpu": "3"}, node_requirements=notin(fx.FAKE_INTEGER_LABEL, 8))]
    pods += [fx.pod(requests={"cpu": "2"}, node_requirements=[fx.req(fx.FAKE_INTEGER_LABEL, "In", 2, 4, 6, 8)])]
    pods += [fx.pod(requests={"cpu": "500m"}, node_requirements=[fx.req(fx.FAKE_INTEGER_LABEL, "In", 4, 6)])]
    return fx.problem(fx.fake_instance_types(8), [fx.node_pool("open")], pods)


# ---- 6: a pod's Exists on a key every pool defines ----------------------------------------------------------------------------------

def exists_problem():
    """Pool `two` (weight 10): zone In [test-zone-1, test-zone-2]; pool `not-one`: zone NotIn [test-zone-1]. Pods with zone Exists
    leave either requirement as it stands; pods pinned to test-zone-3 go to `not-one`."""
    pools = [fx.node_pool("two", weight=10, requirements=[fx.req(fx.ZONE, "In", "test-zone-1", "test-zone-2")], taints=oc.taint("two")),
             fx.node_pool("not-one", requirements=[fx.req(fx.ZONE, "NotIn", "test-zone-1")])]
    ex = [fx.req(fx.ZONE, "Exists")]
    pods = [fx.pod(requests={"cpu": c}, node_requirements=ex, tolerations=oc.tolerate("two")) for c in ["3", "1"] * 3]
    pods += [fx.pod(requests={"cpu": c}, node_requirements=ex) for c in ["2500m", "1200m"] * 3]
    pods += [fx.pod(requests={"cpu": "1"}, node_selector={fx.ZONE: "test-zone-3"}) for _ in range(3)]
    return fx.problem(fx.fake_instance_types(8), pools, pods)


# ---- 7: with a limit stage -----------------------------------------------------------------------------------------------------------

def limit_problem():
    """oc.limit_problem's pool (zone NotIn [test-zone-1], limits.cpu = 36: the fifth claim opens under a limit stage) with pods that
    require zone NotIn [test-zone-2]: the staged claims print NotIn [test-zone-1, test-zone-2]."""
    pods = [fx.pod(requests={"cpu": "3"}, node_requirements=notin(fx.ZONE, "test-zone-2")) for _ in range(10)]
    pods += [fx.pod(requests={"cpu": "1"}, node_selector={fx.ZONE: "test-zone-2"}) for _ in range(4)] + [fx.pod(requests={"cpu": "1"}) for _ in range(8)]
    return fx.problem(fx.fake_instance_types(8), [oc.notin_zone_pool(limits={"cpu": "36"}), fx.node_pool("open")], pods)


# ---- 8: a pod that excludes every zone ---------------------------------------------------------------------------------------------

def no_zone_problem():
    prob = zone_notin_problem()
    prob["pods"] += [fx.pod(requests={"cpu": "1"}, node_requirements=notin(fx.ZONE, *ZONES)) for _ in range(2)]
    return prob


def incompatible_problem():
    """One pool: zone In [test-zone-1] and special Exists. Pods with zone NotIn [test-zone-1] (nothing is left of the pool's set) and
    pods with special DoesNotExist (the static verdict) are unschedulable with Incompatible (2); the 5-cpu pods are placed."""
    pool = fx.node_pool("pinned", requirements=[fx.req(fx.ZONE, "In", "test-zone-1"), fx.req(fx.FAKE_EXOTIC_LABEL, "Exists")])
    pods = [fx.pod(requests={"cpu": "5"}) for _ in range(3)] + [fx.pod(requests={"cpu": "1"}, node_requirements=notin(fx.ZONE, "test-zone-1")) for _ in range(2)]
    pods += [fx.pod(requests={"cpu": "500m"}, node_requirements=[fx.req(fx.FAKE_EXOTIC_LABEL, "DoesNotExist")]) for _ in range(2)]
    return fx.problem(fx.fake_instance_types(8), [pool], pods)


# ---- 9: what still declines ----------------------------------------------------------------------------------------------------------

def pod_gt_problem():
    prob = zone_notin_problem()
    prob["pods"].append(fx.pod(requests={"cpu": "1"}, node_requirements=[fx.req(fx.FAKE_INTEGER_LABEL, "Gt", 4)]))
    return prob


def nodes_problem():
    return fx.with_existing_nodes(zone_notin_problem(), 4, seed=3, small=True)


def spread_problem():
    prob = oc.spread_problem()
    prob["pods"].append(fx.pod(requests={"cpu": "1"}, node_requirements=notin(fx.ZONE, "test-zone-3")))
    return prob


def definedness_problem():
    """Reason 9: example.com/k is a custom key the open pool leaves undefined; a NotIn pod may name it, an In pod may not — until a
    NotIn pod joined the claim (requirements.go:189)."""
    pools = [fx.node_pool("keyed", weight=10, requirements=[fx.req(K, "In", "a", "b")]), fx.node_pool("open")]
    pods = [fx.pod(requests={"cpu": "2"}, node_requirements=notin(K, "b")) for _ in range(3)] + [fx.pod(requests={"cpu": "1"}, node_selector={K: "a"}) for _ in range(3)]
    return fx.problem(fx.fake_instance_types(8), pools, pods)


def dne_mixed_problem():
    """Reason 10: DoesNotExist pods and NotIn pods on one key, over a pool with Exists on it (a NotIn pod turns the claim's Exists into
    NotIn, and the escape applies from then on)."""
    pools = [fx.node_pool("with", weight=10, requirements=[fx.req(fx.FAKE_EXOTIC_LABEL, "Exists")]), fx.node_pool("open")]
    pods = [fx.pod(requests={"cpu": "2"}, node_requirements=notin(fx.FAKE_EXOTIC_LABEL, "optional")) for _ in range(3)]
    pods += [fx.pod(requests={"cpu": "1"}, node_requirements=[fx.req(fx.FAKE_EXOTIC_LABEL, "DoesNotExist")]) for _ in range(3)]
    return fx.problem(fx.fake_instance_types(8), pools, pods)


def notin_bounds_problem():
    """Reason 11: a pod's integer NotIn [1] under a pool with integer Gt 2 — the claim prints the pod's value, outside the bounds."""
    pools = [fx.node_pool("above", weight=10, requirements=[fx.req(fx.FAKE_INTEGER_LABEL, "Gt", 2)]), fx.node_pool("open")]
    pods = [fx.pod(requests={"cpu": "2"}, node_requirements=notin(fx.FAKE_INTEGER_LABEL, 1, 5)) for _ in range(4)] + [fx.pod(requests={"cpu": "1"}) for _ in range(3)]
    return fx.problem(fx.fake_instance_types(8), pools, pods)


def exists_undefined_problem():
    """Reason 12: a pod's zone Exists over the open pool, which leaves the zone undefined — the claim prints Exists."""
    pods = [fx.pod(requests={"cpu": "2"}, node_requirements=[fx.req(fx.ZONE, "Exists")]) for _ in range(3)] + [fx.pod(requests={"cpu": "1"}) for _ in range(3)]
    return fx.problem(fx.fake_instance_types(8), [fx.node_pool("open")], pods)


# ---- seeded fuzz ---------------------------------------------------------------------------------------------------------------------

FUZZ_REASONS = {9, 10, 11, 12}   # what a seed that leaves the cursor engine may name: the by-design declines (csrc/decline.h)


def _turn(rng, r, plan):
    """A pod shape's In requirement turned into a negative one on the same key, the way `plan` allows for the key (so that the
    by-design declines stay rare): NotIn of the values it did NOT select (the pod still fits what it fitted), or DoesNotExist."""
    key, kind = r["key"], plan.get(r["key"])
    domain = {fx.ZONE: ZONES, fx.CAPACITY_TYPE: ["spot", "on-demand"], fx.FAKE_INTEGER_LABEL: [str(i) for i in range(1, 9)], fx.FAKE_EXOTIC_LABEL: ["optional"]}[key]
    if kind == "NotIn":
        rest = [v for v in domain if v not in r["values"]]
        return fx.req(key, "NotIn", *rest) if rest else r
    if kind == "DoesNotExist":
        return fx.req(key, "DoesNotExist")
    return r


def fuzz_problem(seed):
    """oc.fuzz_problem(seed) with each pod shape's selector turned, with probability about one third, into NotIn / DoesNotExist on the
    same keys. Per key one kind of turn, chosen so that the batch stays inside the engine's shape: NotIn where no pool bounds the key,
    DoesNotExist on `special` where no pool requires NotIn on it (a pod with special DoesNotExist fits the small types of the open
    pool). No Exists: the open pool defines no key, and a pod's Exists on a key a pool leaves undefined is a by-design decline (12) —
    the known case pc.exists_problem covers it. Every pod still fits the open pool."""
    prob = oc.fuzz_problem(seed)
    rng = random.Random(77000 + seed)
    pools = prob["nodePools"]
    ops = lambda key: [r["operator"] for p in pools for r in p.get("requirements", []) if r["key"] == key]
    plan = {}
    for key in (fx.ZONE, fx.CAPACITY_TYPE, fx.FAKE_INTEGER_LABEL, fx.FAKE_EXOTIC_LABEL):
        if key == fx.FAKE_EXOTIC_LABEL:
            plan[key] = "DoesNotExist" if "NotIn" not in ops(key) and rng.random() < 0.5 else None
        elif not {"Gt", "Lt"} & set(ops(key)):
            plan[key] = "NotIn"
    seen = {}
    for p in prob["pods"]:
        # (pods of one shape share their selectors: turn a shape once, by its content)
        shape = (repr(p.get("nodeSelector")), repr(pod_reqs(p)))
        if shape not in seen:
            reqs = [fx.req(k, "In", v) for k, v in sorted((p.get("nodeSelector") or {}).items())] + pod_reqs(p)
            out = []
            for r in reqs:
                if r["key"] == fx.FAKE_EXOTIC_LABEL and plan.get(r["key"]) == "DoesNotExist":
                    # (a pod that selected special = optional needs a large type: it keeps its selector; DoesNotExist goes to pods without one, below)
                    out.append(r)
                elif rng.random() < 0.34:
                    out.append(_turn(rng, r, plan))
                else:
                    out.append(r)
            if plan.get(fx.FAKE_EXOTIC_LABEL) == "DoesNotExist" and not any(r["key"] in (fx.FAKE_EXOTIC_LABEL, fx.FAKE_INTEGER_LABEL) for r in out) and rng.random() < 0.34:   # (no `integer`: it may select the large types alone)
                out.append(fx.req(fx.FAKE_EXOTIC_LABEL, "DoesNotExist"))
            seen[shape] = out
        p.pop("nodeSelector", None)
        p.pop("nodeAffinity", None)
        if seen[shape]:
            p["nodeAffinity"] = {"required": [[dict(r) for r in seen[shape]]]}
    return prob


FUZZ_SEEDS = list(range(40))
GPU_FUZZ_SEEDS = list(range(0, 40, 4))


def run_fuzz(oracle, lib, seeds):
    """Every seed equals the oracle under "auto-pod-operators", and the oracle reports no pod error for any. Returns (seeds that ended
    on the cursor engine with reason 0, {seed: reason} of the rest, seeds with a pod requirement that is not an In set)."""
    on_cursor, rest, turned = 0, {}, 0
    for seed, prob, want, got, on, reason in ec.fuzz_cases(oracle, lib, ((seed, fuzz_problem(seed)) for seed in seeds), AUTO, pops=False, mode=SWITCH.mode):
        turned += any(r["operator"] != "In" for p in prob["pods"] for r in pod_reqs(p))
        assert not want["podErrors"], (seed, want["podErrors"])
        if on == "cursor":
            on_cursor += 1
        else:
            assert reason in FUZZ_REASONS, (seed, got["counters"])
            rest[seed] = reason
    print(f"auto-pod-operators kept {on_cursor} of {len(seeds)} seeds on the cursor engine; reasons of the rest {rest}; {turned} seeds carry pod operators")
    return on_cursor, rest, turned
