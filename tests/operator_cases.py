"""Problems whose NodePools carry requirements that are not In sets — NotIn, Exists, DoesNotExist, Gt, Lt — for the cursor engine's
complement templates (csrc/fast_engine.h FastCold::setup, "Complement templates"; engines "auto-operators" / "cursor-operators";
tests/test_cursor_engine_operators.py on the emulation, tests/test_gpu_cursor_operators.py on the device): known shapes, the seeded
fuzz generator and its Switch (tests/engine_checks.py).

What the reference does with such a pool: the NodeClaim starts with the pool's requirement as it stands (requirement.go:60-112: a
complement set, bounds for Gt / Lt); a pod's In Q meets it by Intersection (requirement.go:181-214) and leaves the concrete set of
Q's values outside the pool's NotIn set and inside its bounds, complement off, bounds dropped; instance types meet it by Intersects
(requirements.go:254-274), where two sides that are both NotIn / DoesNotExist pass without an intersection (:260-265).

Every problem here has an open NodePool of the lowest weight, so that the oracle leaves no pod unschedulable (reason 27 is not what
these cases are about)."""
import random

import engine_checks as ec
from karpenter_amd import fixtures as fx

K = "example.com/k"
ZONES = ["test-zone-1", "test-zone-2", "test-zone-3"]
# 15, 16 over "auto" / "cursor" ("auto-nodes" / "cursor-nodes" for a problem with existing nodes, which "auto" does not try): what
# engines 0-14 do is to decline with the reason given per call — 3 for NotIn / Exists / DoesNotExist pools, 1 for Gt / Lt pools (34
# with existing nodes). The engine-only setting declines with 3 alone; the host finds 1 and 34 when it creates the handle ("outside its
# shape ... (reason N)"). The oracle's result has no pod errors.
SWITCH = ec.Switch("cursor", only="cursor-operators", auto="auto-operators", base="auto", base_only="cursor", base_only_declines=(3,), errors=False)
check_declined = SWITCH.declined


def check_engine(oracle, lib, prob, reason, base="auto", base_cursor="cursor"):
    """One problem five ways (SWITCH.check): the claims' requirements are compared by operator, values and bounds (parity.canon_req)."""
    return SWITCH.check(oracle, lib, prob, reason=reason, base=base, base_only=base_cursor)


def claims_of(res, pool):
    return [c for c in res["newNodeClaims"] if c["nodePool"] == pool]


def req_of(claim, key):
    """(operator, sorted values) of the claim's requirement on `key`, None when it has none."""
    for r in claim["requirements"]:
        if r["key"] == key:
            return r["operator"], sorted(r["values"])
    return None


def tolerate(key):
    return [{"key": key, "operator": "Exists"}]


def taint(key):
    return [{"key": key, "value": "x", "effect": "NoSchedule"}]


# ---- 1: bounds on a key no pod selects on -----------------------------------------------------------------------------------------

def bounds_problem():
    """1..8-cpu catalogue (label `integer` = cpus). Pool `above` (weight 10, tainted): integer Gt 2; pool `below` (weight 5): integer
    Lt 3; pool `open`. Half of the pods tolerate the taint and land on `above`; of the others those that fit a 2-cpu type land on
    `below`, the 3-cpu ones on `open`."""
    pools = [fx.node_pool("above", weight=10, requirements=[fx.req(fx.FAKE_INTEGER_LABEL, "Gt", 2)], taints=taint("above")),
             fx.node_pool("below", weight=5, requirements=[fx.req(fx.FAKE_INTEGER_LABEL, "Lt", 3)]), fx.node_pool("open")]
    pods = []
    for i, cpu in enumerate(["3", "1500m", "1", "700m", "250m"] * 12):
        pods.append(fx.pod(requests={"cpu": cpu, "memory": "256Mi"}, tolerations=tolerate("above") if i % 2 else None))
    return fx.problem(fx.fake_instance_types(8), pools, pods)


def integer_of(prob):
    return {it["name"]: int(next(r["values"][0] for r in it["requirements"] if r["key"] == fx.FAKE_INTEGER_LABEL)) for it in prob["instanceTypes"]}


# ---- 2: NotIn on a key pods select on ---------------------------------------------------------------------------------------------

def notin_zone_pool(**kw):
    return fx.node_pool("not-zone-1", weight=10, requirements=[fx.req(fx.ZONE, "NotIn", "test-zone-1")], **kw)


def notin_zone_pods():
    """Queue order is by size: four 7-cpu pods without a selector (a claim each, nothing else fits beside them), two 5-cpu pods
    without one, then 2-cpu pods that admit all three zones (node affinity) — they join the 5-cpu claims, whose NotIn [test-zone-1]
    becomes the concrete In [test-zone-2, test-zone-3] —, 1-cpu pods pinned to test-zone-2, which narrow a claim to In [test-zone-2],
    and pods pinned to test-zone-1, which the pool cannot take."""
    pods = [fx.pod(requests={"cpu": "7"}) for _ in range(4)] + [fx.pod(requests={"cpu": "5"}) for _ in range(2)]
    pods += [fx.pod(requests={"cpu": "2"}, node_requirements=[fx.req(fx.ZONE, "In", *ZONES)]) for _ in range(5)]
    pods += [fx.pod(requests={"cpu": "1"}, node_selector={fx.ZONE: "test-zone-2"}) for _ in range(6)]
    pods += [fx.pod(requests={"cpu": "1200m"}, node_selector={fx.ZONE: "test-zone-1"}) for _ in range(4)]
    return pods


def notin_problem():
    return fx.problem(fx.fake_instance_types(8), [notin_zone_pool(), fx.node_pool("open")], notin_zone_pods())


def zone_kinds(res, pool="not-zone-1"):
    return {req_of(c, fx.ZONE) and (req_of(c, fx.ZONE)[0], tuple(req_of(c, fx.ZONE)[1])) for c in claims_of(res, pool)}


NOTIN_KINDS = {("NotIn", ("test-zone-1",)), ("In", ("test-zone-2", "test-zone-3")), ("In", ("test-zone-2",))}


# ---- 3: DoesNotExist and Exists ---------------------------------------------------------------------------------------------------

def exists_problem():
    """The fake catalogue labels its large types (more than 4 cpu) `special In [optional]` and the others `special DoesNotExist`.
    Pool `without` (weight 10): special DoesNotExist — the small types only, by the escape of requirements.go:260-265; a pod that
    selects on `special` cannot go there. Pool `with` (weight 5): special Exists — the large types only."""
    pools = [fx.node_pool("without", weight=10, requirements=[fx.req(fx.FAKE_EXOTIC_LABEL, "DoesNotExist")]),
             fx.node_pool("with", weight=5, requirements=[fx.req(fx.FAKE_EXOTIC_LABEL, "Exists")]), fx.node_pool("open")]
    pods = [fx.pod(requests={"cpu": "5"}) for _ in range(3)] + [fx.pod(requests={"cpu": c}) for c in ["1", "500m", "1500m"] * 8]
    pods += [fx.pod(requests={"cpu": "1"}, node_selector={fx.FAKE_EXOTIC_LABEL: "optional"}) for _ in range(6)]
    return fx.problem(fx.fake_instance_types(8), pools, pods)


# ---- 4: the escape rule -----------------------------------------------------------------------------------------------------------

def escape_problem():
    """Three instance types that differ in their requirement on example.com/k — DoesNotExist, NotIn [x], In [y] — and three tainted
    pools, each with one pod that tolerates only its taint: k NotIn [y] keeps the first two (DoesNotExist meets NotIn without an
    intersection: the escape), k Exists the last two, k Gt 0 the NotIn type alone (y is no integer, and DoesNotExist meets neither)."""
    its = [fx.fake_instance_type("k-absent", requirements=[fx.req(K, "DoesNotExist")]),
           fx.fake_instance_type("k-not-x", requirements=[fx.req(K, "NotIn", "x")]),
           fx.fake_instance_type("k-is-y", requirements=[fx.req(K, "In", "y")])]
    pools = [fx.node_pool("not-y", weight=30, requirements=[fx.req(K, "NotIn", "y")], taints=taint("not-y")),
             fx.node_pool("exists", weight=20, requirements=[fx.req(K, "Exists")], taints=taint("exists")),
             fx.node_pool("positive", weight=10, requirements=[fx.req(K, "Gt", 0)], taints=taint("positive")), fx.node_pool("open")]
    pods = [fx.pod(requests={"cpu": "1"}, tolerations=tolerate(p)) for p in ("not-y", "exists", "positive")] + [fx.pod(requests={"cpu": "1"})]
    return fx.problem(its, pools, pods)


# ---- 5: Gt on a key pods select on, kwok catalogue ----------------------------------------------------------------------------------

def kwok_problem():
    """kwok catalogue of 24 types (1, 2, 4, 8 cpu x families c, s, m). Pool `big`: instance-cpu Gt 3 and instance-family NotIn [c];
    pods select instance-cpu In [2, 4, 8] (the pool leaves 4 and 8), instance-size In [4] or [8], or nothing; pods that select
    instance-cpu In [2] go to the open pool."""
    pools = [fx.node_pool("big", weight=10, requirements=[fx.req(fx.KWOK_CPU, "Gt", 3), fx.req(fx.KWOK_FAMILY, "NotIn", "c")]), fx.node_pool("open")]
    for p in pools:
        p["nodeClassLabelKey"] = "karpenter.kwok.sh/kwoknodeclass"
    pods = [fx.pod(requests={"cpu": "1500m", "memory": "1Gi"}, node_requirements=[fx.req(fx.KWOK_CPU, "In", "2", "4", "8")]) for _ in range(10)]
    pods += [fx.pod(requests={"cpu": "900m", "memory": "512Mi"}, node_requirements=[fx.req(fx.KWOK_SIZE, "In", s)]) for s in ("4", "8") for _ in range(5)]
    pods += [fx.pod(requests={"cpu": "500m", "memory": "512Mi"}) for _ in range(12)]
    pods += [fx.pod(requests={"cpu": "600m", "memory": "256Mi"}, node_selector={fx.KWOK_CPU: "2"}) for _ in range(5)]
    return fx.problem(fx.kwok_catalog(24), pools, pods, well_known=fx.KWOK_WELL_KNOWN)


# ---- 6: a limit stage of a complement template --------------------------------------------------------------------------------------

def limit_problem():
    """Case 2's pool with limits.cpu = 36: every claim lists the 8-cpu type, so subtractMax takes 8 per claim (36 -> 28 -> 20 -> 12 ->
    4) and the fifth claim opens under the list narrowed to the types of at most 4 cpu — a limit stage, which copies the template's
    packed requirement set, guard bit included."""
    pods = [fx.pod(requests={"cpu": "3"}) for _ in range(10)] + [fx.pod(requests={"cpu": "1"}, node_selector={fx.ZONE: "test-zone-2"}) for _ in range(6)]
    pods += [fx.pod(requests={"cpu": "1"}) for _ in range(10)]
    return fx.problem(fx.fake_instance_types(8), [notin_zone_pool(limits={"cpu": "36"}), fx.node_pool("open")], pods)


# ---- 7: existing nodes and a DaemonSet ----------------------------------------------------------------------------------------------

def nodes_problem():
    prob = fx.with_existing_nodes(bounds_problem(), 4, seed=3, small=True)
    prob["daemonSetPods"] = [fx.pod(uid="daemonset-agent", requests={"cpu": "100m", "memory": "64Mi"}, tolerations=[{"operator": "Exists"}])]
    return prob


# ---- 8: still declined --------------------------------------------------------------------------------------------------------------

def pod_notin_problem():
    prob = notin_problem()
    prob["pods"].append(fx.pod(requests={"cpu": "1"}, node_requirements=[fx.req(fx.ZONE, "NotIn", "test-zone-3")]))
    return prob


def min_values_problem():
    prob = notin_problem()
    prob["nodePools"][0]["requirements"].append(fx.req(fx.INSTANCE_TYPE, "Exists", min_values=2))
    return prob


def pod_gt_problem():
    prob = bounds_problem()
    prob["pods"].append(fx.pod(requests={"cpu": "1"}, node_requirements=[fx.req(fx.FAKE_INTEGER_LABEL, "Gt", 4)]))
    return prob


def spread_problem():
    """A zonal spread over case 2's pool: a topology batch, which the spread engine declines under every setting."""
    pods = [fx.pod(requests={"cpu": "1"}, labels={"app": "web"}, topology_spread=[fx.spread(fx.ZONE, {"app": "web"})]) for _ in range(12)]
    return fx.problem(fx.fake_instance_types(8), [notin_zone_pool(), fx.node_pool("open")], pods + [fx.pod(requests={"cpu": "2"}) for _ in range(4)])


# ---- 9: seeded fuzz -----------------------------------------------------------------------------------------------------------------

def _pool_requirement(rng):
    """One random requirement that is not an In set (two times in three) over zone, capacity type, `integer` or `special`."""
    key = rng.choice([fx.ZONE, fx.CAPACITY_TYPE, fx.FAKE_INTEGER_LABEL, fx.FAKE_EXOTIC_LABEL])
    if key == fx.ZONE:
        vals = rng.sample(ZONES, rng.choice([1, 2]))
        return fx.req(key, rng.choice(["NotIn", "NotIn", "In"]), *vals) if rng.random() < 0.8 else fx.req(key, "Exists")
    if key == fx.CAPACITY_TYPE:
        return fx.req(key, rng.choice(["NotIn", "In"]), rng.choice(["spot", "on-demand"])) if rng.random() < 0.8 else fx.req(key, "Exists")
    if key == fx.FAKE_INTEGER_LABEL:
        op = rng.choice(["Gt", "Lt", "NotIn", "In"])
        if op == "Gt": return fx.req(key, op, rng.randint(0, 5))
        if op == "Lt": return fx.req(key, op, rng.randint(3, 9))
        return fx.req(key, op, *rng.sample(range(1, 9), rng.randint(1, 4)))
    return rng.choice([fx.req(key, "Exists"), fx.req(key, "DoesNotExist"), fx.req(key, "NotIn", "optional"), fx.req(key, "In", "optional")])


def fuzz_problem(seed):
    """Two to four weighted NodePools, each with one or two random requirements (and a taint one time in three), over the 1..8-cpu
    catalogue, plus the open pool; at most 60 pods of at most 800m with random In selectors — on the zone, the capacity type (never
    spot in test-zone-3, which has no such offering), `integer` or `special` — and random tolerations. Every pod fits some type of the
    open pool under its selectors, so the oracle schedules every pod."""
    rng = random.Random(51000 + seed)
    pools = []
    for i in range(rng.randint(2, 4)):
        reqs, seen = [], set()
        for _ in range(rng.randint(1, 2)):
            r = _pool_requirement(rng)
            if r["key"] not in seen:
                seen.add(r["key"]); reqs.append(r)
        pools.append(fx.node_pool(f"pool-{i}", weight=50 - 10 * i, requirements=reqs, taints=taint(f"pool-{i}") if rng.random() < 0.33 else None))
    pools.append(fx.node_pool("open"))
    shapes = []
    for _ in range(rng.randint(3, 9)):
        sel, reqs = {}, []
        if rng.random() < 0.5:
            zs = rng.sample(ZONES, rng.choice([1, 1, 2, 3]))
            reqs.append(fx.req(fx.ZONE, "In", *zs))
            if rng.random() < 0.4: sel[fx.CAPACITY_TYPE] = "on-demand" if "test-zone-3" in zs else rng.choice(["spot", "on-demand"])
        elif rng.random() < 0.3:
            sel[fx.CAPACITY_TYPE] = rng.choice(["spot", "on-demand"])
        pick = rng.random()
        if pick < 0.3: reqs.append(fx.req(fx.FAKE_INTEGER_LABEL, "In", *rng.sample(range(1, 9), rng.randint(1, 4))))
        elif pick < 0.45: sel[fx.FAKE_EXOTIC_LABEL] = "optional"
        tol = [t for i in range(len(pools) - 1) if rng.random() < 0.5 for t in tolerate(f"pool-{i}")]
        shapes.append(dict(requests={"cpu": rng.choice(["100m", "250m", "400m", "800m"]), "memory": rng.choice(["64Mi", "256Mi"])},
                           node_selector=sel or None, node_requirements=reqs or None, tolerations=tol or None))
    pods = [fx.pod(**rng.choice(shapes)) for _ in range(rng.randint(20, 60))]
    return fx.problem(fx.fake_instance_types(8), pools, pods)


FUZZ_SEEDS = list(range(40))
GPU_FUZZ_SEEDS = list(range(0, 40, 4))


def run_fuzz(oracle, lib, seeds):
    """Every seed equals the oracle under "auto-operators", and the oracle reports no pod error for any. Returns (seeds that ended on
    the cursor engine with reason 0, {seed: reason} of the rest)."""
    on_cursor, rest = 0, {}
    for seed, _, want, _, on, reason in ec.fuzz_cases(oracle, lib, ((seed, fuzz_problem(seed)) for seed in seeds), SWITCH.auto, pops=False, mode=SWITCH.mode):
        assert not want["podErrors"], (seed, want["podErrors"])
        if on == "cursor":
            on_cursor += 1
        else:
            rest[seed] = reason
    print(f"auto-operators kept {on_cursor} of {len(seeds)} seeds on the cursor engine; reasons of the rest {rest}")
    return on_cursor, rest
