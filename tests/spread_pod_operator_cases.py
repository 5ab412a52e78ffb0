"""Topology batches whose PODS carry requirements that are not In sets — NotIn, Exists, DoesNotExist — for the spread engine's pod
operators (csrc/topo_engine.h, "The spread engine's pod operators"; engines "auto-pod-operators-spread" / "spread-pod-operators", 29 / 30;
tests/test_spread_engine_pod_operators.py on the emulation, tests/test_gpu_spread_pod_operators.py on the device): known shapes, the
Switch, the seeded fuzz generator and its runner.

What the reference does: a pod's own requirement is the pod's side of the domain choice (podDomains, topology.go:230 — domainMinCount
runs over the domains the pod supports, topologygroup.go:300-322), it narrows the NodeClaim like any requirement (requirements.go:
254-274; a complement set stays a complement set, and Record counts a claim only once its set is ONE concrete value, topology.go:207),
and — for a pod that owns a spread constraint — it is a term of the group's TopologyNodeFilter (topologynodefilter.go:38-97), whose
strict Compatible fails an In / Exists term on a key the bin does not define and passes a NotIn / DoesNotExist term there."""
import copy
import random

import daemonset_cases as dc
import engine_checks as ec
import operator_cases as oc
import pod_operator_cases as pc
import spread_filter_cases as sf
import spread_operator_cases as so
from karpenter_amd import fixtures as fx

ZONES, WEB = oc.ZONES, {"app": "web"}
SPOT, ON_DEMAND = "spot", "on-demand"
notin, claims_of, req_of = pc.notin, oc.claims_of, oc.req_of
# 29, 30 over 26 / 25 (every switch but the one under test): what every setting up to 27 does is to decline with the reason given per
# call — 4 for NotIn / Exists pods, 8 for DoesNotExist. The oracle's result has no pod errors.
SWITCH = ec.Switch("spread", only="spread-pod-operators", auto="auto-pod-operators-spread", base="auto-pod-operators", base_only="spread-filters", errors=False)
ONLY, AUTO, BASE, BASE_ONLY = SWITCH.only, SWITCH.auto, SWITCH.base, SWITCH.base_only
# ... and for a problem that leaves pods unschedulable: pod errors required, queue pops compared, no engine-only leg below the switch
UNSCHEDULABLE = SWITCH._replace(errors=True, pops=True, base_only=None)
check_declined = SWITCH.declined
lone_cell = so.lone_cell


def check_engine(oracle, lib, prob, reason=4, want=None):
    return SWITCH.check(oracle, lib, prob, reason=reason, want=want)


def check_unschedulable(oracle, lib, prob, reason=4):
    return UNSCHEDULABLE.check(oracle, lib, prob, reason=reason)


def problem(pods, pools=None, n_types=8, **kw):
    return fx.problem(fx.fake_instance_types(n_types), pools or [fx.node_pool("open")], pods, **kw)


def spread_pods(n, cpu="1", labels=WEB, reqs=None, key=fx.ZONE, **kw):
    """n pods `labels` that own a spread on `key` over `labels` and carry the node-affinity term `reqs`."""
    return [fx.pod(requests={"cpu": cpu}, labels=labels, node_requirements=reqs, topology_spread=[fx.spread(key, labels, **kw)]) for _ in range(n)]


def spread_uids(prob):
    return {p["uid"] for p in prob["pods"] if p.get("topologySpreadConstraints")}


def by_zone(res, prob):
    """How many of the pods that own a spread constraint sit in each zone, on claims narrowed to it."""
    return so.pods_by_zone(res, spread_uids(prob))


# ---- 1: a lone zone NotIn pod beside a spread: pod_operator_cases.spread_problem() ------------------------------------------------

# ---- 2: the spread pods carry the NotIn themselves ---------------------------------------------------------------------------------

def own_notin_problem(n=8):
    """Eight pods with a zonal spread (maxSkew 1) and zone NotIn [test-zone-3] over the open pool: zones 1 and 2 only, four each —
    the skew is taken over the two domains the pods support — beside four pods without constraints."""
    return problem(spread_pods(n, reqs=notin(fx.ZONE, ZONES[2])) + [fx.pod(requests={"cpu": "2"}) for _ in range(4)])


# ---- 3: counted but not concrete -----------------------------------------------------------------------------------------------------

def counted_problem(operator="NotIn"):
    """spread_operator_cases.counted_problem with the complement coming from PODS: three 7-cpu pods app=web without a constraint and
    zone NotIn [test-zone-1, test-zone-2] take a claim each — a complement set that admits test-zone-3 alone, not a concrete one: they
    count for nothing and the six spread pods land 2 / 2 / 2. With zone In [test-zone-3] instead they count: 3 / 3 / 0."""
    reqs = notin(fx.ZONE, ZONES[0], ZONES[1]) if operator == "NotIn" else [fx.req(fx.ZONE, "In", ZONES[2])]
    return problem([fx.pod(requests={"cpu": "7"}, labels=WEB, node_requirements=reqs) for _ in range(3)] + so.spread_pods(6))


# ---- 4: a NotIn filter term against a key the pool leaves undefined --------------------------------------------------------------------

def undefined_term_problem(operator="NotIn"):
    """The build of spread_filter_cases: three big pods app=web pinned to test-zone-1, no affinity on the capacity type, on claims of
    the open pool, where capacity-type is undefined; six owners whose term is capacity-type NotIn [spot] — it passes a bin that does
    not define the key: counted, 0 / 3 / 3 — or In [on-demand] — it fails there: not counted, 2 / 2 / 2."""
    reqs = notin(fx.CAPACITY_TYPE, SPOT) if operator == "NotIn" else [fx.req(fx.CAPACITY_TYPE, "In", ON_DEMAND)]
    return problem(sf.big() + spread_pods(6, reqs=reqs))


# ---- 5: a NotIn pod defines the key, an In term reads it ---------------------------------------------------------------------------------

def defined_by_notin_problem(joiner=True):
    """spread_filter_cases.then_concrete_problem with a joiner that is NEGATIVE: one 3-cpu big pod app=web on an open-pool claim
    (capacity-type undefined: not counted by the owners' filter capacity-type In [on-demand]); a 2-cpu pod without labels with
    capacity-type NotIn [spot] joins it — the claim now DEFINES the key, as NotIn [spot], which shares on-demand with the term; the
    two 1200m pods app=web that follow ARE counted. Without the joiner they are not."""
    pods = sf.big(1, "3")
    if joiner:
        pods += [fx.pod(requests={"cpu": "2"}, node_selector={fx.ZONE: ZONES[0]}, node_requirements=notin(fx.CAPACITY_TYPE, SPOT))]
    return problem(pods + sf.big(2, "1200m") + sf.owners(4))


# ---- 6: two dictionary-key groups, NotIn on one key ---------------------------------------------------------------------------------------

def two_keys_problem():
    """Thirty pods with a zone spread (maxSkew 3) and a capacity-type spread (maxSkew 4) that carry zone NotIn [test-zone-3], six pods
    without constraints; pool `both` (capacity-type In [spot, on-demand]) in front of the open one."""
    pools = [fx.node_pool("both", weight=10, requirements=[fx.req(fx.CAPACITY_TYPE, "In", SPOT, ON_DEMAND)]), fx.node_pool("open")]
    pods = [fx.pod(requests={"cpu": "500m"}, labels=WEB, node_requirements=notin(fx.ZONE, ZONES[2]),
                   topology_spread=[fx.spread(fx.ZONE, WEB, max_skew=3), fx.spread(fx.CAPACITY_TYPE, WEB, max_skew=4)]) for _ in range(30)]
    return problem(pods + [fx.pod(requests={"cpu": "1"}) for _ in range(6)], pools, n_types=12)


# ---- 7: zonal affinity and anti-affinity over NotIn pods ---------------------------------------------------------------------------------

def affinity_problem():
    """spread_operator_cases.affinity_problem over the open pool with the selectors written as NotIn: two pods with anti-affinity
    on the zone, `NotIn` of the other two zones each (each blocks its zone for the other through the group and its inverse group), a
    pod their selector matches that owns nothing, pods with zonal self-affinity per label that exclude test-zone-1, pods without
    constraints."""
    lonely = {"zone-lonely": "x"}
    pods = [fx.pod(requests={"cpu": "2"}, labels=dict(lonely, **{"my-label": "a"}), pod_anti_requirements=[fx.affinity_term(fx.ZONE, lonely)],
                   node_requirements=notin(fx.ZONE, *[o for o in ZONES if o != z])) for z in ZONES[1:]]
    pods.append(fx.pod(requests={"cpu": "300m"}, labels=lonely))
    for lab in ({"my-label": "a"}, {"my-label": "b"}):
        pods += [fx.pod(requests={"cpu": "1500m"}, labels=lab, pod_requirements=[fx.affinity_term(fx.ZONE, lab)], node_requirements=notin(fx.ZONE, ZONES[0])) for _ in range(7)]
    pods += [fx.pod(requests={"cpu": "700m"}, labels={"my-label": "c"}) for _ in range(5)]
    return problem(pods)


# ---- 8: DoesNotExist beside a spread -----------------------------------------------------------------------------------------------------

def dne_problem():
    """pod_operator_cases.dne_problem's pools and pods, and twelve pods with a zonal spread."""
    prob = pc.dne_problem()
    prob["pods"] += so.spread_pods(12)
    return prob


def dne_term_problem(defined=True):
    """The owners' term is special DoesNotExist. The three big pods app=web select nothing on the key; `defined`: the heavy pool
    requires special In [optional], their claims define the key and the term fails there — not counted, 2 / 2 / 2. Without the
    requirement their claims leave the key undefined and the term passes: 0 / 3 / 3. (The owners land on the open pool either way.)"""
    pools = [fx.node_pool("heavy", weight=10, requirements=[fx.req(fx.FAKE_EXOTIC_LABEL, "In", "optional")] if defined else None), fx.node_pool("open")]
    return problem(sf.big() + spread_pods(6, reqs=[fx.req(fx.FAKE_EXOTIC_LABEL, "DoesNotExist")]), pools)


# ---- 9: a pod's zone Exists over pools that define the zone --------------------------------------------------------------------------------

def exists_problem():
    """pod_operator_cases.exists_problem's pools (zone In [1, 2] tainted, zone NotIn [1]); its Exists pods, and nine spread pods that
    carry zone Exists themselves: the term is Exists, and every claim of these pools defines the zone."""
    prob = pc.exists_problem()
    owners = spread_pods(9, cpu="500m", reqs=[fx.req(fx.ZONE, "Exists")])
    for p in owners:   # (test-zone-1 is the tainted pool's alone)
        p["tolerations"] = fx.pod(tolerations=oc.tolerate("two"))["tolerations"]
    prob["pods"] += owners
    return prob


# ---- 10: unschedulable pods --------------------------------------------------------------------------------------------------------------

def no_zone_problem():
    """2 with two spread pods app=api whose NotIn excludes every zone: Topology (3) on the open pool."""
    prob = own_notin_problem()
    prob["pods"] += spread_pods(2, labels={"app": "api"}, reqs=notin(fx.ZONE, *ZONES))
    return prob


def dne_owner_problem():
    """Eight positive spread pods, four pods without constraints, and two pods app=api that require zone DoesNotExist and own a zonal
    spread: no domain the pod supports — Topology (3). (Beside zone NotIn pods the batch would be the by-design decline 10.)"""
    return problem(so.spread_pods(8) + [fx.pod(requests={"cpu": "2"}) for _ in range(4)] + spread_pods(2, labels={"app": "api"}, reqs=[fx.req(fx.ZONE, "DoesNotExist")]))


def incompatible_problem():
    """pod_operator_cases.incompatible_problem (zone NotIn [test-zone-1] and special DoesNotExist against a pool pinned to test-zone-1
    with special Exists: Incompatible, 2) with six spread pods, which are placed."""
    prob = pc.incompatible_problem()
    prob["pods"] += so.spread_pods(6)
    return prob


# ---- 11: a limit stage ---------------------------------------------------------------------------------------------------------------------

def limit_problem():
    prob = pc.limit_problem()
    prob["pods"] += so.spread_pods(12)
    return prob


# ---- 12: DaemonSet overhead ------------------------------------------------------------------------------------------------------------------

def daemonset_problem():
    prob = own_notin_problem()
    prob["daemonSetPods"] = dc.random_daemonsets(random.Random(32000), ZONES)
    return prob


# ---- 13: still declined ------------------------------------------------------------------------------------------------------------------------

def nodes_problem():
    """Existing nodes and negative pods: out of scope (a negative pod may add a key to a node)."""
    return fx.with_existing_nodes(own_notin_problem(), 4, seed=3, small=True)


def pod_gt_problem():
    prob = own_notin_problem()
    prob["pods"].append(fx.pod(requests={"cpu": "1"}, node_requirements=[fx.req(fx.FAKE_INTEGER_LABEL, "Gt", 4)]))
    return prob


def topology_twin(prob):
    """A by-design decline of the cursor engine's pod operators (9-12) as a topology batch: the same pods, and six with a zonal spread."""
    prob["pods"] += so.spread_pods(6)
    return prob


BY_DESIGN = [(pc.definedness_problem, 9), (pc.dne_mixed_problem, 10), (pc.notin_bounds_problem, 11), (pc.exists_undefined_problem, 12)]


def filter_gt_problem():
    """The owners' term carries integer Gt 2 beside a NotIn: pod-side bounds are reason 1, decided on the host, whatever the filter
    would say (43 is what the kernel keeps for a bounded term it is shown)."""
    return problem(sf.big() + spread_pods(6, reqs=notin(fx.CAPACITY_TYPE, SPOT) + [fx.req(fx.FAKE_INTEGER_LABEL, "Gt", 2)]))


def too_many_slots_problem(n=33):
    """spread_filter_cases.too_many_slots_problem with NotIn terms: n Deployments app=w<i>, each a 3-cpu pod that selects nothing but
    its zone beside two owners with capacity-type NotIn [spot]: n groups whose filter is decided per claim, one more than the 32
    slots of a batch with negative terms (a positive batch keeps its sixteen: spread_filter_cases.too_many_slots_problem)."""
    pods = []
    for i in range(n):
        lab = {"app": f"w{i}"}
        pods += sf.big(1, "3", labels=lab) + spread_pods(2, labels=lab, reqs=notin(fx.CAPACITY_TYPE, SPOT))
    return problem(pods)


# ---- 14: positive batches stay what they are -------------------------------------------------------------------------------------------------

def positive_problems():
    """Known problems of the complement-template and the node-filter cases, existing nodes included: no negative pod, no negative term."""
    return [so.counted_problem(), so.bounds_problem(), so.two_keys_problem(), so.affinity_problem(), so.limit_notin_problem(), so.nodes_mix_problem(),
            sf.by_template_problem(), sf.undefined_problem(), sf.then_concrete_problem(), sf.complement_problem(), sf.custom_key_problem(), sf.taint_problem(),
            sf.limit_stage_problem(), sf.node_problem(), sf.tainted_node_problem(), sf.set_aside_problem()]


# ---- 17: members of one SolveMany --------------------------------------------------------------------------------------------------------------

def many_members():
    return [(own_notin_problem(), AUTO), (undefined_term_problem(), AUTO), (sf.by_template_problem(), AUTO)]


# ---- seeded fuzz ---------------------------------------------------------------------------------------------------------------------------------

# what may take a seed off the spread engine under "auto-pod-operators-spread" (csrc/decline.h): 43 beyond the filter slots' caps, 6
# keys that do not pack (a phantom bit per field), 50 a sixteenth domain
FUZZ_REASONS = {43, 6, 50}
DOMAIN = {fx.ZONE: ZONES, fx.CAPACITY_TYPE: [SPOT, ON_DEMAND]}


def fuzz_problem(seed):
    """spread_operator_cases.fuzz_problem(seed), then per pod SHAPE (labels, nodeSelector, node affinity, constraints — the pods of
    one Deployment), with probability 0.2, one more required node-affinity term on the zone or the capacity type — a key no NodePool
    bounds with Gt / Lt: a nodeSelector on the key becomes NotIn of the other values (the pod fits what it fitted), otherwise NotIn
    [one zone] / NotIn [spot] is added. No Exists, no DoesNotExist, no custom key: the preconditions of reasons 9-12 cannot arise. A
    seed whose draws turned no shape turns its first one. An RNG of its own."""
    prob = so.fuzz_problem(seed)
    rng = random.Random(55000 + seed)
    bounded = {r["key"] for p in prob["nodePools"] for r in p.get("requirements", []) if r["operator"] in ("Gt", "Lt")}
    keys = [k for k in (fx.ZONE, fx.CAPACITY_TYPE) if k not in bounded]
    shapes = {}   # shape -> (turned, key, the zone an added NotIn names), in order of first appearance
    for p in prob["pods"]:
        shape = repr((sorted(p["labels"].items()), p.get("nodeSelector"), p.get("nodeAffinity"), p.get("topologySpreadConstraints"), p.get("podAffinity"), p.get("podAntiAffinity")))
        if shape not in shapes:
            shapes[shape] = (rng.random() < 0.2 and bool(keys), rng.choice(keys) if keys else None, rng.choice(ZONES))
        p["_shape"] = shape
    if keys and not any(t for t, _, _ in shapes.values()):
        first = next(iter(shapes))
        shapes[first] = (True,) + shapes[first][1:]
    for p in prob["pods"]:
        turned, key, zone = shapes[p.pop("_shape")]
        if not turned:
            continue
        sel = dict(p.get("nodeSelector") or {})
        if key in sel:
            kept = sel.pop(key)
            term = fx.req(key, "NotIn", *[v for v in DOMAIN[key] if v != kept])
            p.pop("nodeSelector")
            if sel:
                p["nodeSelector"] = sel
        else:
            term = fx.req(key, "NotIn", zone if key == fx.ZONE else SPOT)
        na = copy.deepcopy(p.get("nodeAffinity") or {})
        na["required"] = [list(t) + [dict(term)] for t in (na.get("required") or [[]])]
        p["nodeAffinity"] = na
    return prob


def negative(prob):
    return any(r["operator"] != "In" for p in prob["pods"] for t in (p.get("nodeAffinity") or {}).get("required", []) for r in t)


FUZZ_SEEDS = list(range(120))
GPU_FUZZ_SEEDS = FUZZ_SEEDS[::4]


def run_fuzz(oracle, lib, seeds):
    """Every seed carries a negative pod and equals the oracle under "auto-pod-operators-spread", pod errors and queue pops included.
    Returns (seeds on the spread engine with reason 0, {seed: reason} of the rest — reasons of FUZZ_REASONS only, seeds whose oracle
    result leaves pods unschedulable)."""
    on_spread, rest, errors = 0, {}, 0
    for seed, prob, want, got, on, reason in ec.fuzz_cases(oracle, lib, ((seed, fuzz_problem(seed)) for seed in seeds), AUTO, pops=True, mode=SWITCH.mode):
        assert negative(prob), seed
        errors += bool(want["podErrors"])
        if on == "spread":
            on_spread += 1
        else:
            assert reason in FUZZ_REASONS, (seed, got["counters"])
            rest[seed] = reason
    print(f"{AUTO}: {on_spread} of {len(seeds)} seeds on the spread engine; reasons of the rest {rest}; {errors} seeds leave pods unschedulable")
    return on_spread, rest, errors
