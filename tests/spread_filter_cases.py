"""Topology batches whose spread groups carry a TopologyNodeFilter that can say no — the owner has a nodeSelector or required node
affinity, or honours taints over a tainted NodePool or node — for the spread engine's filter slots (csrc/topo_engine.h, "Topology
node filters"; engines "auto-filters-spread" / "spread-filters"; tests/test_spread_engine_filters.py on the emulation,
tests/test_gpu_spread_filters.py on the device): known shapes, the comparison helpers, the seeded fuzz generator and its runner.

What the reference does (topologynodefilter.go:38-97, topology.go:197-220): the filter is asked in Record alone. A pod the group
selects is counted on the claim or node it lands on only if some node-affinity term of the OWNER (merged with its nodeSelector) is
strictly Compatible with the bin's requirements — a key the bin does not define fails an In term even when the key is well known —
and, under nodeTaintsPolicy Honor, the owner tolerates the bin's taints. The domain choice never asks the filter.

Most known shapes come in PAIRS that differ in one thing — the policy, or what the heavier NodePool requires — and the tests assert
the placement that tells the two apart. The common build: three "big" pods labelled app=web that own no constraint, pinned to
test-zone-1 and sized for a claim each, in front of six 1-cpu "owner" pods app=web with a zonal spread on app=web (maxSkew 1). Where
the three count, the owners land 0 / 3 / 3 over the zones; where they do not, 2 / 2 / 2."""
import copy
import random

import engine_checks as ec
import operator_cases as oc
import parity
import spread_limit_cases as sl
import spread_operator_cases as so
from karpenter_amd import fixtures as fx

lone_cell, batch_cells = so.lone_cell, so.batch_cells
# 24, 25 over 22 / 23 (every switch but the one under test): what every setting up to 23 does is to decline with reason 43. Pod
# errors and their flags are compared (parity), and queue pops.
SWITCH = ec.Switch("spread", only="spread-filters", auto="auto-filters-spread", base="auto-unschedulable-spread", base_only="spread-unschedulable",
                   reasons=(43,), pops=True)
AUTO, ONLY, BASE, BASE_ONLY = SWITCH.auto, SWITCH.only, SWITCH.base, SWITCH.base_only
check_declined = SWITCH.declined
WEB = {"app": "web"}
ZONES = oc.ZONES
SPOT, ON_DEMAND = "spot", "on-demand"
TEAM = "example.com/team"           # a custom label key: not well known
COUNTED, NOT_COUNTED = {ZONES[1]: 3, ZONES[2]: 3}, {ZONES[0]: 2, ZONES[1]: 2, ZONES[2]: 2}


def check_engine(oracle, lib, prob, want=None):
    """One problem five ways (SWITCH.check; `want`: the oracle's result, computed before)."""
    return SWITCH.check(oracle, lib, prob, want=want)


def check_open(oracle, lib, prob):
    """The other one of a pair when it has NO filter that can say no (policy Ignore): the spread engine solves it under 25 as it
    does under 23, and equals the oracle."""
    want = oracle.solve(prob)
    got = ec.solve(prob, ONLY, lib)
    assert ec.where(got) == ("spread", 0), got["counters"]
    digest = parity.results_digest(got)[0]
    SWITCH.same(got, want, prob)
    assert parity.results_digest(ec.solve(prob, BASE_ONLY, lib))[0] == digest
    return got, want


def owner_uids(prob):
    return {p["uid"] for p in prob["pods"] if p.get("topologySpreadConstraints")}


def owners_by_zone(res, prob):
    """How many of the pods that own a spread constraint sit in each zone, on claims narrowed to it."""
    return so.pods_by_zone(res, owner_uids(prob))


# ---- the building blocks ---------------------------------------------------------------------------------------------------------------

def big(n=3, cpu="7", selector=None, labels=WEB, **kw):
    """n pods app=web without a constraint of their own, pinned to test-zone-1 (and to `selector`)."""
    return [fx.pod(requests={"cpu": cpu}, labels=labels, node_selector=dict({fx.ZONE: ZONES[0]}, **(selector or {})), **kw) for _ in range(n)]


def owners(n=6, cpu="1", selector={fx.CAPACITY_TYPE: ON_DEMAND}, key=fx.ZONE, labels=WEB, affinity_policy=None, taints_policy=None, max_skew=1, **kw):
    """n pods app=web with a spread on `key` over app=web and the nodeSelector `selector`: the owners of the filtered group."""
    return [fx.pod(requests={"cpu": cpu}, labels=labels, node_selector=selector,
                   topology_spread=[fx.spread(key, labels, max_skew=max_skew, affinity_policy=affinity_policy, taints_policy=taints_policy)], **kw) for _ in range(n)]


def problem(pods, pools=None, **kw):
    return fx.problem(fx.fake_instance_types(8), pools or [fx.node_pool("open")], pods, **kw)


# ---- 1: owner only: spread_operator_cases.node_filter_problem() ------------------------------------------------------------------------

# ---- 2: never counted --------------------------------------------------------------------------------------------------------------------

def never_problem(policy=None):
    """The big pods select capacity-type = spot: their class can never match the owners' term capacity-type In [on-demand] — resolved
    at set-up, no slot. Honor (the default): 2 / 2 / 2. nodeAffinityPolicy Ignore: the three count in test-zone-1, 0 / 3 / 3."""
    return problem(big(selector={fx.CAPACITY_TYPE: SPOT}) + owners(affinity_policy=policy))


# ---- 3: dynamic by template --------------------------------------------------------------------------------------------------------------

def by_template_problem(heavy=SPOT):
    """The big pods select on nothing but the zone; the weight-10 pool is capacity-type In [`heavy`], an open pool stands behind it.
    Their claims are the heavy pool's: spot — not counted, 2 / 2 / 2; on-demand — counted, 0 / 3 / 3."""
    pools = [fx.node_pool("heavy", weight=10, requirements=[fx.req(fx.CAPACITY_TYPE, "In", heavy)]), fx.node_pool("open")]
    return problem(big() + owners(), pools)


# ---- 4: undefined against defined --------------------------------------------------------------------------------------------------------

def undefined_problem(policy=None):
    """One open pool that does not define capacity-type at all: the big pods' claims do not define the key, the strict Compatible fails
    the owners' In term although the key is well known: 2 / 2 / 2 (Ignore: 0 / 3 / 3)."""
    return problem(big() + owners(affinity_policy=policy))


# ---- 5: undefined, then concrete ---------------------------------------------------------------------------------------------------------

def then_concrete_problem(joiner=True):
    """As 4 with ONE 3-cpu big pod: its claim does not define capacity-type and the pod is not counted. `joiner`: a 2-cpu pod without
    labels that selects on-demand (and test-zone-1) joins that claim, which is concrete from then on; the two 1200m pods app=web that
    follow it there ARE counted, so test-zone-1 stands at two when the four owners spread: 0 / 2 / 2. Without the joiner the claim
    stays undefined until an owner joins it, the 1200m pods are not counted, and test-zone-1 takes owners."""
    pods = big(1, "3")
    if joiner:
        pods += [fx.pod(requests={"cpu": "2"}, node_selector={fx.ZONE: ZONES[0], fx.CAPACITY_TYPE: ON_DEMAND})]
    pods += big(2, "1200m") + owners(4)
    return problem(pods)


# ---- 6: complement template --------------------------------------------------------------------------------------------------------------

def complement_problem(excluded=SPOT):
    """The heavy pool is capacity-type NotIn [`excluded`]: the big pods' claims keep the pool's own requirement (guard bit set, key
    defined). NotIn [spot] admits on-demand: counted, 0 / 3 / 3. NotIn [on-demand] admits spot alone: not counted, 2 / 2 / 2."""
    pools = [fx.node_pool("heavy", weight=10, requirements=[fx.req(fx.CAPACITY_TYPE, "NotIn", excluded)]), fx.node_pool("open")]
    return problem(big() + owners(), pools)


# ---- 7: custom key -----------------------------------------------------------------------------------------------------------------------

def custom_key_problem(heavy="b"):
    """Only the owners select on example.com/team (= a). Pools team-`heavy` (weight 20), team-a (weight 10), open. The big pods land on
    the heaviest pool: team b — not counted, 2 / 2 / 2; team a — counted, 0 / 3 / 3."""
    pools = [fx.node_pool(f"team-{heavy}-heavy", weight=20, labels={TEAM: heavy}), fx.node_pool("team-a", weight=10, labels={TEAM: "a"}), fx.node_pool("open")]
    return problem(big() + owners(selector={TEAM: "a"}), pools)


# ---- 8: hostname spread with a filter ----------------------------------------------------------------------------------------------------

def hostname_problem(policy=None):
    """One 4-cpu pod app=web on a claim that does not define capacity-type, then three owners with a HOSTNAME spread (maxSkew 1) that
    select on-demand. Honor: the big pod is not counted on its claim, the first owner joins it — three claims. Ignore: the claim
    already holds one counted pod, no owner may join — four claims."""
    return problem(big(1, "4") + owners(3, key=fx.HOSTNAME, affinity_policy=policy))


# ---- 9: two keys in one nodeSelector -----------------------------------------------------------------------------------------------------

def two_keys_problem(heavy="a"):
    """The owners' nodeSelector carries capacity-type = on-demand AND example.com/team = a: one term on two keys. The big pods require
    capacity-type In [on-demand, spot] — the class overlaps the term's field without lying inside it — and do not select on the
    team. Pools team-`heavy` (weight 20), team-a, open: heavy a — counted, 0 / 3 / 3; heavy b — not counted, 2 / 2 / 2."""
    pools = [fx.node_pool(f"team-{heavy}-heavy", weight=20, labels={TEAM: heavy}), fx.node_pool("team-a", weight=10, labels={TEAM: "a"}), fx.node_pool("open")]
    both = [fx.req(fx.CAPACITY_TYPE, "In", ON_DEMAND, SPOT)]
    return problem(big(node_requirements=both) + owners(selector={fx.CAPACITY_TYPE: ON_DEMAND, TEAM: "a"}), pools)


# ---- 10: taint policy --------------------------------------------------------------------------------------------------------------------

TOLERATE = [{"key": "dedicated", "operator": "Exists"}]


def taint_problem(policy="Honor", limits=None, n_big=3, cpu="7"):
    """A tainted weight-10 pool and an open one; the big pods tolerate the taint, the owners (no nodeSelector) do not. Under
    nodeTaintsPolicy Honor the tainted claims are not counted: 2 / 2 / 2. Under the default (Ignore): 0 / 3 / 3."""
    pools = [fx.node_pool("tainted", weight=10, taints=oc.taint("dedicated"), limits=limits), fx.node_pool("open")]
    return problem(big(n_big, cpu, tolerations=TOLERATE) + owners(selector=None, taints_policy=policy), pools)


# ---- 11: limit stage ---------------------------------------------------------------------------------------------------------------------

def limit_stage_problem(policy="Honor"):
    """10 with limits.cpu = 20 on the tainted pool and five 3-cpu big pods: every claim of the pool lists the 8-cpu type, so the third
    one opens under a limit stage — a template id of its own, which must resolve to the tainted template."""
    return taint_problem(policy, limits={"cpu": "20"}, n_big=5, cpu="3")


# ---- 12: existing nodes ------------------------------------------------------------------------------------------------------------------

def node_problem(key=fx.ZONE, capacity_type=SPOT):
    """An empty 8-cpu node in test-zone-1 of capacity type `capacity_type`; three 2-cpu pods app=web without selectors land on it;
    five owners select on-demand and spread over `key`. A spot node does not match the owners' filter: zonal 2 / 2 / 1. An
    on-demand node does, and takes two owners as well: the claims hold 0 / 2 / 1."""
    its = fx.fake_instance_types(8)
    node = fx.state_node("node-a", its[7], ZONES[0], capacity_type, nodepool="open")
    pods = [fx.pod(requests={"cpu": "2"}, labels=WEB) for _ in range(3)] + owners(5, cpu="1", key=key, max_skew=1 if key == fx.ZONE else 2)
    return fx.problem(its, [fx.node_pool("open")], pods, state_nodes=[node])


def tainted_node_problem(policy="Honor"):
    """An empty tainted 8-cpu on-demand node in test-zone-1; three 2-cpu pods app=web that tolerate the taint land on it; the five
    owners do not tolerate it. Honor: the node is not counted."""
    its = fx.fake_instance_types(8)
    node = fx.state_node("node-t", its[7], ZONES[0], ON_DEMAND, nodepool="open", taints=oc.taint("dedicated"))
    pods = [fx.pod(requests={"cpu": "2"}, labels=WEB, tolerations=TOLERATE) for _ in range(3)] + owners(5, selector=None, taints_policy=policy)
    return fx.problem(its, [fx.node_pool("open")], pods, state_nodes=[node])


# ---- 13: set-aside pods ------------------------------------------------------------------------------------------------------------------

def set_aside_problem():
    """2 with a 100-cpu pod (InstanceTypes) and limits.cpu = 28 on the pool: the three big claims take 24 of it, the owners run into
    the limit."""
    prob = never_problem()
    prob["nodePools"][0]["limits"] = {"cpu": "28"}
    prob["pods"] = [fx.pod(requests={"cpu": "100"})] + prob["pods"]
    return prob


# ---- 14: still outside the shape ---------------------------------------------------------------------------------------------------------

def pod_notin_problem():
    """The owners' term is capacity-type NotIn [spot]: a pod requirement that is not positive (reason 4)."""
    pods = big() + [fx.pod(requests={"cpu": "1"}, labels=WEB, node_requirements=[fx.req(fx.CAPACITY_TYPE, "NotIn", SPOT)],
                           topology_spread=[fx.spread(fx.ZONE, WEB)]) for _ in range(6)]
    return problem(pods)


def too_many_slots_problem(n=17):
    """n Deployments app=w<i>, each a 3-cpu pod that selects nothing beside two owners that select on-demand: n groups whose filter is
    decided per claim, one more than there are slots."""
    pods = []
    for i in range(n):
        lab = {"app": f"w{i}"}
        pods += big(1, "3", labels=lab) + owners(2, labels=lab)
    return problem(pods)


def preference_problem():
    prob = undefined_problem()
    prob["pods"].append(fx.pod(requests={"cpu": "1"}, node_preferences=[fx.req(fx.ZONE, "In", ZONES[0])]))
    return prob


# ---- repeated solves ---------------------------------------------------------------------------------------------------------------------

def repeated_solves(lib, prob, engine, n):
    return sl.repeated_solves(lib, prob, engine, n)


# ---- seeded fuzz -------------------------------------------------------------------------------------------------------------------------

# what may take a seed off the spread engine under "auto-filters-spread" (decline.h): 43 beyond the caps (terms, slots, a term on a
# key that is not packed) only; 4 a pod requirement that is not positive; 41 preferences; 5 / 6 keys that do not pack; 44-51 the
# spread engine's other shape limits; 29 limit stages
FUZZ_REASONS = {43, 4, 41, 5, 6, 29} | set(range(44, 52))
CUSTOM = "example.com/tier"


def _selector(rng, owner):
    """A random nodeSelector over {zone, capacity-type, one custom key}. Owners mostly select a capacity type — that is their filter —
    and never the zone they spread over; the other pods are often pinned to a zone, where a zonal group counts them at once."""
    sel = {}
    if not owner and rng.random() < 0.6:
        sel[fx.ZONE] = rng.choice(ZONES[:2])
    if rng.random() < (0.8 if owner else 0.45):
        sel[fx.CAPACITY_TYPE] = ON_DEMAND if owner and rng.random() < 0.7 else rng.choice([ON_DEMAND, SPOT])
    if rng.random() < 0.2:
        sel[CUSTOM] = rng.choice("xy")
    return sel or None


def _pool_reqs(rng):
    reqs, labels = [], {}
    r = rng.random()
    if r < 0.35:
        reqs.append(fx.req(fx.CAPACITY_TYPE, "In", rng.choice([SPOT, ON_DEMAND])))
    elif r < 0.55:
        reqs.append(fx.req(fx.CAPACITY_TYPE, "NotIn", rng.choice([SPOT, ON_DEMAND])))
    if rng.random() < 0.15:
        reqs.append(fx.req(fx.ZONE, "NotIn", ZONES[2]))
    if rng.random() < 0.6:
        labels[CUSTOM] = rng.choice("xy")
    return reqs, labels


def fuzz_problem(seed):
    """2-5 Deployments over one or two label sets. The first owns a zonal (sometimes a hostname) spread on its label, the second carries the
    same label and owns nothing, the others own a spread with probability 0.3, with random policies; all draw a random nodeSelector over {zone, capacity-type, a custom key}; the pods that
    own nothing are larger, so that they stand in front of the owners in the queue. Two or three weighted pools with random In /
    NotIn / nothing on those keys, the heaviest sometimes tainted (the Deployments that own nothing often tolerate it) or limited,
    then an open pool per custom value; sometimes a few existing nodes. The 8-type catalogue."""
    rng = random.Random(99000 + seed)
    its = fx.fake_instance_types(8)
    pools = []
    tainted = rng.random() < 0.35
    for i in range(rng.randint(2, 3)):
        reqs, labels = _pool_reqs(rng)
        pools.append(fx.node_pool(f"pool-{i}", weight=50 - 10 * i, requirements=reqs, labels=labels,
                                  taints=oc.taint("dedicated") if tainted and i == 0 else None,
                                  limits={"cpu": str(rng.choice([12, 20, 30]))} if i == 0 and rng.random() < 0.25 else None))
    pools.append(fx.node_pool("open-x", labels={CUSTOM: "x"}))
    pools.append(fx.node_pool("open-y", labels={CUSTOM: "y"}))
    label_sets = [{"app": "web"}, {"app": "api"}][:1 if rng.random() < 0.6 else 2]
    pods = []
    for i in range(rng.randint(2, 5)):
        lab = label_sets[0] if i < 2 else rng.choice(label_sets)
        owner = i == 0 or (i > 1 and rng.random() < 0.3)   # (the second Deployment carries the first one's label and owns nothing)
        sel = _selector(rng, owner)
        if i == 0:   # the first owner always has a filter on the capacity type ...
            sel = dict(sel or {}, **{fx.CAPACITY_TYPE: (sel or {}).get(fx.CAPACITY_TYPE, ON_DEMAND)})
            first_ct = sel[fx.CAPACITY_TYPE]
        elif i == 1:   # ... and the Deployment beside it is pinned to a zone, mostly without that capacity type
            sel = dict(sel or {}, **{fx.ZONE: (sel or {}).get(fx.ZONE, rng.choice(ZONES[:2]))})
            if sel.get(fx.CAPACITY_TYPE) == first_ct and rng.random() < 0.8:
                del sel[fx.CAPACITY_TYPE]
        kw = {}
        if owner:
            key = fx.ZONE if i == 0 or rng.random() < 0.6 else fx.HOSTNAME
            kw["topology_spread"] = [fx.spread(key, lab, max_skew=1 if rng.random() < 0.85 else 2,
                                               affinity_policy="Ignore" if rng.random() < 0.1 else None,
                                               taints_policy="Honor" if tainted and rng.random() < 0.7 else rng.choice([None, None, "Honor"]))]
            cpu, n = rng.choice(["500m", "1"]), rng.randint(4, 8)
        else:
            if tainted and rng.random() < 0.7:
                kw["tolerations"] = TOLERATE
            cpu, n = rng.choice(["2", "3", "1500m"]), rng.randint(2, 5)
        pods += [fx.pod(requests={"cpu": cpu}, labels=lab, node_selector=sel, **kw) for _ in range(n)]
    nodes = []
    if rng.random() < 0.3:
        for i in range(rng.randint(1, 3)):
            pool = rng.choice(pools)
            nodes.append(fx.state_node(f"node-{i}", its[rng.choice([3, 7])], rng.choice(ZONES[:2]), rng.choice([SPOT, ON_DEMAND]), nodepool=pool["name"],
                                       taints=[dict(t) for t in pool["taints"]], extra_labels=dict(pool["labels"])))
    return fx.problem(its, pools, pods, state_nodes=nodes)


def ignoring(prob):
    """`prob` with both policies of every spread constraint set to Ignore: what the filters are compared against."""
    p = copy.deepcopy(prob)
    for pod in p["pods"]:
        for c in pod.get("topologySpreadConstraints", []):
            c["nodeAffinityPolicy"] = "Ignore"
            c["nodeTaintsPolicy"] = "Ignore"
    return p


def discriminating(oracle, prob, want):
    """A property of the reference alone: its own result — the claim stream, the pods on existing nodes, the pod errors
    (parity.results_digest) — changes when every constraint's two policies are set to Ignore."""
    return parity.results_digest(oracle.solve(ignoring(prob)))[0] != parity.results_digest(want)[0]


FUZZ_SEEDS = list(range(120))
GPU_FUZZ_SEEDS = FUZZ_SEEDS[::4]


def run_fuzz(oracle, lib, seeds):
    """Every seed equals the oracle under "auto-filters-spread", pops included. Returns (seeds on the spread engine with reason 0,
    how many of those are discriminating, {seed: reason} of the rest — reasons of FUZZ_REASONS only)."""
    on_spread, disc, rest = 0, 0, {}
    for seed, prob, want, got, on, reason in ec.fuzz_cases(oracle, lib, ((seed, fuzz_problem(seed)) for seed in seeds), AUTO, pops=True, mode=SWITCH.mode):
        if on == "spread":
            on_spread += 1
            disc += discriminating(oracle, prob, want)
        else:
            assert reason in FUZZ_REASONS, (seed, got["counters"])
            rest[seed] = reason
    print(f"{AUTO}: {on_spread} of {len(seeds)} seeds on the spread engine, {disc} of them discriminating; reasons of the rest {rest}")
    return on_spread, disc, rest
