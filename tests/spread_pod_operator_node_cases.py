"""Topology batches with existing nodes AND pods whose requirements are not In sets — NotIn, Exists, DoesNotExist — for the pod operators
of the spread engine's existing-node path (csrc/topo_nodes.h, "Pod operators beside existing nodes on the spread engine"; engines
"auto-pod-operators-spread-nodes" / "spread-pod-operators-nodes", 35 / 36; tests/test_spread_engine_pod_operators_nodes.py on the
emulation, tests/test_gpu_spread_pod_operators_nodes.py on the device): known shapes, the seeded fuzz and the checks both files run.

What the reference does with such a pod on an existing node is what tests/pod_operator_node_cases.py says of the cursor engine's stage
(a node's label sets are single-valued In sets; a NotIn pod that lands on a node lacking the key writes NotIn onto it). On top of it a
spread group's TopologyNodeFilter (topologynodefilter.go:38-97) is asked about the node that takes a pod: a NotIn / DoesNotExist term
passes a node that lacks the key, an In / Exists term fails it, and on a key the node carries the term reads the node's one value."""
import random

import engine_checks as ec
import kernel_table_cases as kc
import limit_cases as lc
import parity
import pod_operator_cases as pc
import pod_operator_node_cases as nc
import solve_many_cases as mc
import spread_filter_cases as sf
import spread_node_cases as sn
import spread_operator_cases as so
import spread_pod_operator_cases as sp
from karpenter_amd import fixtures as fx

K = nc.K
ZONES, WEB = sp.ZONES, sp.WEB
SPOT, ON_DEMAND = sp.SPOT, sp.ON_DEMAND
# 35, 36 over 32 / 30 (every switch but the one under test): what every setting up to 33 does with such a batch is to decline with the
# reason given per call — 4 for NotIn / Exists pods, 8 for DoesNotExist / In []. The oracle's result has no pod errors.
SWITCH = ec.Switch("spread", only="spread-pod-operators-nodes", auto="auto-pod-operators-spread-nodes", base="auto-pod-operators-nodes", base_only="spread-pod-operators", errors=False)
ONLY, AUTO, BASE, BASE_ONLY = SWITCH.only, SWITCH.auto, SWITCH.base, SWITCH.base_only
# ... and for a problem that leaves pods unschedulable: pod errors required, queue pops compared, no engine-only leg below the switch
UNSCHEDULABLE = SWITCH._replace(errors=True, pops=True, base_only=None)
check_declined = SWITCH.declined
NODE_KEY_DEFINEDNESS = 37
KERNEL, KERNEL_BELOW, KERNEL_NO_NODES = "ksolve_pack_topo_nodes_pn", "ksolve_pack_topo_nodes_p", "ksolve_pack_topo_p"

notin, nodes_of, labels_of, negative_uids, uids = nc.notin, nc.nodes_of, nc.labels_of, nc.negative_uids, nc.uids


def check_engine(oracle, lib, prob, reason=4):
    return SWITCH.check(oracle, lib, prob, reason=reason)


def zone_counts(res, prob, pods):
    """{zone: how many of `pods` (uids) sit there} over existing nodes (by their label) and NodeClaims narrowed to one zone."""
    labels = labels_of(prob)
    out = dict(so.pods_by_zone(res, pods))
    for name, n in nodes_of(res, pods).items():
        out[labels[name][fx.ZONE]] = out.get(labels[name][fx.ZONE], 0) + n
    return out


def _node(name, its, zone, capacity_type=ON_DEMAND, pool="open", size=3, **kw):
    return fx.state_node(name, its[size], zone, capacity_type, pool, **kw)


# ---- 1: a lone zone NotIn pod beside a zonal spread over five nodes ----------------------------------------------------------------

def lone_notin_problem():
    """Five 4-cpu nodes with 3 cpu free, node-0 and node-3 in test-zone-3; nine 1-cpu pods with a zonal spread, two small pods without
    constraints, and ONE 1500m pod with zone NotIn [test-zone-3]: the first in the queue. node-0, the first node in name order, has
    room for it and lies in the zone it excludes."""
    its = fx.fake_instance_types(8)
    nodes = [_node(f"node-{i}", its, z, used={"cpu": "1"}) for i, z in enumerate([ZONES[2], ZONES[0], ZONES[1], ZONES[2], ZONES[0]])]
    pods = so.spread_pods(9) + [fx.pod(requests={"cpu": "500m"}) for _ in range(2)] + [fx.pod(requests={"cpu": "1500m"}, node_requirements=notin(fx.ZONE, ZONES[2]))]
    return fx.problem(its, [fx.node_pool("open")], pods, state_nodes=nodes)


def check_lone_notin(oracle, lib):
    prob = lone_notin_problem()
    got, want = check_engine(oracle, lib, prob)
    labels, lone, owners = labels_of(prob), negative_uids(prob), sp.spread_uids(prob)
    assert len(lone) == 1
    for res in (want, got):
        on = nodes_of(res, lone)
        assert list(on) == ["node-1"] and labels["node-1"][fx.ZONE] == ZONES[0], on        # not node-0, which comes first and has the room
        assert sn.on_nodes(res) >= 10 and "node-0" in nodes_of(res, owners)                # nodes take pods first, node-0 takes spread pods
    assert zone_counts(got, prob, owners) == zone_counts(want, prob, owners) == {z: 3 for z in ZONES}


# ---- 2: the spread owners carry the NotIn themselves: node, claim, node ----------------------------------------------------------------

def own_notin_problem():
    """spread_node_cases.refuse_then_accept_problem with owners that exclude test-zone-3: two nodes in test-zone-1 and one in
    test-zone-3, nine pods with a zonal spread (maxSkew 1) and zone NotIn [test-zone-3]. The skew is taken over the two zones the pods
    support, the nodes' pods counted: a zone-1 node takes a pod, refuses the next (which opens a claim in test-zone-2) and accepts again."""
    its = fx.fake_instance_types(8)
    nodes = [fx.state_node(f"node-{i}", its[5], ZONES[0] if i < 2 else ZONES[2], "on-demand", "default") for i in range(3)]
    lab = {"app": "wave"}
    return fx.problem(its, [fx.node_pool()], sp.spread_pods(9, cpu="500m", labels=lab, reqs=notin(fx.ZONE, ZONES[2])), state_nodes=nodes)


def check_own_notin(oracle, lib):
    prob = own_notin_problem()
    got, want = check_engine(oracle, lib, prob)
    assert sn.node_then_claim_then_node(want, prob)
    owners = sp.spread_uids(prob)
    for res in (want, got):
        assert "node-2" not in nodes_of(res, owners) and nodes_of(res, owners)
        counts = zone_counts(res, prob, owners)
        assert set(counts) == {ZONES[0], ZONES[1]} and abs(counts[ZONES[0]] - counts[ZONES[1]]) <= 1 and sum(counts.values()) == 9, counts


# ---- 3: alive-word block edges ---------------------------------------------------------------------------------------------------------

BLOCK_EDGES = (63, 64, 65, 129)


def block_edge_problem(n_nodes):
    """pod_operator_node_cases.block_edge_problem(n_nodes) as a topology batch: every node but the last lies in test-zone-1, so the last
    node — the last of its 64-node block, or alone in it — is the only one the zone NotIn [test-zone-1] class may take; and twelve
    small pods with a zonal spread. (Without the base problem's test-zone-2 selectors.)"""
    prob = nc.block_edge_problem(n_nodes)
    for n in prob["stateNodes"][:-1]:
        n["labels"][fx.ZONE] = ZONES[0]
    prob["pods"] = [p for p in prob["pods"] if (p.get("nodeSelector") or {}).get(fx.ZONE) != ZONES[1]]   # (the zone-2 selectors would fill the one zone-2 node first)
    for p in prob["pods"]:
        if p["uid"] in uids(prob, "NotIn", fx.ZONE):
            p["requests"]["cpu"] = "350m"   # (ahead of the 300m pods in the queue: the last node still has room when the class arrives)
    prob["pods"] += so.spread_pods(12, cpu="100m", labels={"app": "edge"})
    return prob


def check_block_edge(oracle, lib, n_nodes):
    prob = block_edge_problem(n_nodes)
    got, want = check_engine(oracle, lib, prob)
    last = prob["stateNodes"][-1]["name"]
    assert labels_of(prob)[last][fx.ZONE] == ZONES[1] and (n_nodes - 1) % 64 in (62, 63, 0)
    by_zone = nodes_of(want, uids(prob, "NotIn", fx.ZONE))
    assert list(by_zone) == [last] and nodes_of(got, uids(prob, "NotIn", fx.ZONE)) == by_zone          # the one admissible node, and only it
    by_ct = nodes_of(want, uids(prob, "NotIn", fx.CAPACITY_TYPE))
    assert len(by_ct) > 1 and nodes_of(got, uids(prob, "NotIn", fx.CAPACITY_TYPE)) == by_ct
    assert nodes_of(want, sp.spread_uids(prob)) and want["newNodeClaims"]


# ---- 4: DoesNotExist beside In [x] on one custom key -----------------------------------------------------------------------------------

def dedicated_problem(absent="DoesNotExist"):
    """pod_operator_node_cases.dedicated_problem (every second node carries example.com/dedicated=x; DoesNotExist — or In [] — pods, In
    [x] pods, plain pods) with nine pods that spread over the zones."""
    prob = nc.dedicated_problem(absent)
    prob["pods"] += so.spread_pods(9, cpu="200m")
    return prob


def check_dedicated(oracle, lib):
    for absent in ("DoesNotExist", "In"):
        prob = dedicated_problem(absent)
        got, want = check_engine(oracle, lib, prob, 8)     # (no 37: a DoesNotExist pod changes no later verdict)
        labels = labels_of(prob)
        gone = negative_uids(prob)
        keyed = uids(prob, "In", K) - gone
        for res in (want, got):
            on_gone, on_keyed = nodes_of(res, gone), nodes_of(res, keyed)
            assert on_gone and all(K not in labels[n] for n in on_gone), on_gone           # DoesNotExist / In []: unlabelled nodes only
            assert on_keyed and all(labels[n].get(K) == "x" for n in on_keyed), on_keyed   # In [x]: labelled nodes only
        assert nodes_of(want, sp.spread_uids(prob))


# ---- 5: the topology node filter on a node, four ways ------------------------------------------------------------------------------------

def filter_problem(term, node_labels=None, node_ct=ON_DEMAND, selector=None):
    """spread_filter_cases.node_problem's build: an empty 8-cpu node in test-zone-1 (capacity type `node_ct`, `node_labels` on top); three
    2-cpu pods app=web that select `selector` (nothing: their class does not select on the term's key) land on it; five owners app=web
    spread over the zones and carry the node-affinity term `term` — the one term of their group's node filter; and one pod with zone
    NotIn [test-zone-3], so that every variant is a batch with a negative pod. The pool defines example.com/dedicated (In [x, y])."""
    its = fx.fake_instance_types(8)
    node = fx.state_node("node-a", its[7], ZONES[0], node_ct, nodepool="open", extra_labels=node_labels)
    pods = [fx.pod(requests={"cpu": "2"}, labels=WEB, node_selector=selector) for _ in range(3)] + sp.spread_pods(5, reqs=term)
    pods.append(fx.pod(requests={"cpu": "300m"}, node_requirements=notin(fx.ZONE, ZONES[2])))
    return fx.problem(its, [fx.node_pool("open", requirements=[fx.req(K, "In", "x", "y")])], pods, state_nodes=[node])


# (name, problem, is the node's trio counted by the owners' group?)
def filter_cases():
    return [
        ("a NotIn term against a node that lacks the key", filter_problem(notin(K, "x")), True),
        ("an In term against the same node", filter_problem([fx.req(K, "In", "y")]), False),
        ("a NotIn term, the class selects a value inside the set", filter_problem(notin(fx.CAPACITY_TYPE, SPOT), node_ct=SPOT, selector={fx.CAPACITY_TYPE: SPOT}), False),
        ("... and a value outside it", filter_problem(notin(fx.CAPACITY_TYPE, SPOT), node_ct=ON_DEMAND, selector={fx.CAPACITY_TYPE: ON_DEMAND}), True),
        ("a NotIn term, the class does not select on the key, the node's label inside the set", filter_problem(notin(fx.CAPACITY_TYPE, SPOT), node_ct=SPOT), False),
        ("... and outside it", filter_problem(notin(fx.CAPACITY_TYPE, SPOT), node_ct=ON_DEMAND), True),
    ]


def trio(prob):
    return {p["uid"] for p in prob["pods"] if p["labels"] == WEB and not p.get("topologySpreadConstraints")}


def check_filter_case(oracle, lib, case):
    """The trio lands on the node (test-zone-1). Counted: the owners see three pods there and fill the other zones first — at most one
    of the five in test-zone-1. Not counted: the owners spread as if the zone were empty — two of the five in test-zone-1."""
    _, prob, counted = case
    got, want = check_engine(oracle, lib, prob)
    owners = sp.spread_uids(prob)
    for res in (want, got):
        assert nodes_of(res, trio(prob)) == {"node-a": 3}
        z1 = zone_counts(res, prob, owners).get(ZONES[0], 0)
        assert (z1 <= 1) if counted else (z1 == 2), (counted, zone_counts(res, prob, owners))


# ---- 6: reason 37: an In class, an In term that owners carry --------------------------------------------------------------------------------------------------------------

def definedness_class_problem(every_node_keyed=False):
    """The class form: pod_operator_node_cases.key_definedness_problem (NotIn [b] pods and In [a] pods on example.com/dedicated, node-0
    lacks the key) with six pods that spread over the zones."""
    prob = nc.key_definedness_problem(every_node_keyed=every_node_keyed)
    prob["pods"] += so.spread_pods(6, cpu="200m")
    return prob


def definedness_term_problem(every_node_keyed=False):
    """The In [a] on example.com/dedicated is the node-affinity term of six spread owners — a term of their group's node filter, which
    reads the node's label row: behind a NotIn [b] pod node-0, which lacks the key, would pass it where it failed. The term is the
    owners' class requirement too, so in this batch the CLASS half of the test fires as well: no batch shows the term half alone
    (test_definedness_check_directly asks the function for it)."""
    prob = nc.key_definedness_problem(every_node_keyed=every_node_keyed)
    prob["pods"] = [p for p in prob["pods"] if p["uid"] in uids(prob, "NotIn", K)] + sp.spread_pods(6, cpu="500m", reqs=[fx.req(K, "In", "a")])
    return prob


def check_key_definedness(oracle, lib):
    for make in (definedness_class_problem, definedness_term_problem):
        prob = make()
        assert K not in labels_of(prob)["node-0"] and uids(prob, "NotIn", K) and uids(prob, "In", K)
        auto = check_declined(oracle, lib, prob, NODE_KEY_DEFINEDNESS)           # 35: falls back with 37 and equals the oracle; 36: refuses and names 37
        assert nodes_of(auto, uids(prob, "NotIn", K)).get("node-0")              # a NotIn pod did land on the node that lacks the key
        assert ec.where(ec.solve(prob, BASE, lib)) == ("general", 4)             # every setting below keeps its reason
        twin = make(every_node_keyed=True)                                       # every node carries the key: nothing is ever added to a node
        got, want = check_engine(oracle, lib, twin)
        assert nodes_of(want, uids(twin, "NotIn", K)) and nodes_of(want, uids(twin, "In", K))


# ---- 7: unschedulable negative pods beside nodes ---------------------------------------------------------------------------------------------

def no_zone_problem():
    """2 with two spread pods app=api whose NotIn excludes every zone: no node and no NodePool takes them (Topology, 3)."""
    prob = own_notin_problem()
    prob["pods"] += sp.spread_pods(2, cpu="500m", labels={"app": "api"}, reqs=notin(fx.ZONE, *ZONES))
    return prob


def check_no_zone(oracle, lib):
    prob = no_zone_problem()
    got, want = UNSCHEDULABLE.check(oracle, lib, prob, reason=4)
    assert len(want["podErrors"]) == 2 and got["podErrors"] == want["podErrors"] and nodes_of(want, negative_uids(prob))


# ---- 8, 9, 10: a binding limit, DaemonSet overhead, a complement NodePool ------------------------------------------------------------------

def limit_problem():
    prob = nc.limit_problem()
    prob["pods"] += so.spread_pods(12, cpu="500m")
    return prob


def check_limit(oracle, lib):
    prob = limit_problem()
    got, want = check_engine(oracle, lib, prob)
    assert nodes_of(want, negative_uids(prob)) and lc.stages(got)[0] >= 1 and {"capped", "open"} <= set(lc.pool_of(want))


def daemonset_problem(kind="b"):
    prob = nc.daemonset_problem(kind)
    prob["pods"] += so.spread_pods(9, cpu="500m")
    return prob


def check_daemonsets(oracle, lib):
    for kind in ("a", "b", "c"):
        prob = daemonset_problem(kind)
        got, want = check_engine(oracle, lib, prob)
        assert nodes_of(want, negative_uids(prob)) and want["newNodeClaims"]


def complement_pool_problem():
    """spread_operator_cases' pool zone NotIn [test-zone-1] in front of an open one, nodes of both, owners that exclude test-zone-3
    themselves and pods that exclude spot capacity."""
    its = fx.fake_instance_types(8)
    pools = [pc.oc.notin_zone_pool(), fx.node_pool("open")]
    nodes = [_node(f"node-{i}", its, ZONES[i % 3], pool="open", used={"cpu": "1500m", "pods": "2"}) for i in range(6)]
    pods = sp.spread_pods(9, cpu="700m", reqs=notin(fx.ZONE, ZONES[2])) + [fx.pod(requests={"cpu": "300m"}, node_requirements=notin(fx.CAPACITY_TYPE, SPOT)) for _ in range(6)]
    pods += [fx.pod(requests={"cpu": "3"}) for _ in range(4)]
    return fx.problem(its, pools, pods, state_nodes=nodes)


def check_complement_pool(oracle, lib):
    prob = complement_pool_problem()
    got, want = check_engine(oracle, lib, prob)
    assert nodes_of(want, negative_uids(prob)) and want["newNodeClaims"]


# ---- 11: old settings unchanged ------------------------------------------------------------------------------------------------------------

def check_settings_below(oracle, lib):
    """The problems above under 29, 30 and 32: reason 4 (8), the oracle's result — and the digest every other setting gives."""
    for prob, reason in ((lone_notin_problem(), 4), (own_notin_problem(), 4), (dedicated_problem(), 8), (filter_cases()[0][1], 4)):
        digest = parity.results_digest(ec.solve(prob, AUTO, lib))[0]
        for setting in ("auto-pod-operators-spread", "auto-pod-operators-nodes"):
            res = ec.solve(prob, setting, lib)
            assert ec.where(res) == ("general", reason) and parity.results_digest(res)[0] == digest, (setting, res["counters"])
        ec.refusal_says(ec.refusal(prob, "spread-pod-operators", lib), "spread", reason)


def positive_with_nodes():
    return [sn.block_edge_problem(65), sn.refuse_then_accept_problem(), sf.node_problem(), sf.tainted_node_problem(), so.nodes_mix_problem()]


def check_positive_batches(oracle, names_lib):
    """Positive batches with nodes under 35 / 36: the engine, reason, digest and kernel of 32 / 30; a batch without nodes under 35
    launches ksolve_pack_topo_p; a negative batch with nodes launches ksolve_pack_topo_nodes_pn, and still _nodes_p + reason 4 under 30."""
    for prob in positive_with_nodes():
        for new, old in ((AUTO, BASE), (ONLY, BASE_ONLY)):
            a, ka = kc.solve(prob, old, names_lib)
            b, kb = kc.solve(prob, new, names_lib)
            assert ec.where(a) == ec.where(b) == ("spread", 0) and parity.results_digest(a)[0] == parity.results_digest(b)[0]
            assert ka == kb and kb[-1] == KERNEL_BELOW, (new, ka, kb)
    bare, names = kc.solve(sp.own_notin_problem(), AUTO, names_lib)
    assert ec.where(bare) == ("spread", 0) and names[-1] == KERNEL_NO_NODES, names
    for setting in (AUTO, ONLY):
        res, names = kc.solve(lone_notin_problem(), setting, names_lib)
        assert ec.where(res) == ("spread", 0) and names[-1] == KERNEL, names
    res, names = kc.solve(lone_notin_problem(), BASE, names_lib)
    assert ec.where(res) == ("general", 4) and KERNEL_BELOW in names, names


# ---- 12, 13: repeated solves, SolveMany ------------------------------------------------------------------------------------------------------

def check_repeated(oracle, lib, n):
    prob = own_notin_problem()
    want = oracle.solve(prob)
    digests, last = ec.digests_of_repeated_solves(lib, prob, AUTO, n, "spread")
    assert len(digests) == 1
    SWITCH.same(last, want, prob)


def check_solve_many(oracle, lib):
    """One SolveMany: a member of this shape under 35, a positive spread member and a cursor member — each the lone solve's."""
    members = [(lone_notin_problem(), AUTO), (sf.by_template_problem(), AUTO), (fx.config1(pods=300, n_types=144, seed=7), AUTO)]
    want = [mc.lone_cell(lib, p, s) for p, s in members]
    scheds = mc.open_members(members, lib)
    try:
        results, _ = mc.many(scheds)
    finally:
        mc.close_all(scheds)
    got = [mc.cell_of(r) for r in results]
    mc.assert_cells(got, want, list(range(len(members))))
    assert [(c["engine"], c["engineFallbackReason"]) for c in got] == [("spread", 0), ("spread", 0), ("cursor", 0)], got
    mc.same_as_oracle(oracle, members, results)


# ---- seeded fuzz -------------------------------------------------------------------------------------------------------------------------------

FUZZ_SEEDS = sp.FUZZ_SEEDS
GPU_FUZZ_SEEDS = FUZZ_SEEDS[::4]
# what may take a seed off the spread engine under "auto-pod-operators-spread-nodes" (csrc/decline.h): the by-design declines of the pod
# operators (9-12), the nodes' own (35-37), 43 beyond the filter slots' caps, 50 a sixteenth domain
FUZZ_REASONS = {9, 10, 11, 12, 35, 36, 37, 43, 50}


def fuzz_problem(seed):
    """spread_pod_operator_cases.fuzz_problem(seed) with 5, 64 or 130 nodes of its own catalogue and NodePools."""
    rng = random.Random(93000 + seed)
    return fx.with_existing_nodes(sp.fuzz_problem(seed), rng.choice([5, 64, 130]), seed=seed, small=True)


def run_fuzz(oracle, lib, seeds):
    """Every seed equals the oracle under "auto-pod-operators-spread-nodes", pod errors included. Returns (seeds on the spread engine
    with reason 0, {seed: reason} of the rest, seeds in which the ORACLE places a pod of a negative class on a node, seeds whose oracle
    result leaves a pod error)."""
    on_spread, rest, negative_on_nodes, errors = 0, {}, 0, 0
    for seed, prob, want, got, on, reason in ec.fuzz_cases(oracle, lib, ((seed, fuzz_problem(seed)) for seed in seeds), AUTO, pops=False, mode=SWITCH.mode):
        negative_on_nodes += bool(nodes_of(want, negative_uids(prob)))
        errors += bool(want["podErrors"])
        if on == "spread":
            on_spread += 1
        else:
            assert reason in FUZZ_REASONS, (seed, got["counters"])
            rest[seed] = reason
    print(f"{AUTO}: {on_spread} of {len(seeds)} seeds on the spread engine; reasons of the rest {rest}; the oracle puts a negative pod on a node in "
          f"{negative_on_nodes} seeds; {errors} seeds leave a pod error")
    return on_spread, rest, negative_on_nodes, errors
