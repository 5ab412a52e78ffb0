"""Problems with existing nodes AND pods whose requirements are not In sets — NotIn, Exists, DoesNotExist — for the pod operators of
the cursor engine's existing-node stage (csrc/node_stage.h, "Pod operators beside existing nodes"; engines "auto-pod-operators-nodes" /
"cursor-pod-operators-nodes", 32 / 33; tests/test_cursor_engine_pod_operators_nodes.py on the emulation,
tests/test_gpu_cursor_pod_operators_nodes.py on the device): known shapes, the seeded fuzz and the comparison helpers.

What the reference does with such a pod on an existing node (existingnode.go:100-106, 172-176; requirements.go:133-140, 181-197,
254-274): a node's label sets are single-valued In sets. On a key the node defines as In {a} whatever is compatible leaves In {a}: In S
passes iff a is in S, NotIn S iff it is not, Exists passes, DoesNotExist fails. On a key the node lacks In / Exists fail and NotIn /
DoesNotExist pass — and are written onto the node: behind a NotIn pod a later In / Exists pod passes where it failed before. That one
shape (a key some node lacks with a NotIn class and an In / Exists class on it) is reason 37; everything else is static."""
import random

import engine_checks as ec
import existing_node_cases as en
import kernel_table_cases as kc
import limit_cases as lc
import operator_cases as oc
import parity
import pod_operator_cases as pc
import solve_many_cases as mc
from karpenter_amd import fixtures as fx

K = "example.com/dedicated"
# 32, 33 over 29 / 27 (every switch but the one under test): what every setting up to 30 does with such a batch is to decline from the
# stage with the reason given per call — 4 for NotIn / Exists pods, 8 for DoesNotExist / In []. The oracle's result has no pod errors.
SWITCH = ec.Switch("cursor", only="cursor-pod-operators-nodes", auto="auto-pod-operators-nodes", base="auto-pod-operators-spread", base_only="cursor-pod-operators", errors=False)
ENGINE, AUTO, BASE, BASE_CURSOR = SWITCH.only, SWITCH.auto, SWITCH.base, SWITCH.base_only
# ... and for a problem that leaves pods unschedulable: pod errors required, queue pops compared, no engine-only leg below the switch
UNSCHEDULABLE = SWITCH._replace(errors=True, pops=True, base_only=None)
check_declined = SWITCH.declined
NODE_KEY_DEFINEDNESS = 37

notin, pod_reqs, on_nodes = pc.notin, pc.pod_reqs, en.on_nodes


def check_engine(oracle, lib, prob, reason=4):
    return SWITCH.check(oracle, lib, prob, reason=reason)


def check_unschedulable(oracle, lib, prob, reason=4):
    return UNSCHEDULABLE.check(oracle, lib, prob, reason=reason)


def uids(prob, operator, key=None):
    """The pods with a requirement of `operator` (on `key`); operator None: the pods without any requirement."""
    if operator is None:
        return {p["uid"] for p in prob["pods"] if not pod_reqs(p) and not p.get("nodeSelector")}
    return {p["uid"] for p in prob["pods"] if any(r["operator"] == operator and key in (None, r["key"]) for r in pod_reqs(p))}


def nodes_of(res, pods):
    """{node name: how many of `pods` (uids) the result puts on it}, nodes without any left out."""
    out = {e["name"]: len(pods & set(e["pods"])) for e in res.get("existingNodes", [])}
    return {n: c for n, c in out.items() if c}


def labels_of(prob):
    return {n["name"]: n["labels"] for n in prob["stateNodes"]}


# ---- 1: block edges ------------------------------------------------------------------------------------------------------------------

BLOCK_EDGES = (63, 64, 65, 129)


def block_edge_problem(n_nodes, block0_zone1=False):
    """en.block_edge_problem(n_nodes) plus two negative pod classes, zone NotIn [test-zone-1] and capacity-type NotIn [spot], whose
    pods are small and come last in the queue: they take what the positive pods left, node after node through every block and beyond
    the last node. The last node lies in test-zone-2 here and has 250m more: the positive pods leave it room for one pod of the zone
    class and two of the other, whatever n_nodes is (a last block of one node included).
    block0_zone1: the first 64 nodes all lie in test-zone-1 — the zone class's row of block 0 is all dead, and its cursor must jump the
    block on the first pod."""
    prob = en.block_edge_problem(n_nodes)
    last = prob["stateNodes"][-1]
    last["labels"][fx.ZONE] = "test-zone-2"
    last["available"]["cpu"] = f"{int(last['available']['cpu'][:-1]) + 250 * 10**6}n"
    if block0_zone1:
        for n in prob["stateNodes"][:64]:
            n["labels"][fx.ZONE] = "test-zone-1"
    prob["pods"] += [fx.pod(requests={"cpu": "150m"}, node_requirements=notin(fx.ZONE, "test-zone-1")) for _ in range(n_nodes)]
    prob["pods"] += [fx.pod(requests={"cpu": "50m"}, node_requirements=notin(fx.CAPACITY_TYPE, "spot")) for _ in range(3 * n_nodes)]
    return prob


def last_block(prob):
    """The names of the nodes of the last 64-node block."""
    names = [n["name"] for n in prob["stateNodes"]]
    return set(names[(len(names) - 1) // 64 * 64:])


# ---- 2: one custom key, three operators ----------------------------------------------------------------------------------------------

def dedicated_problem(absent="DoesNotExist", n_nodes=10):
    """Every second node carries example.com/dedicated=x. DoesNotExist pods (or, `absent` = "In": In [] pods) go to the unlabelled nodes
    only, In [x] pods to the labelled ones only, plain pods anywhere. Two NodePools define the key (In [x]; DoesNotExist) so that the
    loop behind the stage takes the pods the nodes leave: no pool leaves the key undefined (reason 9)."""
    its = fx.fake_instance_types(8)
    pools = [fx.node_pool("dedicated", weight=10, requirements=[fx.req(K, "In", "x")]), fx.node_pool("shared", requirements=[fx.req(K, "DoesNotExist")])]
    nodes = [fx.state_node(f"node-{i:02d}", its[3], f"test-zone-{1 + i % 3}", "on-demand", "dedicated" if i % 2 else "shared", used={"cpu": "1", "pods": "1"},
                           extra_labels={K: "x"} if i % 2 else None) for i in range(n_nodes)]
    gone = [fx.req(K, "DoesNotExist")] if absent == "DoesNotExist" else [fx.req(K, "In")]
    pods = [fx.pod(requests={"cpu": c}, node_requirements=gone) for c in ["900m", "600m"] * n_nodes]
    pods += [fx.pod(requests={"cpu": c}, node_requirements=[fx.req(K, "In", "x")]) for c in ["800m", "500m"] * n_nodes]
    pods += [fx.pod(requests={"cpu": "300m"}) for _ in range(2 * n_nodes)]
    return fx.problem(its, pools, pods, state_nodes=nodes)


# ---- 3: NotIn on a key no node carries and no positive class uses ----------------------------------------------------------------------

def unused_key_problem():
    """NotIn [y] on example.com/dedicated: no node carries the key and no class selects on it with In / Exists, so a node that gained
    NotIn [y] answers every later pod as before. The pool defines the key (NotIn [z]): no reason 9."""
    its = fx.fake_instance_types(8)
    pool = fx.node_pool("open", requirements=[fx.req(K, "NotIn", "z")])
    nodes = [fx.state_node(f"node-{i}", its[3], f"test-zone-{1 + i % 2}", "on-demand", "open", used={"cpu": "1"}) for i in range(6)]
    pods = [fx.pod(requests={"cpu": c}, node_requirements=notin(K, "y")) for c in ["700m", "400m"] * 8]
    pods += [fx.pod(requests={"cpu": "500m"}, node_selector={fx.ZONE: "test-zone-2"}) for _ in range(6)] + [fx.pod(requests={"cpu": "50m"}) for _ in range(6)]
    return fx.problem(its, [pool], pods, state_nodes=nodes)


# ---- 4: Exists ---------------------------------------------------------------------------------------------------------------------

def exists_problem():
    """example.com/dedicated Exists: the pool defines the key (In [x, y]: the loop's reason 12 does not apply, and neither does 9) and
    every second node carries it. Exists pods land on labelled nodes only."""
    its = fx.fake_instance_types(8)
    pool = fx.node_pool("keyed", requirements=[fx.req(K, "In", "x", "y")])
    nodes = [fx.state_node(f"node-{i}", its[3], "test-zone-1", "on-demand", "keyed", used={"cpu": "1"}, extra_labels={K: "xy"[i % 4 // 2]} if i % 2 else None) for i in range(8)]
    pods = [fx.pod(requests={"cpu": c}, node_requirements=[fx.req(K, "Exists")]) for c in ["900m", "500m"] * 8]
    pods += [fx.pod(requests={"cpu": "400m"}, node_selector={K: "y"}) for _ in range(4)]
    return fx.problem(its, [pool], pods, state_nodes=nodes)


# ---- 5: reason 37 --------------------------------------------------------------------------------------------------------------------

def key_definedness_problem(every_node_keyed=False, positive="In", keyed_first=False):
    """NotIn [b] pods (the larger: first in the queue) and In [a] pods on example.com/dedicated; node-0 lacks the key, node-1 carries
    a. The oracle puts a NotIn pod on node-0 — which then holds NotIn [b] — and In [a] pods on it afterwards, where they failed
    before: the rows are not static, reason 37. The pool defines the key, so the loop's reason 9 does not come first.
    every_node_keyed: node-0 carries a too — nothing is added to any node, and the batch stays on the cursor engine.
    positive = "Exists": the second kind of pod requires Exists in place of In [a]. keyed_first: the two nodes swap their names (the scheduler
    visits nodes in name order), so that the node that lacks the key — node-1 then — is not the first one."""
    its = fx.fake_instance_types(8)
    pool = fx.node_pool("keyed", requirements=[fx.req(K, "In", "a", "b", "c")])
    large, small = ("node-1", "node-0") if keyed_first else ("node-0", "node-1")
    nodes = [fx.state_node(large, its[7], "test-zone-1", "on-demand", "keyed", extra_labels={K: "a"} if every_node_keyed else None),
             fx.state_node(small, its[1], "test-zone-1", "on-demand", "keyed", used={"cpu": "1"}, extra_labels={K: "a"})]
    pods = [fx.pod(requests={"cpu": "1500m"}, node_requirements=notin(K, "b")) for _ in range(2)]
    pods += [fx.pod(requests={"cpu": "500m"}, node_requirements=[fx.req(K, "In", "a") if positive == "In" else fx.req(K, "Exists")]) for _ in range(6)]
    return fx.problem(its, [pool], pods, state_nodes=sorted(nodes, key=lambda n: n["name"]))


# ---- 6: the switches beside it -----------------------------------------------------------------------------------------------------

def _negatives(n=8):
    return [fx.pod(requests={"cpu": c}, node_requirements=notin(fx.ZONE, "test-zone-1")) for c in ["1100m", "300m"] * n] + \
           [fx.pod(requests={"cpu": "200m"}, node_requirements=notin(fx.CAPACITY_TYPE, "spot")) for _ in range(n)]


def _some_nodes(its, pool, n=6):
    return [fx.state_node(f"node-{i}", its[3], f"test-zone-{1 + i % 3}", "on-demand", pool, used={"cpu": "1500m", "pods": "2"}) for i in range(n)]


def limit_problem():
    """A NodePool limit that binds (limits.cpu = 44 on the preferred pool, 24 of them held by its nodes: later claims open under a limit stage or on the open pool)."""
    its = fx.fake_instance_types(8)
    pools = [fx.node_pool("capped", weight=10, limits={"cpu": "44"}), fx.node_pool("open")]
    pods = _negatives() + [fx.pod(requests={"cpu": "3"}) for _ in range(10)]
    return fx.problem(its, pools, pods, state_nodes=_some_nodes(its, "capped"))


def complement_pool_problem():
    """oc.kwok_problem — pool `big`: instance-cpu Gt 3 and instance-family NotIn [c], which only the view's plain_ops lets onto the
    cursor engine — with nodes and with pods that exclude a zone or spot capacity."""
    prob = fx.with_existing_nodes(oc.kwok_problem(), 8, seed=4, fill=(0.3, 0.6), small=True)
    zones = sorted({n["labels"][fx.ZONE] for n in prob["stateNodes"]})
    prob["pods"] += [fx.pod(requests={"cpu": c, "memory": "128Mi"}, node_requirements=notin(fx.ZONE, zones[0])) for c in ["700m", "200m"] * 6]
    prob["pods"] += [fx.pod(requests={"cpu": "150m", "memory": "128Mi"}, node_requirements=notin(fx.CAPACITY_TYPE, "spot")) for _ in range(6)]
    return prob


def daemonset_problem(kind="b"):
    its = fx.fake_instance_types(8)
    pods = _negatives() + [fx.pod(requests={"cpu": "2"}) for _ in range(6)]
    return fx.with_daemonsets(fx.problem(its, [fx.node_pool("open")], pods, state_nodes=_some_nodes(its, "open")), kind)


def no_zone_problem():
    """Two pods whose NotIn excludes every zone: no node and no NodePool takes them; they keep the reference's error."""
    its = fx.fake_instance_types(8)
    pods = _negatives() + [fx.pod(requests={"cpu": "2"}) for _ in range(4)] + [fx.pod(requests={"cpu": "100m"}, node_requirements=notin(fx.ZONE, *pc.ZONES)) for _ in range(2)]
    return fx.problem(its, [fx.node_pool("open")], pods, state_nodes=_some_nodes(its, "open"))


# ---- 7: the loop's declines, with nodes --------------------------------------------------------------------------------------------

def loop_declines():
    """(reason, problem): pc's by-design declines 9-12 with nodes added — nodes that carry every key the pods name, so that the stage
    itself has nothing to say (no 37) and the loop's setup names its reason."""
    return [(9, _with_nodes(pc.definedness_problem(), {pc.K: "a"})), (10, _with_nodes(pc.dne_mixed_problem(), {fx.FAKE_EXOTIC_LABEL: "optional"})),
            (11, _with_nodes(pc.notin_bounds_problem(), {})), (12, _with_nodes(pc.exists_undefined_problem(), {}))]


def _with_nodes(prob, extra):
    its = prob["instanceTypes"]
    prob["stateNodes"] = [fx.state_node(f"node-{i}", its[7], f"test-zone-{1 + i % 2}", "on-demand", prob["nodePools"][-1]["name"], used={"cpu": "6"}, extra_labels=extra) for i in range(3)]
    return prob


# ---- 8: both memory variants -------------------------------------------------------------------------------------------------------

def variant_problem(n_nodes):
    """test_cursor_engine_nodes.test_lds_and_hbm_variants' problem with negative pods: 3,072 small nodes keep `remaining` in LDS, 3,073
    do not."""
    base = fx.config2(pods=5000, n_types=144, seed=11)
    prob = fx.with_existing_nodes(base, n_nodes, seed=2, fill=(0.93, 1.0), small=True)
    zones = sorted({n["labels"][fx.ZONE] for n in prob["stateNodes"]})
    prob["pods"] = list(prob["pods"]) + [fx.pod(requests={"cpu": "100m", "memory": "100Mi"}, node_requirements=notin(fx.ZONE, zones[0])) for _ in range(40)] + \
        [fx.pod(requests={"cpu": "100m", "memory": "128Mi"}, node_requirements=notin(fx.CAPACITY_TYPE, "spot")) for _ in range(40)]
    return prob


# ---- 9, 10: repeated solves, SolveMany ---------------------------------------------------------------------------------------------

def repeated_problem():
    return fuzz_problem(10)   # (130 nodes; the oracle puts 36 negative pods on nodes and opens four claims)


# ---- seeded fuzz ---------------------------------------------------------------------------------------------------------------------

FUZZ_SEEDS = pc.FUZZ_SEEDS
GPU_FUZZ_SEEDS = FUZZ_SEEDS[3::4]   # every fourth seed; of the seeds 0, 4, ... only five carry a negative pod at all (pc.fuzz_problem turns a shape one time in three)
FUZZ_REASONS = pc.FUZZ_REASONS | {NODE_KEY_DEFINEDNESS}


def fuzz_problem(seed):
    rng = random.Random(91000 + seed)
    return fx.with_existing_nodes(pc.fuzz_problem(seed), rng.choice([5, 64, 130]), seed=seed, small=True)


def negative_uids(prob):
    return {p["uid"] for p in prob["pods"] if any(r["operator"] != "In" or not r["values"] for r in pod_reqs(p))}


def run_fuzz(oracle, lib, seeds):
    """Every seed equals the oracle under "auto-pod-operators-nodes". Returns (seeds that ended on the cursor engine with reason 0,
    {seed: reason} of the rest, seeds in which the ORACLE places a pod of a negative class on a node)."""
    on_cursor, rest, negative_on_nodes = 0, {}, 0
    for seed, prob, want, got, on, reason in ec.fuzz_cases(oracle, lib, ((seed, fuzz_problem(seed)) for seed in seeds), AUTO, pops=False, mode=SWITCH.mode):
        negative_on_nodes += bool(nodes_of(want, negative_uids(prob)))
        if on == "cursor":
            on_cursor += 1
        else:
            assert reason in FUZZ_REASONS, (seed, got["counters"])
            rest[seed] = reason
    print(f"auto-pod-operators-nodes kept {on_cursor} of {len(seeds)} seeds on the cursor engine; reasons of the rest {rest}; "
          f"the oracle puts a negative pod on a node in {negative_on_nodes} seeds")
    return on_cursor, rest, negative_on_nodes


# ---- the checks both test files run (lib: the host emulation, or None for the product library) ---------------------------------------

def check_block_edge(oracle, lib, n_nodes, block0_zone1):
    prob = block_edge_problem(n_nodes, block0_zone1)
    got, want = check_engine(oracle, lib, prob)
    assert got["counters"]["phaseCycles"][19] == 1
    labels, last = labels_of(prob), last_block(prob)
    by_zone, by_ct = nodes_of(want, uids(prob, "NotIn", fx.ZONE)), nodes_of(want, uids(prob, "NotIn", fx.CAPACITY_TYPE))
    assert set(by_zone) & last and set(by_ct) & last, (by_zone, by_ct)              # negative pods sit on nodes of the last block ...
    assert not [n for n in by_zone if labels[n][fx.ZONE] == "test-zone-1"]          # ... and none of the zone class on a zone-1 node
    assert sum(by_zone.values()) < n_nodes and want["newNodeClaims"]                # ... and the nodes ran out before the class did
    if block0_zone1:
        names = [n["name"] for n in prob["stateNodes"]]
        assert by_zone and not set(by_zone) & set(names[:64]) and all(labels[n][fx.ZONE] == "test-zone-1" for n in names[:64])
    assert nodes_of(got, uids(prob, "NotIn", fx.ZONE)) == by_zone and nodes_of(got, uids(prob, "NotIn", fx.CAPACITY_TYPE)) == by_ct


def check_dedicated(oracle, lib):
    for absent in ("DoesNotExist", "In"):
        prob = dedicated_problem(absent)
        got, want = check_engine(oracle, lib, prob, 8)     # (no 37: the batch stays on the cursor engine)
        labels = labels_of(prob)
        gone = negative_uids(prob)
        keyed = uids(prob, "In", K) - gone
        for res in (want, got):
            on_gone, on_keyed = nodes_of(res, gone), nodes_of(res, keyed)
            assert on_gone and all(K not in labels[n] for n in on_gone), on_gone        # DoesNotExist / In []: unlabelled nodes only
            assert on_keyed and all(labels[n].get(K) == "x" for n in on_keyed), on_keyed   # In [x]: labelled nodes only
        both = nodes_of(want, uids(prob, None))
        assert any(K in labels[n] for n in both) and any(K not in labels[n] for n in both)   # plain pods: either kind


def check_unused_key(oracle, lib):
    prob = unused_key_problem()
    got, want = check_engine(oracle, lib, prob)
    assert not any(K in n["labels"] for n in prob["stateNodes"]) and not uids(prob, "In", K) and not uids(prob, "Exists", K)
    assert sum(nodes_of(want, uids(prob, "NotIn", K)).values()) >= 8 and nodes_of(got, uids(prob, "NotIn", K)) == nodes_of(want, uids(prob, "NotIn", K))
    # ... and pods without the requirement joined nodes that NotIn pods had joined before
    assert set(nodes_of(want, uids(prob, None))) & set(nodes_of(want, uids(prob, "NotIn", K)))


def check_exists(oracle, lib):
    prob = exists_problem()
    got, want = check_engine(oracle, lib, prob)
    labels = labels_of(prob)
    on = nodes_of(want, uids(prob, "Exists", K))
    assert on and all(K in labels[n] for n in on) and {labels[n][K] for n in on} == {"x", "y"}, on
    assert any(K not in lb for lb in labels.values()) and nodes_of(got, uids(prob, "Exists", K)) == on


def check_key_definedness(oracle, lib):
    for positive, keyed_first in (("In", False), ("Exists", False), ("In", True)):
        prob = key_definedness_problem(positive=positive, keyed_first=keyed_first)
        want = oracle.solve(prob)
        lacking = "node-1" if keyed_first else "node-0"
        assert K not in labels_of(prob)[lacking] and [n["name"] for n in prob["stateNodes"]] == ["node-0", "node-1"]
        order = next(e["pods"] for e in want["existingNodes"] if e["name"] == lacking)
        first_notin = min(order.index(u) for u in uids(prob, "NotIn", K) if u in order)
        after = [u for u in order[first_notin + 1:] if u in uids(prob, positive, K)]
        assert after, order      # the oracle places In [a] / Exists pods on the node that lacks the key, AFTER a NotIn pod joined it: the decline is needed
        auto = check_declined(oracle, lib, prob, NODE_KEY_DEFINEDNESS)
        assert nodes_of(auto, uids(prob, positive, K)).get(lacking, 0) == len(after)
        assert ec.where(ec.solve(prob, BASE, lib)) == ("general", 4)   # every setting below keeps its reason
        # the twin: every node carries the key — nothing is ever added to a node
        twin = key_definedness_problem(every_node_keyed=True, positive=positive, keyed_first=keyed_first)
        got, want = check_engine(oracle, lib, twin)
        assert nodes_of(want, uids(twin, "NotIn", K)) and nodes_of(want, uids(twin, positive, K))


def check_limit(oracle, lib):
    prob = limit_problem()
    got, want = check_engine(oracle, lib, prob)
    assert nodes_of(want, negative_uids(prob)) and lc.stages(got)[0] >= 1 and {"capped", "open"} <= set(lc.pool_of(want))


def check_complement_pool(oracle, lib):
    prob = complement_pool_problem()
    got, want = check_engine(oracle, lib, prob)
    assert nodes_of(want, negative_uids(prob)) and pc.claims_of(want, "big")
    assert ec.where(ec.solve(prob, "auto-nodes", lib)) == ("general", 34)   # (only plain_ops lets the Gt pool's batch onto the cursor engine)


def check_daemonsets(oracle, lib):
    for kind in ("a", "b", "c"):
        prob = daemonset_problem(kind)
        got, want = check_engine(oracle, lib, prob)
        assert nodes_of(want, negative_uids(prob)) and want["newNodeClaims"]


def check_no_zone(oracle, lib):
    prob = no_zone_problem()
    got, want = check_unschedulable(oracle, lib, prob)
    assert len(want["podErrors"]) == 2 and got["podErrors"] == want["podErrors"] and nodes_of(want, negative_uids(prob))


def check_loop_declines(oracle, lib):
    for reason, prob in loop_declines():
        assert prob["stateNodes"]
        check_declined(oracle, lib, prob, reason)


def check_variants(oracle, lib, names_lib):
    """3,072 / 3,073 nodes: phaseCycles[19] 1 / 2 under the switch; on `names_lib` (a build that reports kernel names) the stage kernel
    is the _p one in front of the PodOps loop, and still the plain one under "cursor-nodes"."""
    for n_nodes, variant, mem in ((3072, 1, "lds"), (3073, 2, "hbm")):
        prob = variant_problem(n_nodes)
        want = oracle.solve(prob)
        got = ec.solve(prob, AUTO, lib)
        assert ec.where(got) == ("cursor", 0) and got["counters"]["phaseCycles"][19] == variant, got["counters"]
        digest = parity.results_digest(got)[0]
        SWITCH.same(got, want, prob)
        assert sum(nodes_of(want, negative_uids(prob)).values()) >= 20 and want["newNodeClaims"] and not want["podErrors"]
        base = ec.solve(prob, BASE, lib)
        assert ec.where(base) == ("general", 4) and parity.results_digest(base)[0] == digest
        res, names = kc.solve(prob, ENGINE, names_lib)
        assert ec.where(res) == ("cursor", 0) and names == (f"ksolve_pack_nodes_{mem}_p", "ksolve_pack_fast_p_g0r1"), names
        assert parity.results_digest(res)[0] == digest
    positive = en.block_edge_problem(63)
    for setting, kernels in (("cursor-nodes", ("ksolve_pack_nodes_lds", "ksolve_pack_fast_g0r1")), ("cursor-pod-operators", ("ksolve_pack_nodes_lds", "ksolve_pack_fast_p_g0r1")),
                             (ENGINE, ("ksolve_pack_nodes_lds_p", "ksolve_pack_fast_p_g0r1"))):   # the setting picks the kernel, not the batch
        res, names = kc.solve(positive, setting, names_lib)
        assert ec.where(res) == ("cursor", 0) and names == kernels, (setting, names)


def check_repeated(oracle, lib, n):
    prob = repeated_problem()
    want = oracle.solve(prob)
    assert nodes_of(want, negative_uids(prob))
    digests, last = ec.digests_of_repeated_solves(lib, prob, AUTO, n, "cursor")
    assert len(digests) == 1
    SWITCH.same(last, want, prob)


def check_solve_many(oracle, lib):
    """One SolveMany: a member under 32 (nodes and negative pods), one under 33, the 37 batch under both, beside plain members."""
    members = [(fx.config1(), "auto"), (block_edge_problem(65, True), AUTO), (dedicated_problem(), ENGINE), (key_definedness_problem(), AUTO),
               (key_definedness_problem(), ENGINE), (fx.config1(pods=300, n_types=144, seed=7), AUTO), (block_edge_problem(65, True), BASE)]
    want = [mc.lone_cell(lib, p, s) for p, s in members]
    scheds = mc.open_members(members, lib)
    try:
        results, _ = mc.many(scheds)
    finally:
        mc.close_all(scheds)
    got = [mc.cell_of(r) for r in results]
    mc.assert_cells(got, want, list(range(len(members))))
    assert [(c["engine"], c["engineFallbackReason"]) for c in got if c["outcome"] != "Unsupported"] == \
        [("cursor", 0), ("cursor", 0), ("cursor", 0), ("general", 37), ("cursor", 0), ("general", 4)], got
    assert got[4]["outcome"] == "Unsupported" and "cursor engine declined the problem (reason 37)" in got[4]["error"], got[4]
    mc.same_as_oracle(oracle, members, results)

