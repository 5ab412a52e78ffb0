"""CPU tests of the cursor engine's existing-node stage (csrc/node_stage.h, engine "cursor-nodes" / "auto-nodes"): through the host
emulation of the device code (tests/emu, test infrastructure only), the real C ABI and the real flattener, against the oracle claim
by claim, node by node and in the reference-equivalent evaluation count. The device run is tests/test_gpu_cursor_nodes.py."""
import pytest

import engine_checks as ec
import existing_node_cases as en
import parity
from karpenter_amd import fixtures as fx
from karpenter_amd.scheduling import NewScheduler, SolveBatch, Unsupported
from test_device_algorithm import emu  # noqa: F401  (fixture)


@pytest.mark.parametrize("n_nodes", en.BLOCK_EDGES)
def test_block_edges(oracle, emu, n_nodes):
    got, want = en.check_engine(oracle, emu, en.block_edge_problem(n_nodes), variant=1)
    names = {e["name"] for e in want["existingNodes"] if e["pods"]}
    assert en.on_nodes(want) >= 2 and want["newNodeClaims"] and not want["podErrors"]
    assert f"node-{n_nodes - 1:04d}" in names or n_nodes == 1       # the last block's last node is reached
    zone3 = [c for c in want["newNodeClaims"] if any(r["key"] == fx.ZONE and r["values"] == ["test-zone-3"] for r in c["requirements"])]
    assert zone3                                                    # the classes no node is compatible with went to NodeClaims


def test_every_pod_on_a_node_and_none(oracle, emu):
    got, want = en.check_engine(oracle, emu, en.all_on_nodes_problem())
    assert not got["newNodeClaims"] and en.on_nodes(got) == 12      # the loop's queue is empty: zero claims, not a failure
    got, want = en.check_engine(oracle, emu, en.none_on_nodes_problem())
    assert en.on_nodes(got) == 0 and len(got["newNodeClaims"]) == len(want["newNodeClaims"]) > 0


def test_negative_remaining(oracle, emu):
    got, _ = en.check_engine(oracle, emu, en.negative_remaining_problem())
    by = {e["name"]: len(e["pods"]) for e in got["existingNodes"]}
    assert by.get("node-0", 0) == 0 and by["node-1"] > 0


@pytest.mark.parametrize("kind", ["a", "b", "c"])
def test_nodes_with_daemonsets(oracle, emu, kind):
    prob = fx.with_daemonsets(fx.with_existing_nodes(fx.config2(pods=1500, n_types=60, seed=4), 70, seed=3), kind)
    got, _ = en.check_engine(oracle, emu, prob)
    assert en.on_nodes(got) > 0 and got["newNodeClaims"]


def test_production_like(oracle, emu):
    # (config4: 4,800 pod classes — past the 4,096 whose cursors fit in LDS beside the nodes' remaining resources, which go to HBM)
    for prob, variant in ((fx.config2(pods=6000, n_types=144, seed=3), 1), (fx.config4(pods=8000, n_types=1000, n_pools=16, seed=5), 2)):
        q = fx.with_daemonsets(fx.with_existing_nodes(prob, 200, seed=9), "c")
        got, _ = en.check_engine(oracle, emu, q, variant=variant)
        assert en.on_nodes(got) > 200 and got["newNodeClaims"] and not got["podErrors"]


def test_lds_and_hbm_variants(oracle, emu):
    """One problem on each side of kNodeStageLdsRem (96 KiB of remaining resources: 3,072 nodes at four resource dimensions)."""
    base = fx.config2(pods=5000, n_types=144, seed=11)
    assert len({k for it in base["instanceTypes"] for k in it["capacity"]}) == 4
    for n_nodes, variant in ((3072, 1), (3073, 2)):
        prob = fx.with_existing_nodes(base, n_nodes, seed=2, fill=(0.93, 1.0), small=True)
        got, _ = en.check_engine(oracle, emu, prob, variant=variant)
        assert en.on_nodes(got) > 500 and got["newNodeClaims"]


def test_step_limit(oracle, emu):
    """maxSteps (the ctx deadline's stand-in): a step is a queue pop across both stages; the cursor engine equals the general engine
    stopped at the same step."""
    prob = fx.with_existing_nodes(fx.config2(pods=2000, n_types=60, seed=6), 30, seed=1)
    full = ec.solve(prob, "cursor-nodes", emu)
    uid_on_node = {u for e in full["existingNodes"] for u in e["pods"]}
    assert 200 < len(uid_on_node) < 1900
    for steps in (1, 63, 64, 65, 150, 1200, 1999):
        c = ec.solve(dict(prob, options=dict(prob["options"], maxSteps=steps)), "cursor-nodes", emu)
        g = ec.solve(dict(prob, options=dict(prob["options"], maxSteps=steps)), "general", emu)
        assert c["counters"]["engine"] == "cursor" and c["timedOut"] and g["timedOut"], steps
        parity.assert_same_results(c, g)
        assert c["scheduledPods"] == g["scheduledPods"] == steps and c["counters"]["pops"] == g["counters"]["pops"]
        assert c["counters"]["referenceBinEvaluations"] == g["counters"]["referenceBinEvaluations"]
    # a limit the queue never reaches is no limit
    c = ec.solve(dict(prob, options=dict(prob["options"], maxSteps=2000)), "cursor-nodes", emu)
    assert not c["timedOut"]
    ec.same(c, oracle.solve(prob), prob)


def test_step_limit_inside_the_node_prefix(oracle, emu):
    """The queue's first pods all land on nodes: limits inside that prefix and one past it."""
    its = fx.fake_instance_types(8)
    nodes = [fx.state_node(f"node-{i}", its[7], "test-zone-1", "on-demand", "default") for i in range(2)]
    pods = [fx.pod(requests={"cpu": "1"}) for _ in range(10)] + [fx.pod(requests={"cpu": "100m"}, node_selector={fx.ZONE: "test-zone-2"}) for _ in range(6)]
    prob = fx.problem(its, [fx.node_pool()], pods, state_nodes=nodes)
    want = oracle.solve(prob)
    assert en.on_nodes(want) == 10 and want["newNodeClaims"]       # queue order: the ten 1-cpu pods first
    for steps in (4, 10, 11):
        c = ec.solve(dict(prob, options={"maxSteps": steps}), "cursor-nodes", emu)
        g = ec.solve(dict(prob, options={"maxSteps": steps}), "general", emu)
        assert c["counters"]["engine"] == "cursor" and c["timedOut"] and g["timedOut"]
        parity.assert_same_results(c, g)
        assert c["scheduledPods"] == steps and c["counters"]["referenceBinEvaluations"] == g["counters"]["referenceBinEvaluations"]


def test_repeated_solves_and_batches(oracle, emu):
    prob = fx.with_daemonsets(fx.with_existing_nodes(fx.config2(pods=3000, n_types=144, seed=8), 100, seed=4), "b")
    s = NewScheduler(dict(prob, options=dict(prob["options"], engine="auto-nodes")), solver_lib=emu)
    digests = set()
    for _ in range(5):
        r = s.Solve()
        assert r["counters"]["engine"] == "cursor" and r["counters"]["engineFallbackReason"] == 0
        digests.add(parity.results_digest(r)[0])
    s.close()
    assert len(digests) == 1
    ec.same(r, oracle.solve(prob), prob)
    # ksolve_solve_batch: such handles run alone through solve(), plain ones in the batched cursor kernel
    probs = [fx.with_existing_nodes(fx.config2(pods=1200, n_types=60, seed=90 + i), 40 + 30 * i, seed=i) if i % 2 == 0 else fx.config2(pods=1200, n_types=60, seed=90 + i) for i in range(5)]
    scheds = [NewScheduler(dict(p, options=dict(p["options"], engine="auto-nodes")), solver_lib=emu) for p in probs]
    for _ in range(2):
        got = SolveBatch(scheds)
        assert [g["counters"]["engine"] for g in got] == ["cursor"] * 5
        for g, p in zip(got, probs):
            assert parity.results_digest(g)[0] == parity.results_digest(ec.solve(p, "auto-nodes", emu))[0]
            ec.same(g, oracle.solve(p), p)
            assert (en.on_nodes(g) > 0) == bool(p["stateNodes"])
    for s in scheds:
        s.close()


def _declined(oracle, emu, prob, reason, match="cursor engine"):
    with pytest.raises(Unsupported, match=match):
        ec.solve(prob, "cursor-nodes", emu)
    auto = ec.solve(prob, "auto-nodes", emu)
    assert auto["counters"]["engine"] == "general" and auto["counters"]["engineFallbackReason"] == reason, auto["counters"]
    ec.same(auto, oracle.solve(prob), prob)


def test_declines(oracle, emu):
    its = fx.fake_instance_types(8)
    node = fx.state_node("node-0", its[5], "test-zone-1", "on-demand", "default", used={"cpu": "500m", "pods": "1"})
    plain = [fx.pod(requests={"cpu": "900m"}) for _ in range(8)]
    # a node under consolidateAfter and a pod that must skip it (scheduler.go:628): bound to a node that is not being deleted
    quiet = fx.state_node("node-1", its[5], "test-zone-1", "on-demand", "default", under_consolidate_after=True)
    moving = [fx.pod(requests={"cpu": "900m"}, phase="Running", node_name="somewhere") for _ in range(3)]
    sim = {"consolidationSimulation": True}
    _declined(oracle, emu, fx.problem(its, [fx.node_pool()], plain + moving, state_nodes=[node, quiet], options=sim), 30)
    # ... while pending pods alone are exempt: the stage runs, and the node takes pods
    got, _ = en.check_engine(oracle, emu, fx.problem(its, [fx.node_pool()], plain, state_nodes=[node, quiet], options=sim))
    assert {e["name"] for e in got["existingNodes"] if e["pods"]} == {"node-0", "node-1"}
    # a NotIn pod could ADD a key to a node's requirements: setup()'s reason 4, found by the stage
    notin = plain + [fx.pod(requests={"cpu": "100m"}, node_requirements=[fx.req(fx.ZONE, "NotIn", "test-zone-2")])]
    _declined(oracle, emu, fx.problem(its, [fx.node_pool()], notin, state_nodes=[node]), 4)
    # a host port: outside the cursor engine's shape with or without nodes
    ported = plain + [fx.pod(requests={"cpu": "1"}, host_ports=[8080]) for _ in range(2)]
    _declined(oracle, emu, fx.problem(its, [fx.node_pool()], ported, state_nodes=[node]), 34)
    # an unschedulable pod: the stage runs, the loop stops at the pod (reason 27), the general engine re-solves from pristine nodes
    huge = plain + [fx.pod(requests={"cpu": "1000"})]
    prob = fx.problem(its, [fx.node_pool()], huge, state_nodes=[node])
    _declined(oracle, emu, prob, 27)
    assert len(oracle.solve(prob)["podErrors"]) == 1 and en.on_nodes(oracle.solve(prob)) > 0


def test_other_engines_still_refuse_nodes(emu):
    """"auto" and "cursor" behave as before; a problem without nodes launches no new kernel and counts the same work under the new names."""
    prob = en.block_edge_problem(5)
    assert ec.solve(prob, "auto", emu)["counters"]["engine"] == "general"
    with pytest.raises(Unsupported, match="cursor engine"):
        ec.solve(prob, "cursor", emu)
    a = ec.solve(fx.config1(), "auto", emu)["counters"]
    for engine in ("auto-nodes", "cursor-nodes"):
        c = ec.solve(fx.config1(), engine, emu)["counters"]
        assert c["engine"] == "cursor" and c["phaseCycles"][19] == 0
        assert (c["binEvaluations"], c["phaseCycles"][21], c["slowSorts"], c["referenceBinEvaluations"], c["pops"]) == \
               (a["binEvaluations"], a["phaseCycles"][21], a["slowSorts"], a["referenceBinEvaluations"], a["pops"])


def test_with_existing_nodes_leaves_the_problem_alone():
    prob = fx.config2(pods=500, n_types=60, seed=1)
    before = repr(prob)
    q = fx.with_existing_nodes(prob, 12, seed=2)
    assert len(q["stateNodes"]) == 12 and {k: v for k, v in q.items() if k != "stateNodes"} == {k: v for k, v in prob.items() if k != "stateNodes"}
    assert repr(prob) == before and repr(fx.with_existing_nodes(prob, 12, seed=2)) == repr(q)
    pools = {p["name"] for p in prob["nodePools"]}
    assert all(n["labels"][fx.NODEPOOL] in pools and n["initialized"] for n in q["stateNodes"])


SEEDS = list(range(60))


def test_seeded_fuzz(oracle, emu):
    clean = sum(1 for s in SEEDS if not oracle.solve(en.fuzz_problem(s))["podErrors"])
    assert clean * 4 >= len(SEEDS) * 3
    ran, placed, _ = en.run_fuzz(oracle, emu, SEEDS)
    assert ran * 4 >= len(SEEDS) * 3, ran       # at most a quarter left to the general engine
    assert placed > 0
