"""CPU tests of DaemonSet overhead on the CURSOR and SPREAD engines (csrc/fast_engine.h, csrc/topo_engine.h): the engines read a
type's allocatable less the overhead of its daemon-overhead group (ksolve_fast_eff_alloc, ksp.h eff_alloc). Through the host
emulation of the device code (tests/emu, test infrastructure only), the real C ABI and the real flattener, against the oracle claim
by claim and in the reference-equivalent evaluation count. The device run of the same cases is tests/test_gpu_daemonsets.py."""
import pytest

import daemonset_cases as dc
import engine_checks as ec
import parity
from karpenter_amd import fixtures as fx
from karpenter_amd.scheduling import NewScheduler, SolveBatch, Unsupported
from test_device_algorithm import emu  # noqa: F401  (fixture)

PLANS = ("cursor-wide", "cursor-hbm")


def test_known_answers_on_the_cursor_engine(oracle, emu):
    """suite_test.go "Daemonsets" (:2143-2460) with engine="cursor": no fallback, and FinalizeScheduling's smallest overhead is on
    the NodeClaim (nodeclaim.go:353-377)."""
    got = {}
    for name, prob in dc.known_answers():
        got[name], _ = dc.check_engine(oracle, emu, prob, "cursor", PLANS + ("cursor-pair",))
    req = got["one-group"]["newNodeClaims"][0]["requests"]
    assert int(req["cpu"]) == 2 * 10**9 and int(req["pods"]) == 2 * 10**9                 # suite_test.go:2155-2172
    # the full default catalogue has five resource dimensions (two GPU vendors): declined as before, DaemonSets or not
    prob = fx.problem(fx.fake_default_instance_types(), [fx.node_pool()], [fx.pod(requests={"cpu": "1", "memory": "1Gi"})], daemonset_pods=[fx.pod(requests={"cpu": "1", "memory": "1Gi"})])
    auto = ec.solve(prob, "auto", emu)
    assert auto["counters"]["engine"] == "general"
    ec.same(auto, oracle.solve(prob), prob)


@pytest.mark.parametrize("kind", ["a", "b", "c"])
def test_production_like_daemonsets_on_the_cursor_engine(oracle, emu, kind):
    for prob in (fx.config1(), fx.config2(pods=6000, n_types=144, seed=3), fx.config4(pods=8000, n_types=1000, n_pools=16, seed=5)):
        q = fx.with_daemonsets(prob, kind)
        got, _ = dc.check_engine(oracle, emu, q, "cursor", PLANS)
        assert not got["podErrors"]
    pair = ec.solve(fx.with_daemonsets(fx.config1(), kind), "cursor-pair", emu)   # one row of class slots: the two-wavefront kernel's plan
    assert pair["counters"]["engine"] == "cursor"
    ec.same(pair, oracle.solve(fx.with_daemonsets(fx.config1(), kind)), mode=ec.SETS)


@pytest.mark.parametrize("kind,pods", [("a", 2000), ("b", 5000), ("c", 20000)])
def test_production_like_daemonsets_on_the_spread_engine(oracle, emu, kind, pods):
    got, _ = dc.check_engine(oracle, emu, fx.with_daemonsets(fx.config3(pods=pods, n_types=144, seed=5), kind), "spread")
    assert not got["podErrors"] and len(got["newNodeClaims"]) >= pods // 5


def test_with_daemonsets_leaves_the_problem_alone():
    prob = fx.config2(pods=500, n_types=60, seed=1)
    before = repr(prob)
    for kind, n in (("a", 2), ("b", 4), ("c", 6)):
        q = fx.with_daemonsets(prob, kind)
        assert len(q["daemonSetPods"]) == n and {k: v for k, v in q.items() if k != "daemonSetPods"} == {k: v for k, v in prob.items() if k != "daemonSetPods"}
    assert repr(prob) == before
    with pytest.raises(ValueError):
        fx.with_daemonsets(prob, "z")


def _it(name, cpu, mem, arch):
    return fx.fake_instance_type(name, resources={"cpu": str(cpu), "memory": f"{mem}Gi", "pods": "200"}, architecture=arch)


def test_overhead_changes_the_pareto_vectors(oracle, emu):
    """Several Pareto vectors per requirement set that differ from the ones without DaemonSets. First catalogue: the arm64 type
    dominates the amd64 one; an arm64 DaemonSet of 40Gi leaves it less memory, so the dominated type becomes maximal. Second: a cpu-heavy
    amd64 type and a memory-heavy arm64 type are both maximal; an amd64 DaemonSet of 20 cpu makes the first dominated."""
    pods = [fx.pod(requests={"cpu": "3", "memory": "100Mi"}) for _ in range(30)] + [fx.pod(requests={"cpu": "100m", "memory": "20Gi"}) for _ in range(30)] + \
           [fx.pod(requests={"cpu": "500m", "memory": "1Gi"}) for _ in range(60)]
    its = [_it("amd-mid", 16, 32, "amd64"), _it("arm-big", 32, 64, "arm64"), _it("small", 2, 2, "amd64")]
    ds = [fx.pod(requests={"cpu": "100m", "memory": "40Gi"}, node_selector={fx.ARCH: "arm64"})]
    plain, _ = dc.check_engine(oracle, emu, fx.problem(its, [fx.node_pool()], pods), "cursor")
    got, want = dc.check_engine(oracle, emu, fx.problem(its, [fx.node_pool()], pods, daemonset_pods=ds), "cursor", PLANS)
    assert [c["instanceTypes"] for c in got["newNodeClaims"]] == [c["instanceTypes"] for c in want["newNodeClaims"]]
    assert [c["instanceTypes"] for c in got["newNodeClaims"]] != [c["instanceTypes"] for c in plain["newNodeClaims"]]
    assert any(c["instanceTypes"] == ["amd-mid"] for c in got["newNodeClaims"])       # a claim only the formerly dominated type holds
    its = [_it("amd-cpu", 32, 16, "amd64"), _it("arm-mem", 16, 64, "arm64"), _it("small", 2, 2, "amd64")]
    ds = [fx.pod(requests={"cpu": "20", "memory": "100Mi"}, node_selector={fx.ARCH: "amd64"})]
    got, want = dc.check_engine(oracle, emu, fx.problem(its, [fx.node_pool()], pods, daemonset_pods=ds), "cursor", PLANS)
    assert [c["instanceTypes"] for c in got["newNodeClaims"]] == [c["instanceTypes"] for c in want["newNodeClaims"]]
    assert all("small" not in c["instanceTypes"] for c in got["newNodeClaims"])        # 2 cpu cannot hold a 20-cpu DaemonSet


def test_types_that_cannot_hold_their_daemons(oracle, emu):
    its = fx.fake_instance_types(8)   # fake-it-0: 1 cpu, fake-it-1: 2 cpu, ...
    ds = [fx.pod(requests={"cpu": "2500m"})]
    pods = [fx.pod(requests={"cpu": "100m"}) for _ in range(30)]
    got, _ = dc.check_engine(oracle, emu, fx.problem(its, [fx.node_pool()], pods, daemonset_pods=ds), "cursor", PLANS)
    for c in got["newNodeClaims"]:
        assert not {"fake-it-0", "fake-it-1"} & set(c["instanceTypes"]) and c["instanceTypes"]
    # a DaemonSet no type can hold: every pod is unschedulable — the general engine owns the error codes
    prob = fx.problem(its, [fx.node_pool()], pods, daemonset_pods=[fx.pod(requests={"cpu": "1000"})])
    with pytest.raises(Unsupported, match="cursor engine"):
        ec.solve(prob, "cursor", emu)
    auto = ec.solve(prob, "auto", emu)
    assert auto["counters"]["engine"] == "general" and auto["counters"]["engineFallbackReason"] == 27
    want = oracle.solve(prob)
    ec.same(auto, want, mode=ec.SETS)
    assert len(want["podErrors"]) == 30 and not want["newNodeClaims"]


def test_nodepool_limits_with_daemonsets(oracle, emu):
    its = fx.fake_instance_types(8)
    ds = [fx.pod(requests={"cpu": "500m", "memory": "100Mi"})]
    pods = [fx.pod(requests={"cpu": "1"}) for _ in range(40)]
    # limits that never bind
    dc.check_engine(oracle, emu, fx.problem(its, [fx.node_pool(limits={"cpu": "100000"})], pods, daemonset_pods=ds), "cursor", PLANS)
    # limits that bind: declined as without DaemonSets, auto equals the oracle
    prob = fx.problem(its, [fx.node_pool(limits={"cpu": "20"})], pods, daemonset_pods=ds)
    with pytest.raises(Unsupported, match="cursor engine"):
        ec.solve(prob, "cursor", emu)
    auto = ec.solve(prob, "auto", emu)
    assert auto["counters"]["engine"] == "general" and auto["counters"]["engineFallbackReason"] in (23, 24)
    ec.same(auto, oracle.solve(prob), prob)
    # Whether the limit binds depends on subtractMax (scheduler.go:1049-1066) taking its maximum over the types that fit size +
    # overhead: a 900Mi pod fits the 32-cpu / 1Gi type alone but not beside a 200Mi DaemonSet, so a claim's options are the 8-cpu
    # type only and each of the two claims takes 8 cpu of the 48 — the 32-cpu type is never excluded (48 -> 40 -> 32). Counting 32
    # per claim would leave 16 and exclude it before the second claim (reason 24).
    its = [fx.fake_instance_type("cpu-32-mem-1", resources={"cpu": "32", "memory": "1Gi", "pods": "100"}),
           fx.fake_instance_type("cpu-8-mem-64", resources={"cpu": "8", "memory": "64Gi", "pods": "100"})]
    ds = [fx.pod(requests={"cpu": "100m", "memory": "200Mi"})]
    pods = [fx.pod(requests={"cpu": "1", "memory": "900Mi"}) for _ in range(10)]
    prob = fx.problem(its, [fx.node_pool(limits={"cpu": "48"})], pods, daemonset_pods=ds)
    got, want = dc.check_engine(oracle, emu, prob, "cursor")
    assert len(want["newNodeClaims"]) == 2 and all(c["instanceTypes"] == ["cpu-8-mem-64"] for c in want["newNodeClaims"])
    # (without the DaemonSet the first claim does keep the 32-cpu type, 32 cpu are taken and the type is excluded before the second claim)
    without = ec.solve(fx.problem(its, [fx.node_pool(limits={"cpu": "48"})], pods), "auto", emu)
    assert without["counters"]["engine"] == "general" and without["counters"]["engineFallbackReason"] == 24


def test_still_declined_with_daemonsets(oracle, emu):
    its = fx.fake_instance_types(8)
    ds = [fx.pod(requests={"cpu": "100m"})]
    # a host port: the per-group port conflict (nodeclaim.go:562-565) is not a dominance test
    prob = fx.problem(its, [fx.node_pool()], [fx.pod(requests={"cpu": "1"}, host_ports=[8080]) for _ in range(4)] + [fx.pod(requests={"cpu": "1"})], daemonset_pods=ds)
    spread = fx.problem(its, [fx.node_pool()], [fx.pod(labels={"a": "b"}, host_ports=[8080], topology_spread=[fx.spread(fx.ZONE, {"a": "b"})]) for _ in range(4)], daemonset_pods=ds)
    # one existing node
    node = fx.state_node("node-0", its[3], "test-zone-1", "on-demand", "default", used={"cpu": "500m", "pods": "1"})
    nodes = fx.problem(its, [fx.node_pool()], [fx.pod(requests={"cpu": "900m"}) for _ in range(8)], daemonset_pods=ds, state_nodes=[node])
    for p, engine in ((prob, "cursor"), (nodes, "cursor"), (spread, "spread")):
        with pytest.raises(Unsupported, match=f"{engine} engine"):
            ec.solve(p, engine, emu)
        auto = ec.solve(p, "auto", emu)
        assert auto["counters"]["engine"] == "general"
        ec.same(auto, oracle.solve(p), p)


CURSOR_SEEDS = list(range(60))
# spread_fuzz_problem builds on mix_cases.fuzz_problem, whose seeds = 2 mod 5 draw a NodePool limit of 20 cpu (it binds) and
# whose seeds = 3 mod 4 draw the kinds that leave pods unschedulable: both are the general engine's with or without DaemonSets. Of
# the sixty seeds kept the oracle alone reports pod errors for six.
SPREAD_SEEDS = [s for s in range(200) if s % 5 != 2 and s % 4 != 3][:60]


def test_seeded_fuzz_cursor_shaped(oracle, emu):
    clean = sum(1 for s in CURSOR_SEEDS if not oracle.solve(dc.cursor_fuzz_problem(s))["podErrors"])
    assert clean * 4 >= len(CURSOR_SEEDS) * 3
    ran, _ = dc.run_fuzz(oracle, emu, dc.cursor_fuzz_problem, CURSOR_SEEDS, "cursor")
    assert ran * 4 >= len(CURSOR_SEEDS) * 3, ran       # at most a quarter left to the general engine


def test_seeded_fuzz_spread_shaped(oracle, emu):
    clean = sum(1 for s in SPREAD_SEEDS if not oracle.solve(dc.spread_fuzz_problem(s))["podErrors"])
    assert clean * 4 >= len(SPREAD_SEEDS) * 3
    ran, _ = dc.run_fuzz(oracle, emu, dc.spread_fuzz_problem, SPREAD_SEEDS, "spread")
    assert ran * 4 >= len(SPREAD_SEEDS) * 3, ran


def test_repeated_solves_and_batches_of_daemonset_handles(oracle, emu):
    prob = fx.with_daemonsets(fx.config2(pods=3000, n_types=144, seed=8), "c")
    s = NewScheduler(prob, solver_lib=emu)
    digests = set()
    for _ in range(5):
        r = s.Solve()
        assert r["counters"]["engine"] == "cursor"
        digests.add(parity.results_digest(r)[0])
    s.close()
    assert len(digests) == 1
    # ksolve_solve_batch: the engine ksolve_solve picks — cursor-shaped handles in the batched cursor kernel, spread-shaped ones alone
    probs = [fx.with_daemonsets(fx.config2(pods=1200, n_types=60, seed=90 + i), "abc"[i % 3]) for i in range(6)]
    probs += [fx.with_daemonsets(fx.config3(pods=600, n_types=60, seed=3 + i), "bc"[i]) for i in range(2)]
    scheds = [NewScheduler(p, solver_lib=emu) for p in probs]
    for _ in range(2):
        want = [oracle.solve(p) for p in probs]   # (same() sorts the option lists in place)
        got = SolveBatch(scheds)
        assert [g["counters"]["engine"] for g in got] == ["cursor"] * 6 + ["spread"] * 2
        for g, w, p in zip(got, want, probs):
            assert parity.results_digest(g)[0] == parity.results_digest(ec.solve(p, "auto", emu))[0]   # ... and byte for byte what ksolve_solve returns
            ec.same(g, w, mode=ec.SETS)
    for s in scheds:
        s.close()


def test_counters_without_daemonsets_are_the_parents(emu):
    """fx.config1() on the commit before DaemonSets reached the fast engines (recorded from a run of that commit on the emulation):
    a problem without DaemonSets does the same work as before."""
    c = NewScheduler(fx.config1(), solver_lib=emu).Solve()["counters"]
    assert c["engine"] == "cursor" and c["claims"] == 41
    assert (c["binEvaluations"], c["phaseCycles"][21], c["slowSorts"], c["referenceBinEvaluations"]) == (320881, 5000, 267, 77421)   # phaseCycles[21] = fullEvaluations
