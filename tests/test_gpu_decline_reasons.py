"""GPU tests (run with -m gpu on an MI355X) of the fast engines' decline reasons (csrc/decline.h): the product library through the C
ABI against the oracle. The cases end in the reasons whose code both engines share (the NodePool-limit steps limits_exclude /
subtract_max of fast_engine.h: 23, 24, and limits that never bind), in the reason the host acts on in a batch (26) and in the one
after which a spread handle keeps its engine (27). Every expected reason and claim count below is a literal: the reasons were recorded
from the emulation of the commit before decline.h existed, the claim counts from the oracle.

A NodePool's `nodes` limit is never counted down inside one Solve() (subtractMax, scheduler.go:1049-1066, runs over instance-type
capacities, which carry no `nodes`): it stops a template only when nothing is left of it at the start (scheduler.go:711-715). So
the reason-23 case gives its first NodePool `nodes: 0`, the only limit below the claims the pods need that can bind."""
import pytest

import engine_checks as ec
from gpu_support import built  # noqa: F401  (fixture)
from karpenter_amd import fixtures as fx
from karpenter_amd.scheduling import NewScheduler, SolveBatch, Unsupported

pytestmark = pytest.mark.gpu

AB = {"a": "b"}


def pods(n, engine, **kw):
    """n equal pods; for the spread engine each carries one zonal spread constraint over all of them."""
    if engine == "spread":
        kw = dict(kw, labels=AB, topology_spread=[fx.spread(fx.ZONE, AB)])
    return [fx.pod(**kw) for _ in range(n)]


def limit_nodes_problem(engine):
    """Reason 23: the heavier NodePool has no node left; the general engine opens every claim on the other one."""
    pools = [fx.node_pool("first", weight=10, limits={"nodes": "0"}), fx.node_pool("second")]
    return fx.problem(fx.fake_instance_types(8), pools, pods(30, engine, requests={"cpu": "3"}))


def limit_cpu_problem(engine):
    """Reason 24 after several claims: every claim of a 3-cpu pod keeps the 8-cpu type, so subtractMax takes 8 cpu of the 40 per claim
    (40 -> 32 -> 24 -> 16 -> 8 -> 0) and no type is excluded before the sixth claim; the thirty pods need more than five."""
    return fx.problem(fx.fake_instance_types(8), [fx.node_pool(limits={"cpu": "40"})], pods(30, engine, requests={"cpu": "3"}))


def loose_limits_problem(engine):
    """Limits that never bind on three NodePools a zone each (lightest: any zone): subtract_max runs for every claim, reason 0."""
    lim = {"cpu": "100000"}
    pools = [fx.node_pool("one", weight=10, limits=lim, requirements=[fx.req(fx.ZONE, "In", "test-zone-1")]),
             fx.node_pool("two", weight=5, limits=lim, requirements=[fx.req(fx.ZONE, "In", "test-zone-2")]), fx.node_pool("any", limits=lim)]
    ps = pods(12, engine, requests={"cpu": "3"})
    if engine == "cursor":
        ps += [fx.pod(requests={"cpu": "2"}, node_selector={fx.ZONE: z}) for z in ("test-zone-2", "test-zone-3") for _ in range(9)]
    return fx.problem(fx.fake_instance_types(8), pools, ps)


def unschedulable_problem(engine):
    """Reason 27: one pod no instance type holds among twenty that are placed."""
    return fx.problem(fx.fake_instance_types(8), [fx.node_pool()], pods(20, engine, requests={"cpu": "1"}) + pods(1, engine, requests={"memory": "2Ti"}))


# (reason of the parent commit's emulation, NodeClaims the oracle opens)
LIMIT_CASES = {("nodes", "cursor"): (23, 15), ("nodes", "spread"): (23, 15), ("cpu", "cursor"): (24, 5), ("cpu", "spread"): (24, 5)}
LOOSE_CLAIMS = {"cursor": 12, "spread": 6}


@pytest.mark.parametrize("engine", ["cursor", "spread"])
@pytest.mark.parametrize("limit", ["nodes", "cpu"])
def test_limit_reasons(oracle, limit, engine):
    prob = (limit_nodes_problem if limit == "nodes" else limit_cpu_problem)(engine)
    reason, claims = LIMIT_CASES[limit, engine]
    want = oracle.solve(prob)
    assert len(want["newNodeClaims"]) == claims
    auto = ec.solve(prob, "auto", None)
    ec.same(auto, want, mode=ec.SETS)
    assert (auto["counters"]["engine"], auto["counters"]["engineFallbackReason"]) == ("general", reason), auto["counters"]
    with pytest.raises(Unsupported, match=rf"{engine} engine declined the problem \(reason {reason}\)"):
        ec.solve(prob, engine, None)


@pytest.mark.parametrize("engine", ["cursor", "spread"])
def test_limits_that_never_bind_stay_on_the_fast_engine(oracle, engine):
    prob = loose_limits_problem(engine)
    want = oracle.solve(prob)
    assert len(want["newNodeClaims"]) == LOOSE_CLAIMS[engine] and len({c["nodePool"] for c in want["newNodeClaims"]}) == 3 and not want["podErrors"]
    auto = ec.solve(prob, "auto", None)
    assert (auto["counters"]["engine"], auto["counters"]["engineFallbackReason"]) == (engine, 0), auto["counters"]
    ec.same(auto, want, mode=ec.SETS)


def test_batch_hands_back_a_handle_out_of_claim_slots(oracle):
    """ksolve_solve_batch reads the reason the same way ksolve_solve does: with the LDS plan capped at 64 claims (ldsClaimCap pins
    the plan, so nothing escalates) a problem of 100 claims comes back with reason 26 and runs on the general engine, beside a
    handle that stays on the cursor engine."""
    its = fx.fake_instance_types(8)
    small = fx.problem(its, [fx.node_pool()], [fx.pod(requests={"cpu": "7"}) for _ in range(100)], options={"ldsClaimCap": 64})
    other = fx.problem(its, [fx.node_pool()], [fx.pod(requests={"cpu": "1"}) for _ in range(40)])
    want = [oracle.solve(small), oracle.solve(other)]
    assert len(want[0]["newNodeClaims"]) == 100
    scheds = [NewScheduler(small), NewScheduler(other)]
    got = SolveBatch(scheds)
    for s in scheds:
        s.close()
    assert [(g["counters"]["engine"], g["counters"]["engineFallbackReason"]) for g in got] == [("general", 26), ("cursor", 0)]
    for g, w in zip(got, want):
        ec.same(g, w, mode=ec.SETS)


@pytest.mark.parametrize("engine", ["cursor", "spread"])
def test_an_unschedulable_pod_twice_on_one_handle(oracle, engine):
    prob = unschedulable_problem(engine)
    want = oracle.solve(prob)
    assert len(want["podErrors"]) == 1 and want["newNodeClaims"]
    s = NewScheduler(prob)
    try:
        for _ in range(2):
            got = s.Solve()
            assert (got["counters"]["engine"], got["counters"]["engineFallbackReason"]) == ("general", 27), got["counters"]
            ec.same(got, oracle.solve(prob), prob)   # (same() sorts the option lists in place: a fresh document per comparison)
    finally:
        s.close()
    with pytest.raises(Unsupported, match=rf"{engine} engine declined the problem \(reason 27\)"):
        ec.solve(prob, engine, None)
