"""The spread engine (csrc/topo_engine.h; BASELINE configs[2]: the reference benchmark's own mix of zonal / hostname topology spread,
zonal pod affinity and hostname anti-affinity, scheduling_benchmark_test.go:259-455) against the oracle, claim by claim and in the
reference-equivalent evaluation count. CPU tests run the engine's source compiled for the host (tests/emu, test infrastructure)
behind the real C ABI and the host flattener; the `-m gpu` tests at the bottom run the same cases on the device library."""
import random

import pytest

import engine_checks as ec
import parity
from engine_checks import same, solve
from karpenter_amd import fixtures as fx
from karpenter_amd.scheduling import NewScheduler, Unsupported, device_available
from mix_cases import fuzz_problem, mix
from test_device_algorithm import emu  # noqa: F401  (fixture)


def check_spread(oracle, lib, prob):
    """engine=spread must solve it (no fallback) and equal the oracle; so must auto (which has to pick it) and the general engine."""
    return ec.three_ways(oracle, lib, prob, "spread", mode=ec.STRICT)


@pytest.mark.parametrize("pods,types,seed", [(300, 144, 1), (1500, 144, 5), (4000, 500, 42), (2500, 60, 9)])
def test_the_benchmark_mix(oracle, emu, pods, types, seed):
    got, want = check_spread(oracle, emu, fx.config3(pods=pods, n_types=types, seed=seed))
    assert not got["podErrors"] and len(got["newNodeClaims"]) == pods // 5   # every anti-affinity pod a NodeClaim of its own


def test_few_anti_affinity_pods_many_claims_without_one(oracle, emu):
    # the list of claims that hold no member of the anti-affinity group is the normal case here, not the exception; with a small
    # catalogue the claims fill up and the scan goes past the first window
    prob = fx.config3(pods=3000, n_types=20, seed=11, anti_affinity_pods=40)
    got, _ = check_spread(oracle, emu, prob)
    assert len(got["newNodeClaims"]) > 40


@pytest.mark.parametrize("seed", range(96))
def test_spread_fuzz(oracle, emu, seed):
    """Random mixes inside the engine's shape, on small catalogues so that constraints interact: shared selectors across kinds,
    pods pinned to zones / capacity types, several NodePools with different zones, claims that fill up. Whatever `auto` runs must
    equal the oracle; where the spread engine ran to the end (no unschedulable pod) it is held to the oracle by itself."""
    prob = fuzz_problem(seed)
    want = oracle.solve(prob)
    auto = solve(prob, "auto", emu)
    same(auto, want)
    if auto["counters"]["engine"] == "spread":
        got = solve(prob, "spread", emu)
        assert got["counters"]["engine"] == "spread"
        same(got, want)
    else:
        # outside the shape (a pod with a nodeSelector AND a spread constraint: its groups carry a node filter), an unschedulable pod,
        # a NodePool limit that excludes a type: the general engine, and asking for the spread engine alone is refused
        assert auto["counters"]["engine"] == "general" and auto["counters"]["engineFallbackReason"] != 0, auto["counters"]
        with pytest.raises(Unsupported):
            solve(prob, "spread", emu)


def test_fuzz_really_runs_the_spread_engine(oracle, emu):
    ran = 0
    for seed in range(12):
        rng = random.Random(9100 + seed)
        prob = fx.problem(fx.fake_instance_types(12), [fx.node_pool()], mix(rng, 80, kinds=[0, 1, 2, 3, 7, 7]))
        r = solve(prob, "auto", emu)
        same(r, oracle.solve(prob))
        ran += r["counters"]["engine"] == "spread"
    assert ran >= 8, ran


def test_kwok_catalogue_with_selectors_and_taints(oracle, emu):
    # BASELINE configs[1]'s selectors and the tainted NodePool, plus configs[2]'s constraints on a third of the pods
    rng = random.Random(5)
    base = fx.config2(pods=1200, n_types=144, seed=3)
    pods = fx.expand_pod_groups(base)["pods"]
    for i, p in enumerate(pods):
        lab = {"my-label": "abc"[i % 3]}
        p["labels"] = lab
        r = rng.random()
        if r < 0.15:
            p["topologySpreadConstraints"] = [fx.spread(fx.ZONE, lab)]
        elif r < 0.3:
            p["topologySpreadConstraints"] = [fx.spread(fx.HOSTNAME, lab, max_skew=2)]
        elif r < 0.35:
            p["podAntiAffinity"] = {"required": [fx.affinity_term(fx.HOSTNAME, {"my-label": "a"})], "preferred": []}
    prob = dict(base, pods=pods, podGroups=[])
    want = oracle.solve(prob)
    auto = solve(prob, "auto", emu)
    same(auto, want)


@pytest.mark.parametrize("case", ["hostname_affinity", "preference", "three_zonal_groups", "node_affinity_filter", "skew_7"])
def test_outside_its_shape_it_declines_loudly(oracle, emu, case):
    lab = {"app": "x"}
    kw = {"hostname_affinity": dict(pod_requirements=[fx.affinity_term(fx.HOSTNAME, lab)]),
          "preference": dict(pod_preferences=[fx.weighted(10, fx.affinity_term(fx.ZONE, lab))]),
          "three_zonal_groups": dict(topology_spread=[fx.spread(fx.ZONE, lab), fx.spread(fx.CAPACITY_TYPE, lab)], pod_requirements=[fx.affinity_term(fx.ZONE, lab)]),
          "node_affinity_filter": dict(topology_spread=[fx.spread(fx.ZONE, lab)], node_selector={fx.ZONE: "test-zone-1"}),
          "skew_7": dict(topology_spread=[fx.spread(fx.HOSTNAME, lab, max_skew=7)])}[case]
    pods = [fx.pod(labels=lab, requests={"cpu": "500m"}, **kw) for _ in range(6)]
    prob = fx.problem(fx.fake_instance_types(12), [fx.node_pool()], pods)
    with pytest.raises(Unsupported):
        solve(prob, "spread", emu)
    auto = solve(prob, "auto", emu)
    assert auto["counters"]["engine"] == "general"
    same(auto, oracle.solve(prob))


def test_an_unschedulable_pod_hands_the_problem_to_the_general_engine(oracle, emu):
    lab = {"app": "x"}
    pods = [fx.pod(labels=lab, requests={"cpu": "500m"}, topology_spread=[fx.spread(fx.ZONE, lab)]) for _ in range(5)]
    pods.append(fx.pod(labels=lab, requests={"cpu": "100000"}, topology_spread=[fx.spread(fx.HOSTNAME, lab)]))
    prob = fx.problem(fx.fake_instance_types(12), [fx.node_pool()], pods)
    auto = solve(prob, "auto", emu)
    assert auto["counters"]["engine"] == "general" and auto["counters"]["engineFallbackReason"] == 27 and len(auto["podErrors"]) == 1
    same(auto, oracle.solve(prob))


def test_repeated_solves_and_a_step_limit(oracle, emu):
    prob = fx.config3(pods=2000, n_types=144, seed=8)
    s = NewScheduler(dict(prob, options=dict(prob["options"], engine="spread")), solver_lib=emu)
    a, b = s.Solve(), s.Solve()
    s.close()
    assert parity.results_digest(a)[0] == parity.results_digest(b)[0]
    same(a, oracle.solve(prob))
    # the ctx deadline stand-in (scheduler.go:477-480): the pods placed so far are the results, the rest is not an error of theirs
    lim = solve(dict(prob, options=dict(prob["options"], maxSteps=700)), "spread", emu)
    assert lim["counters"]["engine"] == "spread" and lim["scheduledPods"] == 700


# ---- the same on the device ------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu


@gpu
@pytest.mark.parametrize("pods,types,seed", [(1500, 144, 5), (20000, 500, 42)])
def test_the_benchmark_mix_on_the_device(oracle, pods, types, seed):
    assert device_available()
    check_spread(oracle, None, fx.config3(pods=pods, n_types=types, seed=seed))


@gpu
def test_spread_fuzz_on_the_device(oracle):
    assert device_available()
    ran = 0
    for seed in range(24):
        prob = fuzz_problem(seed)
        r = solve(prob, "auto", None)
        same(r, oracle.solve(prob))
        ran += r["counters"]["engine"] == "spread"
    assert ran >= 8, ran
    prob = fx.config3(pods=3000, n_types=20, seed=11, anti_affinity_pods=40)
    check_spread(oracle, None, prob)


def test_round_6_widening_two_key_groups_min_domains_zonal_anti_affinity(oracle, emu):
    """What the engine took on after its first GPU passes: two groups on dictionary keys per pod (zone + capacity-type spread; spread and
    affinity on one key), minDomains, pod anti-affinity on a dictionary key with its inverse group — each with the answers the reference's
    tests assert, then against the oracle claim by claim."""
    lab = {"app": "x"}
    its, pool = fx.fake_instance_types(12), [fx.node_pool()]
    def run(pods, spread=True):
        prob = fx.problem(its, pool, pods)
        want = oracle.solve(prob)
        got = solve(prob, "spread" if spread else "auto", emu)
        # (a batch with an unschedulable pod is the general engine's: error codes, diagnostics, the relaxation ladder)
        assert got["counters"]["engine"] == ("spread" if spread else "general") and bool(want["podErrors"]) == (not spread)
        same(got, want)
        return got
    # minDomains larger than the zones there are: the global minimum counts as zero, maxSkew 1 lets ONE pod per zone in (topology_test.go:485-543)
    got = run([fx.pod(labels=lab, requests={"cpu": "500m"}, topology_spread=[fx.spread(fx.ZONE, lab, min_domains=5)]) for _ in range(3)])
    assert sorted(len(c["pods"]) for c in got["newNodeClaims"]) == [1, 1, 1]
    got = run([fx.pod(labels=lab, requests={"cpu": "500m"}, topology_spread=[fx.spread(fx.ZONE, lab, min_domains=5)]) for _ in range(6)], spread=False)
    assert len(got["podErrors"]) == 3
    run([fx.pod(labels=lab, requests={"cpu": "500m"}, topology_spread=[fx.spread(fx.ZONE, lab, min_domains=2, max_skew=2)]) for _ in range(9)])
    # zone + capacity-type spread on every pod (topology_test.go:1665-1740)
    run([fx.pod(labels=lab, requests={"cpu": "500m"}, topology_spread=[fx.spread(fx.ZONE, lab), fx.spread(fx.CAPACITY_TYPE, lab)]) for _ in range(5)])
    run([fx.pod(labels=lab, requests={"cpu": "500m"}, topology_spread=[fx.spread(fx.ZONE, lab, max_skew=2), fx.spread(fx.CAPACITY_TYPE, lab, max_skew=3)]) for _ in range(12)])
    got = run([fx.pod(labels=lab, requests={"cpu": "500m"}, topology_spread=[fx.spread(fx.ZONE, lab), fx.spread(fx.CAPACITY_TYPE, lab)]) for _ in range(12)], spread=False)
    assert len(got["podErrors"]) == 7   # (each constraint picks ITS minimum domain from the claim's own set; the two picks must meet)
    # spread and affinity on one key: the spread's minimum-count zone must be one the affinity admits
    run([fx.pod(labels=lab, requests={"cpu": "500m"}, topology_spread=[fx.spread(fx.ZONE, lab, max_skew=4)], pod_requirements=[fx.affinity_term(fx.ZONE, lab)]) for _ in range(4)])
    # anti-affinity on the zone: the first pod blocks every zone it COULD land in — all three (Schrödinger, topology_test.go:2502-2531)
    got = run([fx.pod(labels=lab, requests={"cpu": "500m"}, pod_anti_requirements=[fx.affinity_term(fx.ZONE, lab)]) for _ in range(5)], spread=False)
    assert len(got["newNodeClaims"]) == 1 and len(got["podErrors"]) == 4
    # ... pinned to zones they fill them one by one; pods the group does not select go anywhere
    aff = {"security": "s2"}
    zp = [fx.pod(requests={"cpu": "2"}, pod_anti_requirements=[fx.affinity_term(fx.ZONE, aff)], labels=aff, node_selector={fx.ZONE: f"test-zone-{i}"}) for i in (1, 2, 3)]
    got = run(zp + [fx.pod(requests={"cpu": "1"}) for _ in range(4)])
    assert len(got["newNodeClaims"]) == 3
    # ... and a pod the group selects is kept out of their zones by the inverse group (:2466-2500)
    zq = [fx.pod(requests={"cpu": "2"}, pod_anti_requirements=[fx.affinity_term(fx.ZONE, aff)], node_selector={fx.ZONE: f"test-zone-{i}"}) for i in (1, 2, 3)]
    victim = fx.pod(labels=aff)
    got = run(zq + [victim], spread=False)
    assert list(got["podErrors"]) == [victim["uid"]]
    got = run(zq[:2] + [victim])          # one zone is left for it
    assert not got["podErrors"]
