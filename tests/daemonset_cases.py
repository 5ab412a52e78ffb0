"""Problems with DaemonSets for the fast engines' tests (tests/test_fast_engines_daemonsets.py on the emulation,
tests/test_gpu_daemonsets.py on the device): the known answers, seeded fuzz generators and the comparison helper."""
import random

import engine_checks as ec
from karpenter_amd import fixtures as fx
from mix_cases import fuzz_problem, lite_problem


def check_engine(oracle, lib, prob, engine, plans=()):
    """engine (cursor / spread) must solve it — no fallback, reason 0 — and equal the oracle; so must auto (which has to pick the
    same engine) and the general engine; `plans`: further cursor settings that must agree. Instance-type lists as sets: daemon-overhead
    groups are visited in Go map order by the reference (scheduler.go:1001), so their order across groups is not defined."""
    return ec.three_ways(oracle, lib, prob, engine, plans=plans)


def four_resource_default_types():
    """The fake provider's default catalogue without its two GPU types: their extended resources make five resource dimensions,
    which the cursor engine declines whatever else the problem holds (test_cursor_engine.py); the DaemonSet known answers of
    suite_test.go do not involve them."""
    return [t for t in fx.fake_default_instance_types() if "gpu" not in t["name"]]


def known_answers():
    """The cases of test_device_algorithm.py::test_daemonset_overhead that have no existing node (suite_test.go "Daemonsets",
    :2143-2460), as (name, problem)."""
    its = four_resource_default_types()
    ds = [fx.pod(requests={"cpu": "1", "memory": "1Gi"})]
    out = [("one-group", fx.problem(its, [fx.node_pool()], [fx.pod(requests={"cpu": "1", "memory": "1Gi"})], daemonset_pods=ds))]
    ds2 = ds + [fx.pod(requests={"cpu": "2"}, node_selector={fx.ARCH: "arm64"})]
    pods = [fx.pod(requests={"cpu": f"{c}m"}) for c in (500, 900, 1500, 2500, 3500) for _ in range(4)]
    out.append(("arm64-group", fx.problem(its, [fx.node_pool()], pods, daemonset_pods=ds2)))
    out.append(("arm64-group-arm-pod", fx.problem(its, [fx.node_pool()], pods + [fx.pod(node_selector={fx.ARCH: "arm64"}, requests={"cpu": "3"})], daemonset_pods=ds2)))
    pools = [fx.node_pool(taints=[{"key": "k", "value": "v", "effect": "NoSchedule"}])]
    tol = [{"key": "k", "operator": "Exists"}]
    ds3 = [fx.pod(requests={"cpu": "1"}), fx.pod(requests={"cpu": "500m"}, tolerations=tol,
                                                 node_requirements=[[fx.req(fx.ZONE, "In", "nowhere")], [fx.req(fx.ZONE, "In", "test-zone-2")]])]
    out.append(("intolerant-and-relaxing", fx.problem(its, pools, [fx.pod(requests={"cpu": "1"}, tolerations=tol) for _ in range(6)], daemonset_pods=ds3)))
    return out


def random_daemonsets(rng, zones):
    """1-4 DaemonSets: selectors on arch / zone / os, tolerations, two-term node affinities whose first term matches nothing."""
    out = []
    for _ in range(rng.randrange(1, 5)):
        kw = dict(requests={"cpu": f"{rng.choice([25, 50, 100, 250])}m", "memory": f"{rng.choice([32, 64, 128])}Mi"})
        r = rng.random()
        if r < 0.25:
            kw["node_selector"] = {fx.ARCH: rng.choice(["amd64", "arm64"])}
        elif r < 0.40:
            kw["node_selector"] = {fx.ZONE: rng.choice(zones)}
        elif r < 0.50:
            kw["node_selector"] = {fx.OS: "linux"}
        elif r < 0.65:
            kw["node_requirements"] = [[fx.req(fx.OS, "In", "plan9")], [rng.choice([fx.req(fx.OS, "In", "linux"), fx.req(fx.ARCH, "In", "arm64"), fx.req(fx.ZONE, "In", rng.choice(zones))])]]
        if rng.random() < 0.6:
            kw["tolerations"] = [{"operator": "Exists"}]
        out.append(fx.pod(**kw))
    return out


def _zones(prob):
    return sorted({v for it in prob["instanceTypes"] for r in it["requirements"] if r["key"] == fx.ZONE for v in r["values"]})


def cursor_fuzz_problem(seed):
    rng = random.Random(31000 + seed)
    prob = lite_problem(rng, rng.choice([30, 200, 900]))
    prob["daemonSetPods"] = random_daemonsets(rng, _zones(prob))
    return prob


def spread_fuzz_problem(seed):
    prob = fuzz_problem(seed)
    rng = random.Random(32000 + seed)
    prob["daemonSetPods"] = random_daemonsets(rng, _zones(prob))
    return prob


def run_fuzz(oracle, lib, make, seeds, engine):
    """Whatever `auto` runs equals the oracle; returns (problems that ran on `engine`, histogram of fallback reasons)."""
    ran, reasons = 0, {}
    for _, _, _, _, on, reason in ec.fuzz_cases(oracle, lib, ((seed, make(seed)) for seed in seeds), "auto", pops=False):
        if on == engine:
            ran += 1
        else:
            assert on == "general"
            reasons[reason] = reasons.get(reason, 0) + 1
    print(f"{engine}: {ran} of {len(seeds)} on the fast engine; general engine by reason {dict(sorted(reasons.items()))}")
    return ran, reasons
