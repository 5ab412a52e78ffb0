"""Problems with existing nodes for the cursor engine's node stage (csrc/node_stage.h; tests/test_cursor_engine_nodes.py on the
emulation, tests/test_gpu_cursor_nodes.py on the device): known shapes, the seeded fuzz generator and the comparison helper."""
import random

import daemonset_cases as dc
import engine_checks as ec
from karpenter_amd import fixtures as fx
from mix_cases import lite_problem


def check_engine(oracle, lib, prob, variant=None):
    """"cursor-nodes" must solve it on the cursor engine — no fallback, reason 0 — and equal the oracle claim by claim, node by node
    and in the reference-equivalent evaluation count; so must "auto-nodes" (which has to pick the same engine) and the general
    engine. `variant`: where the stage must have kept the nodes' remaining resources (1 LDS, 2 HBM; phaseCycles[19])."""
    got, want = ec.three_ways(oracle, lib, prob, "cursor-nodes", auto="auto-nodes", kind="cursor")
    if variant is not None:
        assert got["counters"]["phaseCycles"][19] == variant
    return got, want


def on_nodes(res):
    return sum(len(e["pods"]) for e in res.get("existingNodes", []))


TAINT = {"key": "dedicated", "value": "batch", "effect": "NoSchedule"}


def block_edge_problem(n_nodes):
    """`n_nodes` small nodes (2 or 4 cpu, half used) in zones 1 and 2, every seventh one tainted; pods that fill one node after the other, through
    every block and beyond the last node; and three classes no node is compatible with: a zone without nodes, a
    label key the nodes lack (the NodePool's own label, which these nodes do not carry), and — on the tainted nodes — every pod
    that does not tolerate the taint."""
    its = fx.fake_instance_types(8)
    pool = fx.node_pool(labels={"team": "a"})
    nodes = []
    for i in range(n_nodes):
        it = its[1 + 2 * (i % 2)]
        nodes.append(fx.state_node(f"node-{i:04d}", it, f"test-zone-{1 + i % 2}", "on-demand", "default",
                                   used={"cpu": f"{500 + 250 * (i % 3)}m", "pods": "1"}, taints=[TAINT] if i % 7 == 3 else None))
    pods = [fx.pod(requests={"cpu": "700m"}) for _ in range(max(3, n_nodes // 2 + 5))]
    pods += [fx.pod(requests={"cpu": "300m"}, tolerations=[{"key": "dedicated", "operator": "Exists"}]) for _ in range(7 * n_nodes + 9)]
    pods += [fx.pod(requests={"cpu": "1200m"}, node_selector={fx.ZONE: "test-zone-2"}) for _ in range(n_nodes // 3 + 2)]
    pods += [fx.pod(requests={"cpu": "400m"}, node_selector={fx.ZONE: "test-zone-3"}) for _ in range(5)]       # no node in that zone
    pods += [fx.pod(requests={"cpu": "200m"}, node_selector={"team": "a"}) for _ in range(5)]                  # no node has the key
    return fx.problem(its, [pool], pods, state_nodes=nodes)


BLOCK_EDGES = (1, 63, 64, 65, 129)


def all_on_nodes_problem():
    its = fx.fake_instance_types(8)
    nodes = [fx.state_node(f"node-{i}", its[7], "test-zone-1", "on-demand", "default") for i in range(3)]
    return fx.problem(its, [fx.node_pool()], [fx.pod(requests={"cpu": "500m"}) for _ in range(12)], state_nodes=nodes)


def none_on_nodes_problem():
    its = fx.fake_instance_types(8)
    nodes = [fx.state_node(f"node-{i}", its[2], "test-zone-1", "on-demand", "default", used={"cpu": "2800m"}) for i in range(70)]
    return fx.problem(its, [fx.node_pool()], [fx.pod(requests={"cpu": "500m"}) for _ in range(40)], state_nodes=nodes)


def negative_remaining_problem():
    """node-0 is over-committed on memory (remaining < 0: resources.Fits refuses everything, existingnode.go:96, even pods that
    ask for no memory); node-1 takes the pods."""
    its = fx.fake_instance_types(8)
    nodes = [fx.state_node("node-0", its[5], "test-zone-1", "on-demand", "default", used={"memory": "100Gi"}),
             fx.state_node("node-1", its[5], "test-zone-1", "on-demand", "default", used={"cpu": "1"})]
    pods = [fx.pod(requests={"cpu": "900m"}) for _ in range(9)]
    return fx.problem(its, [fx.node_pool()], pods, state_nodes=nodes)


def _zones(prob):
    return sorted({v for it in prob["instanceTypes"] for r in it["requirements"] if r["key"] == fx.ZONE for v in r["values"]})


def fuzz_problem(seed):
    """mix_cases.lite_problem plus random nodes (fixtures.with_existing_nodes) and, two times in three, random DaemonSets."""
    rng = random.Random(33000 + seed)
    prob = lite_problem(rng, rng.choice([30, 200, 900]))
    prob = fx.with_existing_nodes(prob, rng.choice([1, 5, 40, 64, 130]), seed=seed, fill=(0.3, 1.0))
    if rng.random() < 0.66:
        prob["daemonSetPods"] = dc.random_daemonsets(rng, _zones(prob))
    return prob


def run_fuzz(oracle, lib, seeds):
    """Whatever "auto-nodes" runs equals the oracle; returns (problems the cursor engine solved, pods it put on nodes, reasons)."""
    ran, placed, reasons = 0, 0, {}
    for _, _, _, got, on, reason in ec.fuzz_cases(oracle, lib, ((seed, fuzz_problem(seed)) for seed in seeds), "auto-nodes", pops=False):
        if on == "cursor":
            ran += 1
            placed += on_nodes(got)
        else:
            assert on == "general"
            reasons[reason] = reasons.get(reason, 0) + 1
    print(f"cursor + node stage: {ran} of {len(seeds)}, {placed} pods on existing nodes; general engine by reason {dict(sorted(reasons.items()))}")
    return ran, placed, reasons
