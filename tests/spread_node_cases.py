"""Problems with existing nodes AND topology groups for the spread engine's node path (csrc/topo_nodes.h, engines
"spread-nodes" / "auto-nodes-spread"; tests/test_spread_engine_nodes.py on the emulation, tests/test_gpu_spread_nodes.py on the
device): the benchmark mix with nodes, block edges, the node that refuses and later accepts, small known answers, the seeded fuzz
and the comparison helper."""
import random

import engine_checks as ec
import mix_cases
from karpenter_amd import fixtures as fx


def check_engine(oracle, lib, prob):
    """"spread-nodes" must solve it on the spread engine — no fallback, reason 0 — and equal the oracle: claims, nodes, the
    reference-equivalent evaluation count and the cost (instance-type lists as sets under DaemonSets, whose overhead groups the
    reference visits in Go map order, scheduler.go:1001); so must "auto-nodes-spread" (which has to pick the same engine) and the
    general engine."""
    return ec.three_ways(oracle, lib, prob, "spread-nodes", auto="auto-nodes-spread", kind="spread")


def on_nodes(res):
    return sum(len(e["pods"]) for e in res.get("existingNodes", []))


# (pods, n_types, seed) of fixtures.config3, nodes, pods on nodes, NodeClaims — and the last two with DaemonSets "c"
MIX = [((300, 144, 1), 5, (128, 56), (129, 56)),
       ((1500, 144, 5), 40, (1238, 262), (1236, 264)),
       ((4000, 500, 42), 200, (3392, 608), (3378, 622))]


def mix_problem(cfg, n_nodes, daemonsets=False):
    pods, n_types, seed = cfg
    prob = fx.with_existing_nodes(fx.config3(pods=pods, n_types=n_types, seed=seed), n_nodes, seed=3)
    return fx.with_daemonsets(prob, "c") if daemonsets else prob


BLOCK_EDGES = (1, 63, 64, 65, 129)


def block_edge_problem(n_nodes):
    """`n_nodes` two-cpu nodes alternating over zones 1 and 2; pods with zonal and hostname spread (at most two per node), more
    of them than the nodes hold: they are taken block after block, and beyond the last node on NodeClaims."""
    its = fx.fake_instance_types(8)
    nodes = [fx.state_node(f"node-{i:04d}", its[1], f"test-zone-{1 + i % 2}", "on-demand", "default") for i in range(n_nodes)]
    lab = {"app": "edge"}
    pods = [fx.pod(labels=lab, requests={"cpu": "300m"}, topology_spread=[fx.spread(fx.ZONE, lab), fx.spread(fx.HOSTNAME, lab, max_skew=2)])
            for _ in range(2 * n_nodes + 7)]
    return fx.problem(its, [fx.node_pool(requirements=[fx.req(fx.ZONE, "In", "test-zone-1", "test-zone-2")])], pods, state_nodes=nodes)


def refuse_then_accept_problem():
    """Three zones in the pool, every node in zone 1, zonal spread with maxSkew 1: a node refuses the second pod (skew), the pod
    opens a NodeClaim in another zone, and once zones 2 and 3 hold a pod each the nodes of zone 1 accept again."""
    its = fx.fake_instance_types(8)
    nodes = [fx.state_node(f"node-{i}", its[5], "test-zone-1", "on-demand", "default") for i in range(2)]
    lab = {"app": "wave"}
    pods = [fx.pod(labels=lab, requests={"cpu": "500m"}, topology_spread=[fx.spread(fx.ZONE, lab)]) for _ in range(9)]
    return fx.problem(its, [fx.node_pool()], pods, state_nodes=nodes)


def node_then_claim_then_node(want, prob):
    """From the oracle's answer: some zone-1 node took a pod before AND after a pod of the same class went to a NodeClaim in another
    zone. The pods are of one class with equal requests and creation times, so the queue pops them in uid order (queue.go:98-107),
    which is the order of prob["pods"]."""
    at = {p["uid"]: i for i, p in enumerate(sorted(prob["pods"], key=lambda p: p["uid"]))}
    elsewhere = []
    for c in want["newNodeClaims"]:
        zones = [r["values"] for r in c["requirements"] if r["key"] == fx.ZONE][0]
        if zones != ["test-zone-1"]:
            elsewhere += [at[u] for u in c["pods"]]
    for e in want["existingNodes"]:
        took = [at[u] for u in e["pods"]]
        if any(a < b < c for a in took for c in took for b in elsewhere):
            return True
    return False


def fuzz_problem(seed):
    rng = random.Random(51000 + seed)
    return fx.with_existing_nodes(mix_cases.fuzz_problem(seed), rng.choice([1, 5, 40, 64, 130]), seed=seed, fill=(0.3, 1.0))


def run_fuzz(oracle, lib, seeds):
    """Whatever "auto-nodes-spread" runs equals the oracle. A seed is a CANDIDATE when the same problem without its nodes runs on
    the spread engine under "auto" and the oracle solves it WITH nodes without pod errors; returns (candidates, candidates the
    spread engine solved with reason 0, pods it put on nodes, histogram of the other candidates' reasons)."""
    cands, ran, placed, reasons = 0, 0, 0, {}
    for _, prob, want, got, on, reason in ec.fuzz_cases(oracle, lib, ((seed, fuzz_problem(seed)) for seed in seeds), "auto-nodes-spread", pops=False):
        bare = ec.solve(dict(prob, stateNodes=[]), "auto", lib)["counters"]["engine"]
        if bare != "spread" or want["podErrors"]:
            continue
        cands += 1
        if on == "spread":
            ran += 1
            placed += on_nodes(got)
        else:
            reasons[reason] = reasons.get(reason, 0) + 1
    print(f"spread engine with nodes: {ran} of {cands} candidates ({len(seeds)} seeds), {placed} pods on existing nodes; "
          f"general engine by reason {dict(sorted(reasons.items()))}")
    return cands, ran, placed, reasons
