"""The two random batch generators of the fast engines' shapes, which the case modules build on: lite_problem (the cursor engine's
shape; tests/test_cursor_engine.py) and mix / fuzz_problem (the spread engine's; tests/test_spread_engine.py)."""
import copy
import random

from karpenter_amd import fixtures as fx


def lite_problem(rng, n_pods):
    """Random provisioning batches of the shape the cursor engine solves: In selectors on arch / os / zone / capacity type and
    a custom NodePool label, taints + tolerations, weighted pools, instance types whose allocatable vectors do not dominate
    each other (several Pareto-maximal types per requirement set), requests that straddle them."""
    kwok = rng.random() < 0.4
    if kwok:
        its = fx.kwok_catalog(rng.choice([24, 72, 144, 300])); wk = fx.KWOK_WELL_KNOWN; zones = list(fx.KWOK_ZONES)
    else:
        its = copy.deepcopy(fx.fake_instance_types(rng.choice([6, 20, 60]))); wk = fx.FAKE_WELL_KNOWN; zones = ["test-zone-1", "test-zone-2", "test-zone-3"]
        for it in its:   # cpu-heavy and memory-heavy shapes: no single type dominates
            if rng.random() < 0.5:
                it["capacity"]["memory"] = f"{rng.choice([1, 2, 4, 8, 64, 256])}Gi"
            if rng.random() < 0.3:
                it["capacity"]["pods"] = str(rng.choice([3, 8, 30, 110]))
    archs = sorted({v for it in its for r in it["requirements"] if r["key"] == fx.ARCH for v in r["values"]})
    pools, teams = [], []
    for i in range(rng.choice([0, 0, 1, 2])):
        kw = {}
        reqs = []
        if rng.random() < 0.4: reqs.append(fx.req(fx.ZONE, "In", *rng.sample(zones, rng.choice([1, 2, 3]))))
        if rng.random() < 0.3: reqs.append(fx.req(fx.CAPACITY_TYPE, "In", rng.choice(["spot", "on-demand"])))
        if rng.random() < 0.4: kw["taints"] = [{"key": "dedicated", "value": f"t{i}", "effect": "NoSchedule"}]
        if rng.random() < 0.5: kw["labels"] = {"team": f"t{i}"}; teams.append(f"t{i}")
        if rng.random() < 0.3: kw["limits"] = {"cpu": "100000"}     # present, never binding
        pools.append(fx.node_pool(f"pool-{i}", weight=rng.randrange(1, 20), requirements=reqs, **kw))
    pools.append(fx.node_pool("catch-all", weight=0))   # every pod without a team selector can land here
    if kwok:
        for np_ in pools: np_["nodeClassLabelKey"] = "karpenter.kwok.sh/kwoknodeclass"
    sizes = [(c, m) for c in (100, 250, 700, 1500, 3000) for m in (64, 300, 1024, 5000)]
    classes = []
    for _ in range(rng.randrange(1, 40)):
        sel = {}
        if rng.random() < 0.3: sel[fx.ARCH] = rng.choice(archs)
        if rng.random() < 0.3: sel[fx.ZONE] = rng.choice(zones[:2])
        if rng.random() < 0.2: sel[fx.CAPACITY_TYPE] = rng.choice(["spot", "on-demand"])
        if rng.random() < 0.15: sel[fx.OS] = "linux"
        if teams and rng.random() < 0.15: sel["team"] = rng.choice(teams)
        reqs = None
        if fx.ZONE not in sel and rng.random() < 0.2: reqs = [fx.req(fx.ZONE, "In", *rng.sample(zones, 2))]
        tol = [{"key": "dedicated", "operator": "Exists"}] if (rng.random() < 0.4 or "team" in sel) else None
        c, m = rng.choice(sizes)
        classes.append(dict(requests={"cpu": f"{c}m", "memory": f"{m}Mi"}, node_selector=sel or None, node_requirements=reqs, tolerations=tol))
    pods = [fx.pod(**rng.choice(classes)) for _ in range(n_pods)]
    return fx.problem(its, pools, pods, well_known=wk)


def mix(rng, n, zones=("test-zone-1", "test-zone-2", "test-zone-3"), letters="abc", kinds=range(12), big=False, filters=False):
    labels = [{"my-label": c} for c in letters]
    cpus = [100, 250, 500, 1000, 1500] if not big else [1000, 2000, 4000]
    res = lambda: {"cpu": f"{rng.choice(cpus)}m", "memory": f"{rng.choice([100, 256, 512, 1024])}Mi"}
    pods = []
    lonely = 0
    for _ in range(n):
        kind = rng.choice(list(kinds))
        lab, sel = rng.choice(labels), rng.choice(labels)
        kw = dict(labels=lab, requests=res())
        if kind == 0:
            kw["topology_spread"] = [fx.spread(fx.ZONE, sel, max_skew=rng.choice([1, 1, 2, 3]))]
        elif kind == 1:
            kw["topology_spread"] = [fx.spread(fx.HOSTNAME, sel, max_skew=rng.choice([1, 1, 2]))]
        elif kind == 2:
            kw["pod_requirements"] = [fx.affinity_term(fx.ZONE, lab if rng.random() < 0.8 else sel)]
        elif kind == 3:
            kw["pod_anti_requirements"] = [fx.affinity_term(fx.HOSTNAME, lab if rng.random() < 0.7 else sel)]
        elif kind == 4:
            kw["topology_spread"] = [fx.spread(fx.ZONE, sel), fx.spread(fx.HOSTNAME, sel, max_skew=2)]
        elif kind == 5:
            kw["node_selector"] = {fx.ZONE: rng.choice(zones)}
            if filters and rng.random() < 0.5:
                kw["topology_spread"] = [fx.spread(fx.CAPACITY_TYPE, sel)]
        elif kind == 6:
            kw["node_selector"] = {fx.CAPACITY_TYPE: rng.choice(["spot", "on-demand"])}
            if filters:
                kw["topology_spread"] = [fx.spread(fx.ZONE, sel, max_skew=rng.choice([1, 2]))]
        elif kind == 7 and not filters:
            kw["topology_spread"] = [fx.spread(fx.CAPACITY_TYPE, sel)]
        elif kind == 8:    # two groups on dictionary keys: each narrows from the claim's own set (topology.go:226-250)
            kw["topology_spread"] = [fx.spread(fx.ZONE, sel, max_skew=rng.choice([1, 2])), fx.spread(fx.CAPACITY_TYPE, sel)]
        elif kind == 12:   # ... loose enough to be satisfiable together
            kw["topology_spread"] = [fx.spread(fx.ZONE, sel, max_skew=3), fx.spread(fx.CAPACITY_TYPE, sel, max_skew=4)]
        elif kind == 9:    # minDomains (topologygroup.go:318-320)
            kw["topology_spread"] = [fx.spread(fx.ZONE, sel, min_domains=rng.choice([2, 3, 3, 5] if rng.random() < 0.1 else [2, 3]), max_skew=rng.choice([1, 2]))]
        elif kind == 10 and lonely < 2:   # anti-affinity on a dictionary key: a pod blocks every zone it could land in — a few of them, pinned to a zone each
            lonely += 1
            kw["pod_anti_requirements"] = [fx.affinity_term(fx.ZONE, {"zone-lonely": "x"})]
            kw["labels"] = dict(lab, **{"zone-lonely": "x"})
            kw["node_selector"] = {fx.ZONE: zones[lonely]}
        elif kind == 11:   # spread and affinity on the same key
            kw["topology_spread"] = [fx.spread(fx.ZONE, sel, max_skew=2)]
            kw["pod_requirements"] = [fx.affinity_term(fx.ZONE, lab)]
        pods.append(fx.pod(**kw))
    return pods


def fuzz_problem(seed):
    rng = random.Random(7000 + seed)
    kwok = seed % 2 == 0
    zones = tuple(fx.KWOK_ZONES[:3]) if kwok else ("test-zone-1", "test-zone-2", "test-zone-3")
    # (three seeds of four draw from the kinds that rarely leave a pod unschedulable — such a batch is the general engine's —, the fourth from all)
    kinds = range(12) if seed % 4 == 3 else (0, 0, 1, 1, 2, 3, 4, 5, 6, 7, 9, 10, 12, 12)
    pods = mix(rng, rng.randrange(30, 160), zones=zones, kinds=kinds, big=seed % 4 == 3, filters=seed % 8 == 7)
    pools = [fx.node_pool()]
    if seed % 3 == 1:
        pools = [fx.node_pool("a", requirements=[fx.req(fx.ZONE, "In", *zones[:2])], weight=10), fx.node_pool("b")]
    if seed % 5 == 2:
        pools = [fx.node_pool("few", limits={"cpu": "20"}, weight=5), fx.node_pool("rest")]
    if kwok:
        for np_ in pools:
            np_["nodeClassLabelKey"] = "karpenter.kwok.sh/kwoknodeclass"
        return fx.problem(fx.kwok_catalog(24), pools, pods, well_known=fx.KWOK_WELL_KNOWN)
    return fx.problem(fx.fake_instance_types(12), pools, pods)
