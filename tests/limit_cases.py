"""Problems whose NodePool limits BIND for the cursor engine's limit stages (csrc/fast_engine.h FastLimits, engines "auto-limits" /
"cursor-limits"; tests/test_cursor_engine_limits.py on the emulation, tests/test_gpu_cursor_limits.py on the device): known shapes,
the seeded fuzz generator and its Switch (tests/engine_checks.py).

What the reference does when a limit binds (scheduler.go:706-727): a template whose pool has no node left, or whose type list
filtered by the remaining resources is empty, is skipped for the pod; a list that shrank opens the NodeClaim with the shorter list;
subtractMax (scheduler.go:1049-1066) then takes the largest capacity among the claim's options off the pool's remaining resources."""
import random

import daemonset_cases as dc
import engine_checks as ec
from karpenter_amd import fixtures as fx
from mix_cases import lite_problem

# 11, 12 over "auto" ("auto-nodes" for a problem with existing nodes, which "auto" does not try): what engines 0-10 do is to decline
# with reason 23 / 24. No engine-only leg below the switch. declined(): plain "auto" stops earlier, at the limit.
SWITCH = ec.Switch("cursor", only="cursor-limits", auto="auto-limits", base="auto", reasons=(23, 24), base_first=True)
check_declined = SWITCH.declined


def _limit_word(res):
    """phaseCycles[23] of a cursor solve under engines 11 / 12 (csrc/fast_engine.h FastCold::finish; zero under every other setting):
    limit stages created | rows of class slots << 16 | claims open at the first exclusion << 32."""
    return res["counters"]["phaseCycles"][23] & 0xFFFFFFFFFFFFFFFF


def stages(res):
    """(limit stages the solve created, claims open when a limit first excluded a type or None)."""
    v = _limit_word(res)
    first = v >> 32
    return v & 0xFFFF, (None if first == 0xFFFFFFFF else first)


def rows(res):
    """Rows of 64 class slots of the kernel that ran: 1, or 4 when more than 64 pod classes are live at once in the queue."""
    return (_limit_word(res) >> 16) & 0xFFFF


def check_engine(oracle, lib, prob, base="auto"):
    """The limit binds in this problem: SWITCH.check under `base`."""
    return SWITCH.check(oracle, lib, prob, base=base)


def pool_of(res):
    return [c["nodePool"] for c in res["newNodeClaims"]]


def cpu_of(prob):
    return {it["name"]: fx.quantity_float(it["capacity"]["cpu"]) for it in prob["instanceTypes"]}


def max_cpu(claim, cpus):
    return max(cpus[t] for t in claim["instanceTypes"])


# ---- 1, 2: the decline-reason cases of tests/test_gpu_decline_reasons.py, rebuilt ------------------------------------------------

def cpu_chain_problem(second_pool):
    """Thirty 3-cpu pods, a NodePool with limits.cpu = 40 on the 1..8-cpu catalogue: every claim keeps the 8-cpu type, so subtractMax
    takes 8 of the 40 per claim (40 -> 32 -> 24 -> 16 -> 8 -> 0) and the first exclusion — of every type — happens at the sixth claim.
    Alone, the pool's template is skipped from then on and the eleventh pod is unschedulable (reason 27, out of scope); with a second,
    unlimited NodePool of lower weight the pods move there."""
    pools = [fx.node_pool("first", weight=10, limits={"cpu": "40"})] + ([fx.node_pool("second")] if second_pool else [])
    return fx.problem(fx.fake_instance_types(8), pools, [fx.pod(requests={"cpu": "3"}) for _ in range(30)])


def nodes_zero_problem():
    """Reason 23 for engines 0-10: the heavier NodePool has no node left (scheduler.go:711-715); every claim lands on the other one."""
    pools = [fx.node_pool("first", weight=10, limits={"nodes": "0"}), fx.node_pool("second")]
    return fx.problem(fx.fake_instance_types(8), pools, [fx.pod(requests={"cpu": "3"}) for _ in range(30)])


# ---- 3: two resources -----------------------------------------------------------------------------------------------------------

def two_resource_problem():
    """kwok catalogue of 24 types (1, 2, 4, 8 cpu x 2, 4, 8 GiB per cpu), one NodePool with limits on cpu AND memory, a second
    without: memory excludes the 64 GiB types before cpu excludes anything, cpu excludes the 8-cpu types later."""
    pools = [fx.node_pool("limited", weight=10, limits={"cpu": "26", "memory": "170Gi"}), fx.node_pool("open")]
    for p in pools:
        p["nodeClassLabelKey"] = "karpenter.kwok.sh/kwoknodeclass"
    pods = [fx.pod(requests={"cpu": "1500m", "memory": "1Gi"}) for _ in range(14)] + [fx.pod(requests={"cpu": "300m", "memory": "512Mi"}) for _ in range(40)]
    return fx.problem(fx.kwok_catalog(24), pools, pods, well_known=fx.KWOK_WELL_KNOWN)


# ---- 4: DaemonSets ----------------------------------------------------------------------------------------------------------------

def daemonset_problem(n_pods=30):
    """The cpu-32 / cpu-8 catalogue of test_fast_engines_daemonsets.test_nodepool_limits_with_daemonsets: a 900Mi pod fits the
    32-cpu / 1Gi type alone but not beside the 200Mi DaemonSet, so a claim's options are the 8-cpu type only and subtractMax, over
    the types that fit size + overhead, takes 8 cpu of the 48 per claim (48 -> 40 -> 32 -> 24: the 32-cpu type is excluded at the
    fourth claim, -> 16 -> 8). Ten pods need two claims and the limit never binds (the existing test); thirty need five. Counting 32
    for the first claim would leave 16, then 8, then nothing for the fourth."""
    its = [fx.fake_instance_type("cpu-32-mem-1", resources={"cpu": "32", "memory": "1Gi", "pods": "100"}),
           fx.fake_instance_type("cpu-8-mem-64", resources={"cpu": "8", "memory": "64Gi", "pods": "100"})]
    ds = [fx.pod(requests={"cpu": "100m", "memory": "200Mi"})]
    pods = [fx.pod(requests={"cpu": "1", "memory": "900Mi"}) for _ in range(n_pods)]
    return fx.problem(its, [fx.node_pool(limits={"cpu": "48"})], pods, daemonset_pods=ds)


def daemonset_overhead_problem():
    """1..8-cpu catalogue, a 500m DaemonSet, limits.cpu = 20 on the heavier pool (8, 8, then 20 - 16 = 4: the types above 4 cpu are
    excluded and a claim of the narrower list holds fewer pods beside the DaemonSet), a second pool for the rest."""
    ds = [fx.pod(requests={"cpu": "500m", "memory": "100Mi"})]
    pools = [fx.node_pool("first", weight=10, limits={"cpu": "20"}), fx.node_pool("second")]
    return fx.problem(fx.fake_instance_types(8), pools, [fx.pod(requests={"cpu": "1"}) for _ in range(40)], daemonset_pods=ds)


# ---- 5: a claim of an early stage takes pods after a later stage exists -----------------------------------------------------------

def early_stage_problem():
    """Twelve 3-cpu pods, then (queue order: larger requests first, queue.go:72-108) twenty 1-cpu pods; limits.cpu = 36 on the
    heavier pool of the 1..8-cpu catalogue. The 3-cpu pods open four claims that keep the 8-cpu type (36 -> 28 -> 20 -> 12 -> 4), then
    one under the list narrowed to the types of at most 4 cpu, then claims of the second pool; the 1-cpu pods that follow fill the
    room the first four claims have left."""
    pools = [fx.node_pool("first", weight=10, limits={"cpu": "36"}), fx.node_pool("second")]
    pods = [fx.pod(requests={"cpu": "3"}) for _ in range(12)] + [fx.pod(requests={"cpu": "1"}) for _ in range(20)]
    return fx.problem(fx.fake_instance_types(8), pools, pods)


def early_claim_took_a_pod_after_a_later_stage(prob, res):
    """Read off a result: some claim of pool "first" whose options are all of at most 4 cpu holds a 3-cpu pod — it was opened under the
    narrowed list while the 3-cpu pods were in the queue — and some claim of that pool that still lists the 8-cpu type (opened under
    the full list; lists only narrow) holds a 1-cpu pod. Every 3-cpu pod is popped before every 1-cpu pod, so that claim received the
    1-cpu pod after the narrower claim existed."""
    cpus = cpu_of(prob)
    size = {p["uid"]: p["requests"]["cpu"] for p in prob["pods"]}
    first = [c for c in res["newNodeClaims"] if c["nodePool"] == "first"]
    narrow = [c for c in first if max_cpu(c, cpus) <= 4 and any(size[u] == "3" for u in c["pods"])]
    early = [c for c in first if max_cpu(c, cpus) == 8 and any(size[u] == "1" for u in c["pods"])]
    return bool(narrow) and bool(early)


# ---- 6: four rows of class slots; the HBM plans -----------------------------------------------------------------------------------

def many_classes_problem(seed=0):
    """Ninety pod classes of ONE size (selectors on zone / capacity type / arch in every combination, with and without a toleration):
    equal requests leave the queue order to the uids, so all classes are live at once — more than 64: the kernel with four rows of class
    slots — while the heavier, tainted pool's cpu limit narrows its list (kwok cpu sizes 1 .. 256: 600 -> 344 -> 88 -> 24 -> 8 -> 0)."""
    rng = random.Random(9300 + seed)
    its = fx.kwok_catalog(144); zones = list(fx.KWOK_ZONES)
    archs = sorted({v for it in its for r in it["requirements"] if r["key"] == fx.ARCH for v in r["values"]})
    pools = [fx.node_pool("limited", weight=10, limits={"cpu": "600"}, taints=[{"key": "dedicated", "value": "x", "effect": "NoSchedule"}]), fx.node_pool("catch-all")]
    for np_ in pools: np_["nodeClassLabelKey"] = "karpenter.kwok.sh/kwoknodeclass"
    classes, seen = [], set()
    while len(classes) < 90:
        sel = {}
        if rng.random() < 0.6: sel[fx.ZONE] = rng.choice(zones)
        if rng.random() < 0.5: sel[fx.CAPACITY_TYPE] = rng.choice(["spot", "on-demand"])
        if rng.random() < 0.5: sel[fx.ARCH] = rng.choice(archs)
        if rng.random() < 0.3: sel[fx.OS] = "linux"
        tol = rng.choice([None, [{"key": "dedicated", "operator": "Exists"}]])
        key = (tuple(sorted(sel.items())), str(tol))
        if key in seen: continue
        seen.add(key)
        classes.append(dict(requests={"cpu": "2", "memory": "1Gi"}, node_selector=sel or None, tolerations=tol))
    pods = [fx.pod(**classes[i % 90]) for i in range(90)] + [fx.pod(**rng.choice(classes)) for _ in range(1400)]
    return fx.problem(its, pools, pods, well_known=fx.KWOK_WELL_KNOWN)


def escalation_problem(n_claims):
    """`n_claims` 7-cpu pods, one claim each on the 1..8-cpu catalogue — more in-flight claims than the LDS plan holds, so the solve
    ends with reason 26 and starts again on the next memory plan (setup() resets the stages) — and a cpu limit on the heavier pool
    that binds inside the first hundred claims of every attempt."""
    pools = [fx.node_pool("first", weight=10, limits={"cpu": "700"}), fx.node_pool("second")]
    pods = [fx.pod(requests={"cpu": "7"}) for _ in range(n_claims)] + [fx.pod(requests={"cpu": "500m"}) for _ in range(300)]
    return fx.problem(fx.fake_instance_types(8), pools, pods)


# ---- 8: more limit stages than template ids ---------------------------------------------------------------------------------------

def power_catalogue():
    """Eight types of 1, 2, 4 .. 128 cpu that hold three pods each."""
    return [fx.fake_instance_type(f"p-{c}", resources={"cpu": str(c), "memory": f"{2 * c}Gi", "pods": "3"}) for c in (1, 2, 4, 8, 16, 32, 64, 128)]


def stage_chain_problem(n_limited):
    """`n_limited` weighted NodePools with limits.cpu = 127 over power_catalogue() and a catch-all pool: small pods, three to a claim, so
    a pool's remaining cpu goes 127 -> 63 -> 31 -> 15 -> 7 -> 3 -> 1 -> 0 and its list narrows SEVEN times (types <= 64, 32, 16, 8,
    4, 2, 1 cpu), one limit stage each. Template ids are below 32: with n_limited + 1 templates there are 31 - n_limited ids for
    stages — three pools need 21 of 28, four pools 28 of 27: the last narrowing of the fourth pool finds no id (reason 29)."""
    pools = [fx.node_pool(f"pool-{i}", weight=50 - 10 * i, limits={"cpu": "127"}) for i in range(n_limited)] + [fx.node_pool("catch-all")]
    pods = [fx.pod(requests={"cpu": "100m", "memory": "64Mi"}) for _ in range(3 * 7 * n_limited + 12)]
    return fx.problem(power_catalogue(), pools, pods)


# ---- 10: seeded fuzz --------------------------------------------------------------------------------------------------------------

def _zones(prob):
    return sorted({v for it in prob["instanceTypes"] for r in it["requirements"] if r["key"] == fx.ZONE for v in r["values"]})


def fuzz_problem(seed, open_catch_all=False):
    """mix_cases.lite_problem with a cpu limit on EVERY NodePool, drawn between 5% and 60% of the batch's total cpu request;
    DaemonSets two times in three and existing nodes one time in two, as existing_node_cases.fuzz_problem adds them.
    open_catch_all: the lightest pool (lite_problem's "catch-all") keeps no limit, so that pods the limited pools turn away have
    somewhere to go."""
    rng = random.Random(35000 + seed)
    prob = lite_problem(rng, rng.choice([30, 200, 900]))
    total = sum(fx.quantity_float(p["requests"]["cpu"]) for p in prob["pods"])
    for np_ in prob["nodePools"]:
        limit = {"cpu": f"{max(1, int(1000 * total * rng.uniform(0.05, 0.60)))}m"}
        if not (open_catch_all and np_["name"] == "catch-all"):
            np_["limits"] = limit
    if rng.random() < 0.5:
        prob = fx.with_existing_nodes(prob, rng.choice([1, 5, 40, 64, 130]), seed=seed, fill=(0.3, 1.0))
    if rng.random() < 0.66:
        prob["daemonSetPods"] = dc.random_daemonsets(rng, _zones(prob))
    return prob


SHAPE_REASONS = set(range(1, 9)) | {20, 21, 25, 26} | set(range(30, 37)) | {100}   # decline.h: setup(), the caches, the claim slots, existing nodes

# The generator above limits EVERY pool, and subtractMax charges a pool the largest type each claim still lists, so in most draws
# the oracle itself leaves pods unschedulable (76 of the seeds 0-79; the cursor engine hands those back with reason 27, which
# engines 11 / 12 do not change) and in most others the existing nodes take every pod. Of the seeds 0-1199 the oracle schedules
# every pod AND opens a NodeClaim in twelve: the first twelve below — chosen by the oracle's results alone. With them: the seeds
# 0-5 (the limit binds, pods stay unschedulable) and the first six seeds whose pods all land on existing nodes (nothing binds).
# So the shares that test_seeded_fuzz asserts — the limit binds in 18 of 24, 12 of those 18 stay on the cursor engine, exactly
# the two thirds asked for — are a property of THIS SELECTION, not of the generator: drawn blindly, about one seed in a hundred
# binds and stays on the cursor engine. What the list does check is parity with the oracle on each seed and the reason of every
# seed that leaves the cursor engine; OPEN_SEEDS below is the unselected complement.
SEEDS = [16, 107, 138, 205, 212, 267, 413, 684, 752, 754, 778, 970] + [0, 1, 2, 3, 4, 5] + [59, 63, 71, 89, 90, 120]
GPU_SEEDS = [16, 138, 212, 413, 684, 778] + [0] + [59]
# fuzz_problem(seed, open_catch_all=True): a contiguous range
OPEN_SEEDS = list(range(24))


def run_fuzz(oracle, lib, seeds, open_catch_all=False):
    """Whatever "auto-limits" runs equals the oracle, and it leaves the cursor engine only for a reason that stands: 27 only when
    the oracle has pod errors, otherwise 29 or a shape reason. Returns (seeds whose limit binds — reason 23 / 24 under
    "auto-nodes", which is "auto" for a problem without existing nodes and differs from "auto-limits" in the limits alone —, how
    many of those "auto-limits" solved on the cursor engine, histogram of the reasons "auto-limits" ended with)."""
    binds, on_cursor, reasons = 0, 0, {}
    problems = ((seed, fuzz_problem(seed, open_catch_all)) for seed in seeds)
    for seed, prob, want, got, on, r in ec.fuzz_cases(oracle, lib, problems, SWITCH.auto, pops=False, mode=SWITCH.mode):
        bound = ec.where(ec.solve(prob, "auto-nodes", lib)) in (("general", 23), ("general", 24))
        binds += bound
        on_cursor += bound and on == "cursor"
        assert on == "cursor" or (r == 27 and want["podErrors"]) or r == 29 or r in SHAPE_REASONS, (seed, got["counters"])
        reasons[r] = reasons.get(r, 0) + 1
    print(f"limits bind in {binds} of {len(seeds)} seeds; auto-limits kept {on_cursor} of those on the cursor engine; reasons {dict(sorted(reasons.items()))}")
    return binds, on_cursor, reasons
