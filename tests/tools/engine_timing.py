"""What the timing tools of the engine settings (tests/tools/*_engines.py; TEST TOOLS, device only) have in common: the import path,
a solve on a FRESH handle timed with the host clock, the leg of one setting and the "digests agree" reduction. A handle that fell
back solves later batches on the general engine at once, so every repeat is a fresh handle and the time is the host clock around its
first Solve() without result download (which ends in a device synchronise)."""
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)


def use_tree(tree):
    """Solve with the karpenter_amd package of another checkout (the problems and the test modules stay this tree's), so that two
    commits are timed on identical inputs. Before the first import of the package."""
    sys.path.insert(0, os.path.abspath(tree))


def solve_fresh(prob, engine, want_results, solver_lib=None):
    """(result, seconds) of one Solve() on a handle of its own."""
    from karpenter_amd.scheduling import NewScheduler
    s = NewScheduler(dict(prob, options=dict(prob["options"], engine=engine)), solver_lib=solver_lib)
    try:
        t = time.perf_counter()
        r = s.Solve(want_results=want_results)
        return r, time.perf_counter() - t
    finally:
        s.close()


def timed_leg(prob, engine, repeats, pods=None, solver_lib=None):
    """One warm-up, `repeats` timed solves, one more with Results for the digest -> (that result, the times, the fields every tool
    prints for a setting; pods: with pods_per_s)."""
    import parity
    solve_fresh(prob, engine, False, solver_lib)
    times = [solve_fresh(prob, engine, False, solver_lib)[1] for _ in range(repeats)]
    r, _ = solve_fresh(prob, engine, True, solver_lib)
    c = r["counters"]
    med = statistics.median(times)
    leg = {"engine": c["engine"], "engineFallbackReason": c["engineFallbackReason"], "claims": c["claims"],
           "solve_s": [round(x, 4) for x in times], "median_s": round(med, 4), "results_digest": parity.results_digest(r)[0]}
    if pods is not None:
        leg["pods_per_s"] = round(pods / med)
    return r, times, leg


def timed_on_one_handle(prob, engine, repeats):
    """ONE handle: a warm-up solve, `repeats` timed solves without result download, one more with Results -> (that result, the
    times, pack_kernel_ms of every timed solve). For settings that do not fall back."""
    from karpenter_amd.scheduling import NewScheduler
    s = NewScheduler(dict(prob, options=dict(prob["options"], engine=engine)))
    try:
        s.Solve(want_results=False)
        times, kernel = [], []
        for _ in range(repeats):
            t = time.perf_counter()
            r = s.Solve(want_results=False)
            times.append(time.perf_counter() - t)
            kernel.append(r["timings"][0]["pack_kernel_ms"])
        return s.Solve(), times, kernel
    finally:
        s.close()


def own_fixtures(name):
    """karpenter_amd/fixtures.py of THIS tree as a module of its own, whichever package use_tree() puts first."""
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "karpenter_amd", "fixtures.py"))
    fx = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fx)
    return fx


def oracle_digest(prob):
    import oracle
    import parity
    return parity.results_digest(oracle.solve(prob))[0]


def digests_agree(legs, want=None):
    """Every leg printed one Results digest (and `want`, the oracle's, when given)."""
    return len({leg["results_digest"] for leg in legs.values()} | ({want} if want is not None else set())) == 1


def claims_by_pool(res):
    pools = {}
    for cl in res["newNodeClaims"]:
        pools[cl["nodePool"]] = pools.get(cl["nodePool"], 0) + 1
    return pools


def over(legs, a, b):
    """median seconds under `a` over median seconds under `b`"""
    return round(legs[a]["median_s"] / legs[b]["median_s"], 2)
