"""scheduling.SolveMany (ksolve_solve_many; csrc/solve_calls.h solve_many_plain, csrc/topo_many.h) — the member lists and the checks that
tests/test_solve_many.py runs through the host emulation and tests/test_gpu_solve_many.py on the device, at the same shapes.

The contract under test: every member of the call gets the result Solve() gives the same problem on a fresh handle of its own —
outcome, error text, engine, fallback reason, memory plan, attempts, digest — and members of the spread engine's shape share
launches. A member is (problem, engine setting); its cell is what the engine matrix records per solve (tools/engine_matrix._cell).
fixtures.pod() numbers uids from a process-wide counter and uids are part of the digest: a member's lone solve and its solve as a
member always use the SAME problem document."""
import os
import random
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import engine_checks as ec  # noqa: E402
import engine_matrix as em  # noqa: E402
import mix_cases  # noqa: E402
import operator_cases as oc  # noqa: E402
import parity  # noqa: E402
import spread_filter_cases as sf  # noqa: E402
import spread_limit_cases as sl  # noqa: E402
import spread_node_cases as sn  # noqa: E402
import spread_operator_cases as so  # noqa: E402
import spread_unschedulable_cases as su  # noqa: E402
from karpenter_amd import fixtures as fx  # noqa: E402
from karpenter_amd.scheduling import MANY_STATS, NewScheduler, SolveBatch, SolveMany  # noqa: E402

CELL3 = ("engine", "engineFallbackReason", "digest")


def with_engine(prob, setting):
    return dict(prob, options=dict(prob.get("options", {}), engine=setting))


def open_members(members, lib):
    return [NewScheduler(with_engine(prob, setting), solver_lib=lib) for prob, setting in members]


def close_all(scheds):
    for s in scheds:
        s.close()


def many(scheds):
    """One SolveMany over open schedulers -> (every member's Results or exception, the call's counters)."""
    stats = {}
    out = SolveMany(scheds, errors="return", stats=stats)
    assert len(out) == len(scheds) and set(stats) == set(MANY_STATS), stats
    return out, stats


def cell_of(member):
    """The engine matrix's cell (seven fields) of one member of a SolveMany(errors="return")."""
    return em._cell(exc=member) if isinstance(member, Exception) else em._cell(member)


def lone_cell(lib, prob, setting):
    """The same seven fields of Solve() on a fresh handle of its own. Where it solves, (engine, reason, digest) are
    spread_operator_cases.lone_cell's."""
    try:
        r = ec.solve(prob, setting, lib)
    except Exception as e:
        return em._cell(exc=e)
    cell = em._cell(r)
    assert tuple(cell[f] for f in CELL3) == so.lone_cell(lib, prob, setting)
    return cell


def assert_cells(got, want, names):
    diff = [(names[i], f, got[i][f], want[i][f]) for i in range(len(want)) for f in em.FIELDS if got[i][f] != want[i][f]]
    assert not diff, f"{len(diff)} fields differ (member, field, as a member, alone): {diff[:10]}"


def same_as_oracle(oracle, members, results):
    """Every member that solved equals the oracle (claims, assignment, requirements, nodes, pod errors, evaluations, cost). In place
    on the instance-type lists of DaemonSet problems: cells are taken before."""
    for (prob, _), r in zip(members, results):
        if not isinstance(r, Exception):
            ec.same(r, oracle.solve(prob), prob)


# ---- 1: the engine matrix ---------------------------------------------------------------------------------------------------------------

def matrix_cells(lib, settings=None, probs=None, way="alone"):
    """{cell name: cell} for every problem of the engine matrix (or `probs`) under every setting (or `settings`), the problems of one
    setting opened on fresh handles and solved in ONE SolveMany; named as the record names the lone solves ("…|alone"), or by `way`."""
    probs = em.problems() if probs is None else probs
    out = {}
    for setting in (em.SETTINGS if settings is None else settings):
        opened = []
        for name, prob in probs:
            try:
                opened.append((name, NewScheduler(with_engine(prob, setting), solver_lib=lib)))
            except Exception as e:   # (a problem the host library refuses to open under the setting is its own cell, as in the record)
                out[f"{name}|{setting}|{way}"] = em._cell(exc=e)
        try:
            results, _ = many([s for _, s in opened])
            for (name, _), r in zip(opened, results):
                out[f"{name}|{setting}|{way}"] = cell_of(r)
        finally:
            close_all([s for _, s in opened])
    return out


def recorded_alone(key):
    return {k: v for k, v in em.load(key).items() if k.endswith("|alone")}


# ---- 2: launches are shared -------------------------------------------------------------------------------------------------------------

SHARED_PODS = [60, 80, 100, 120, 140, 160, 180, 200, 220, 240, 270, 300]


def shared_members():
    """Twelve plain topology mixes of 60 to 300 pods, twelve seeds."""
    return [(sl.mix_problem((pods, 144, 1 + i), None), "auto") for i, pods in enumerate(SHARED_PODS)]


def check_shared(oracle, lib):
    members = shared_members()
    want = [lone_cell(lib, p, s) for p, s in members]
    scheds = open_members(members, lib)
    try:
        results, stats = many(scheds)
    finally:
        close_all(scheds)
    assert (stats["spread_launches"], stats["spread_members"], stats["alone_members"], stats["general_members"]) == (1, 12, 0, 0), stats
    got = [cell_of(r) for r in results]
    assert_cells(got, want, list(range(12)))
    assert all(c["engine"] == "spread" and c["engineFallbackReason"] == 0 for c in got), got
    same_as_oracle(oracle, members, results)
    # what the call is for: the same list through SolveBatch runs every member on the general engine
    assert [c[0] for c in so.batch_cells(lib, [p for p, _ in members], "auto")] == ["general"] * 12


# ---- 3: all six flavours in one call ----------------------------------------------------------------------------------------------------

def flavour_members():
    plain = fx.config1()
    return [(sl.mix_problem((300, 144, 1), None), "auto"),                       # ksolve_pack_topo_many
            (sn.mix_problem((300, 144, 1), 5), "auto-nodes-spread"),             # ..._nodes_many
            (su.chain_web_problem(), "auto-unschedulable-spread"),               # ..._many_u
            (su.chain_nodes_problem(), "auto-unschedulable-spread"),             # ..._nodes_many_u
            (sf.by_template_problem(), "auto-filters-spread"),                   # ..._many_f
            (sf.node_problem(), "auto-filters-spread"),                          # ..._nodes_many_f
            (so.counted_problem(), "auto-operators-spread"),                     # complement templates: the plain kernel
            (so.daemonset_problem(), "auto-operators-spread"),                   # ... with DaemonSets
            (mix_cases.lite_problem(random.Random(11), 80), "auto"),             # the cursor engine
            (oc.min_values_problem(), "auto"),                                   # the general engine
            (dict(plain, pods=[], podGroups=[]), "auto")]                        # no pods
FLAVOUR_ENGINES = ["spread"] * 8 + ["cursor", "general", "general"]


def check_flavours(oracle, lib, members, results, stats, want):
    assert stats["spread_launches"] == 6 and stats["spread_members"] == 8, stats
    got = [cell_of(r) for r in results]
    assert_cells(got, want, list(range(len(members))))   # (in input order: the digests below are pairwise distinct, so a permutation cannot hide)
    assert [c["engine"] for c in got] == FLAVOUR_ENGINES, [(c["engine"], c["engineFallbackReason"], c["error"]) for c in got]
    assert len({c["digest"] for c in got}) == len(got)
    same_as_oracle(oracle, members, results)


# ---- 4: hand-backs and refusals inside the call ------------------------------------------------------------------------------------------

def handback_members():
    plain = fx.config1()
    return [(su.chain_web_problem(), "auto"),                                          # reason 27 to the general engine
            (sf.preference_problem(), "auto-filters-spread"),                          # 41
            (sf.pod_notin_problem(), "auto-filters-spread"),                           # 4
            (sf.too_many_slots_problem(), "auto-filters-spread"),                      # 43
            (sl.mix_problem((300, 144, 1), {"cpu": "100"}), "spread"),                 # Unsupported: declined, reason 24
            (dict(plain, pods=plain["pods"][:40]), "spread"),                          # Unsupported: outside its shape
            (sl.mix_problem((80, 144, 21), None), "auto"), (sl.mix_problem((120, 144, 22), None), "auto"), (sl.mix_problem((160, 144, 23), None), "auto")]
HANDBACK_WANT = [("general", 27), ("general", 41), ("general", 4), ("general", 43), "spread engine declined the problem (reason 24)",
                 "spread engine requested for a problem outside its shape", ("spread", 0), ("spread", 0), ("spread", 0)]


def check_handbacks(oracle, lib, members, results, stats, want):
    got = [cell_of(r) for r in results]
    assert_cells(got, want, list(range(len(members))))
    for c, w in zip(want, HANDBACK_WANT):   # the lone cells are what the issue says they are
        if isinstance(w, str):
            assert c["outcome"] == "Unsupported" and w in c["error"], c
        else:
            assert (c["outcome"], c["engine"], c["engineFallbackReason"]) == ("ok",) + w, c
    # The counts the lone cells imply, with where each reason is found. Refused: the two Unsupported cells. On the general engine's
    # launch: the four "general" cells. Reason 41 under a setting with the filters is the host's: create() sees the relaxation rows of
    # the pod with preferences and never enables the spread engine (ksolve_impl.h create(), DECLINE_TOPO_PREFERENCES), so that member
    # is no member of the spread launches and no hand-back. Reasons 27 (a pod the first pass cannot place), 4 (FastCold::setup finds the
    # class that is not positive) and 43 (setup_filters runs out of slots) are the kernel's: three hand-backs. The plain problem under
    # "spread" is refused by the host before anything runs; the limited mix under "spread" is declined inside its launch. So the
    # launches hold the nine members less those two: 3 solved + 1 declined + 3 handed back = 7.
    general = sum(c["engine"] == "general" for c in want)
    by_kernel = sum(c["engine"] == "general" and c["engineFallbackReason"] in (27, 4, 43) for c in want)
    assert stats["refused"] == sum(c["outcome"] == "Unsupported" for c in want) == 2, stats
    assert stats["general_members"] == general == 4, stats
    assert stats["handed_back"] == by_kernel == 3, stats
    assert stats["spread_members"] == 7 and stats["spread_launches"] == 2, stats   # (the plain kernel, and the one with the filters)
    assert stats["alone_members"] == 0 and stats["cursor_members"] == 0 and stats["probe_members"] == 0, stats
    same_as_oracle(oracle, members, results)


# ---- 5: more members than CUs -----------------------------------------------------------------------------------------------------------

N_CROWD = 264


def crowd_members(pods=24):
    return [(fx.problem(fx.fake_instance_types(12), [fx.node_pool()], mix_cases.mix(random.Random(31000 + seed), pods)), "auto") for seed in range(N_CROWD)]


def check_crowd(lib, members):
    """-> (the call's counters, the seconds handle creation and the SolveMany call took — the lone solves are outside that clock)."""
    import time
    want = [lone_cell(lib, p, s) for p, s in members]
    t = time.perf_counter()
    scheds = open_members(members, lib)
    try:
        results, stats = many(scheds)
        seconds = time.perf_counter() - t
    finally:
        close_all(scheds)
    assert stats["spread_launches"] == 1 and stats["spread_members"] == N_CROWD, stats
    assert_cells([cell_of(r) for r in results], want, list(range(N_CROWD)))
    return stats, seconds


# ---- 6: the same handles again ----------------------------------------------------------------------------------------------------------

def passes_on_same_handles(lib, members, passes=3):
    """(the lone cells, [(results, stats)] of `passes` SolveMany calls on the SAME handles). The lone solves come first: the
    reference is computed once and shared by the tests of the list."""
    want = [lone_cell(lib, p, s) for p, s in members]
    scheds = open_members(members, lib)
    try:
        return want, [many(scheds) for _ in range(passes)]
    finally:
        close_all(scheds)


def check_again(runs):
    """Each later pass gives the digests, engines and reasons (and outcomes, texts) of the first — run-order rings, set-aside lists and
    node counters start over, tw.enabled is kept after reason 27 and cleared after the others."""
    cells = [[em._cell(exc=r) if isinstance(r, Exception) else em._cell(r) for r in results] for results, _ in runs]
    for got in cells[1:]:
        diff = [(i, f, got[i][f], cells[0][i][f]) for i in range(len(got)) for f in ("outcome", "error") + CELL3 if got[i][f] != cells[0][i][f]]
        assert not diff, diff
    # a member handed back with reason 27 goes through the spread engine's launch again, one handed back for its shape does not
    # (a spread-only member the engine declines stays a spread member too: a refusal changes nothing on the handle)
    for_shape = runs[0][1]["handed_back"] - sum(c["engine"] == "general" and c["engineFallbackReason"] in (27, 100) for c in cells[0])
    for _, later in runs[1:]:
        assert later["spread_members"] == runs[0][1]["spread_members"] - for_shape, (runs[0][1], later)
    return cells


# ---- 7: seeded fuzz ---------------------------------------------------------------------------------------------------------------------

def check_fuzz(oracle, lib, seeds, calls):
    """spread_filter_cases.fuzz_problem under "auto-filters-spread", the seeds dealt over `calls` SolveMany calls: every member equals
    the oracle (pops included) and its lone cell; as many members on the spread engine as lone solves, at least three quarters of the
    seeds (what test_seeded_fuzz of the filter tests holds the lone solves to)."""
    per = (len(seeds) + calls - 1) // calls
    on_spread = lone_on_spread = 0
    for k in range(calls):
        members = [(sf.fuzz_problem(seed), sf.AUTO) for seed in seeds[k * per:(k + 1) * per]]
        want = [lone_cell(lib, p, s) for p, s in members]
        scheds = open_members(members, lib)
        try:
            results, stats = many(scheds)
        finally:
            close_all(scheds)
        got = [cell_of(r) for r in results]
        assert_cells(got, want, seeds[k * per:(k + 1) * per])
        for (prob, _), r in zip(members, results):
            assert not isinstance(r, Exception), r
            o = oracle.solve(prob)
            ec.same(r, o, prob, sf.SWITCH.mode)
            ec.same_pops(r, o)
        on_spread += sum(c["engine"] == "spread" for c in got)
        lone_on_spread += sum(c["engine"] == "spread" for c in want)
        assert stats["spread_members"] - stats["handed_back"] == sum(c["engine"] == "spread" for c in got), stats
    assert on_spread == lone_on_spread and 4 * on_spread >= 3 * len(seeds), (on_spread, lone_on_spread, len(seeds))
    return on_spread
