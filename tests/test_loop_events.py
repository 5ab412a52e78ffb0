"""CPU tests of the tail behind the cursor engine's fast loop (karpenter_amd/csrc/fast_engine.h, fast_hot_run): sort-only pods,
new-claim pods, pods of a class without a slot and pods whose claim's move reaches past the window are finished by the loop's
own function and no longer go through the one-pod loop (fast_slow_run). The results and every reported count stay what they were.

Through the host emulation against the oracle and the general engine, with the lanes of every wave-wide call in both orders, on
the three memory plans. `onePodLoopCalls` is the driver's count of fast_slow_run calls (phaseCycles[11], in every build).

One-pod-loop calls at the commit before the tail, on the emulation and on the device alike: 5,638 for config2(20000, 500, 42),
5,545 for config2(26000, 500, 42), 1,534 for config2(3000, 16, 42)."""
import pytest

import limit_cases as lc
import parity
import pod_operator_cases as pc
import unschedulable_cases as uc
from karpenter_amd import fixtures as fx
from karpenter_amd.scheduling import NewScheduler
from test_device_algorithm import emu  # noqa: F401  (fixture)
from test_device_fuzz_all import emu_reversed  # noqa: F401  (fixture)

PLANS = ((0, "cursor"), (1, "cursor-wide"), (2, "cursor-hbm"))
# pods, types, NodeClaims, fullEvaluations (the select steps the engine reported before the tail: one per pod and the extra ones),
# at least this many slow sorts, the one-pod loop's calls stay below this (None: below the claim count)
SHAPES = [(20000, 500, 57, 20000, 3000, 1500), (26000, 500, 73, 26238, 3000, 1500), (3000, 16, 525, 7005, 0, None)]


def with_options(prob, **kw):
    return dict(prob, options=dict(prob["options"], **kw))


@pytest.fixture(scope="module")
def wanted(oracle):
    """Per shape, once: the problem, the oracle's digest and evaluation count, the general engine's slowSorts."""
    cache = {}

    def get(pods, types, claims, lib):
        if pods not in cache:
            prob = fx.config2(pods=pods, n_types=types, seed=42)
            want = oracle.solve(prob)
            assert len(want["newNodeClaims"]) == claims
            general = NewScheduler(with_options(prob, engine="general"), solver_lib=lib).Solve()
            assert general["counters"]["engine"] == "general" and parity.results_digest(general)[0] == parity.results_digest(want)[0]
            cache[pods] = {"prob": prob, "digest": parity.results_digest(want)[0], "evals": want["counters"]["binEvaluations"], "slow": general["counters"]["slowSorts"]}
        return cache[pods]
    return get


def check_shape(lib, wanted, pods, types, claims, full, min_slow, cap):
    w = wanted(pods, types, claims, lib)
    assert w["slow"] >= min_slow
    for plan, engine in PLANS:
        got = NewScheduler(with_options(w["prob"], engine=engine), solver_lib=lib).Solve()
        c = got["counters"]
        assert c["engine"] == "cursor" and c["cursorMemoryPlan"] == plan
        assert len(got["newNodeClaims"]) == claims
        assert parity.results_digest(got)[0] == w["digest"]
        assert c["referenceBinEvaluations"] == w["evals"]
        assert c["slowSorts"] == w["slow"]
        assert c["phaseCycles"][21] == full                  # fullEvaluations
        print(f"config2({pods}, {types}) {engine}: one-pod loop calls {c['onePodLoopCalls']}")
        assert c["onePodLoopCalls"] < (claims if cap is None else cap)


@pytest.mark.parametrize("pods,types,claims,full,min_slow,cap", SHAPES)
def test_events_leave_the_one_pod_loop(wanted, emu, pods, types, claims, full, min_slow, cap):
    check_shape(emu, wanted, pods, types, claims, full, min_slow, cap)


@pytest.mark.parametrize("pods,types,claims,full,min_slow,cap", SHAPES)
def test_events_leave_the_one_pod_loop_lanes_reversed(wanted, emu_reversed, pods, types, claims, full, min_slow, cap):
    check_shape(emu_reversed, wanted, pods, types, claims, full, min_slow, cap)


def sixteen_nodepools():
    """fixtures.config4 at a size at which more than 64 pod classes are live at once: the kernels with four rows of class slots."""
    return fx.config4(pods=8000, n_types=200, n_pools=16, seed=42)


def four_rows_ran(prob, lib):
    """The engine reports its rows of class slots only where limits are set (phaseCycles[23], limit_cases.rows): the same problem with
    a limit on every NodePool that never binds, under the setting that takes limits."""
    limited = dict(prob, nodePools=[dict(p, limits={"cpu": "100000000"}) for p in prob["nodePools"]])
    res = NewScheduler(with_options(limited, engine="cursor-limits"), solver_lib=lib).Solve()
    assert res["counters"]["engine"] == "cursor" and lc.stages(res)[0] == 0
    return lc.rows(res) == 4


def test_sixteen_nodepools_four_rows(oracle, emu):
    """A 16-NodePool batch on the kernels with four rows of class slots: the tail's row select of the cursor, the refresh that skips
    rows, the record with four acceptance words — against the oracle and the general engine, on the three memory plans."""
    prob = sixteen_nodepools()
    assert four_rows_ran(prob, emu)
    want = oracle.solve(prob)
    general = NewScheduler(with_options(prob, engine="general"), solver_lib=emu).Solve()
    for plan, engine in PLANS:
        got = NewScheduler(with_options(prob, engine=engine), solver_lib=emu).Solve()
        c = got["counters"]
        assert c["engine"] == "cursor" and c["cursorMemoryPlan"] == plan
        parity.assert_same_results(got, want)
        assert c["referenceBinEvaluations"] == want["counters"]["binEvaluations"] and c["slowSorts"] == general["counters"]["slowSorts"]
        assert c["phaseCycles"][21] == 8161                  # fullEvaluations, as reported before the tail
        print(f"config4(8000, 200, 16) {engine}: one-pod loop calls {c['onePodLoopCalls']}")
        assert c["onePodLoopCalls"] < 1000                   # 5,574 before the tail


# ---- the tail's events meet the handlers of the opt-in engines ----

def test_unschedulable_pod_behind_a_full_order(oracle, emu):
    """Engines 20 / 21: a pod that fits nowhere in the MIDDLE of the queue, behind four claims — the fast loop's tail raises
    FEV_NEWCLAIM, new_claim answers 2, the pod is set aside and the loop's state stands behind it; then the same with more than 64
    classes live (four rows) and failing pods at the head, inside and at the tail of the queue."""
    uc.check_engine(oracle, emu, uc.tail_run_problem())
    uc.check_engine(oracle, emu, uc.many_classes_problem())


def test_limit_excludes_a_type_at_a_new_claim(oracle, emu):
    """Engines 11 / 12: every new claim of the limited pool takes 8 cpu of its 40, the sixth excludes every type and the pods move to
    the second pool (limit stages are created inside FEV_NEWCLAIM); then the four-row problem whose limit narrows the list by stages."""
    res, _ = lc.check_engine(oracle, emu, lc.cpu_chain_problem(True))
    assert lc.stages(res)[1] == 5 and lc.rows(res) == 1   # (five claims open when the limit first excludes a type)
    res, _ = lc.check_engine(oracle, emu, lc.many_classes_problem())
    assert lc.rows(res) == 4 and lc.stages(res)[0] >= 1


def test_pod_operators(oracle, emu):
    """Engines 26 / 27: pods with NotIn requirements, whose new claims carry complement sets."""
    res, _ = pc.check_engine(oracle, emu, pc.zone_notin_problem())
    assert pc.kinds(res, fx.ZONE) == pc.ZONE_NOTIN_KINDS


# ---- the measuring switch ----

def test_without_the_tail_the_results_are_the_same(emu, tmp_path):
    """-DKSOLVE_LOOP_TAIL=0 (every pod that is not plain goes through fast_slow_run, as before the tail: what profiles/loop_events
    measures against) reports the same digest and the same counts, and the one-pod loop's calls of before."""
    import os
    import subprocess
    lib = str(tmp_path / "libksolve_emu_tail0.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-DKSOLVE_LOOP_TAIL=0", "-o", lib,
                           os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu", "ksolve_emu.cpp")])
    for pods, types, calls in ((20000, 500, 5638), (3000, 16, 1534)):
        prob = with_options(fx.config2(pods=pods, n_types=types, seed=42), engine="cursor")
        a, b = NewScheduler(prob, solver_lib=lib).Solve(), NewScheduler(prob, solver_lib=emu).Solve()
        assert parity.results_digest(a)[0] == parity.results_digest(b)[0]
        keys = ("binEvaluations", "referenceBinEvaluations", "slowSorts", "sorts", "pops", "claims")
        assert [a["counters"][k] for k in keys] == [b["counters"][k] for k in keys] and a["counters"]["phaseCycles"][21] == b["counters"]["phaseCycles"][21]
        assert a["counters"]["onePodLoopCalls"] == calls


@pytest.mark.parametrize("at", [1024, 2048])
def test_cancel_at_a_poll_boundary(emu, monkeypatch, at):
    """A Solve() cancelled at a polled block reports the full run stopped there, with the order of the last sort the reference would
    have run: the entries in front of a polled block are not the tail's."""
    prob = fx.config2(pods=20000, n_types=500, seed=42)
    monkeypatch.setenv("KSOLVE_TEST_CANCEL_AT", str(at))
    got = NewScheduler(with_options(prob, engine="cursor"), solver_lib=emu).Solve()
    monkeypatch.delenv("KSOLVE_TEST_CANCEL_AT")
    assert got["timedOut"] and got["scheduledPods"] == at and got["counters"]["engine"] == "cursor"
    parity.assert_same_results(got, NewScheduler(with_options(prob, engine="general", maxSteps=at), solver_lib=emu).Solve())


def test_step_limit_never_enters_the_fast_loop(emu):
    prob = fx.config2(pods=20000, n_types=500, seed=42)
    got = NewScheduler(with_options(prob, engine="cursor", maxSteps=5000), solver_lib=emu).Solve()
    assert got["counters"]["engine"] == "cursor" and got["scheduledPods"] == 5000
    parity.assert_same_results(got, NewScheduler(with_options(prob, engine="general", maxSteps=5000), solver_lib=emu).Solve())
