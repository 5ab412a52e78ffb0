"""CPU tests of the cursor engine's limit stages (csrc/fast_engine.h FastLimits / FastCold::limit_stage, engines "auto-limits" /
"cursor-limits"): through the host emulation of the device code (tests/emu, test infrastructure only), the real C ABI and the real
flattener, against the oracle in claims, instance-type lists, pod assignment and the reference-equivalent evaluation count. The
problems are tests/limit_cases.py's; the device run is tests/test_gpu_cursor_limits.py."""
import pytest

import engine_checks as ec
import limit_cases as lc
import parity
from karpenter_amd import fixtures as fx
from karpenter_amd.scheduling import NewScheduler, SolveBatch, Unsupported
from test_device_algorithm import emu  # noqa: F401  (fixture)


def test_cpu_chain(oracle, emu):
    """Case 1. Alone the pool leaves twenty pods unschedulable: the engine passes the sixth claim's exclusion (where engines 0-10
    stop with 24) and stops at the pod no template takes (27, out of scope). With a second pool the pods move there: the template
    skip, with the hostname numbers of the oracle (same() compares them through the claims)."""
    alone = lc.cpu_chain_problem(False)
    assert len(oracle.solve(alone)["newNodeClaims"]) == 5 and len(oracle.solve(alone)["podErrors"]) == 20
    lc.check_declined(oracle, emu, alone, 27)
    got, want = lc.check_engine(oracle, emu, lc.cpu_chain_problem(True))
    assert lc.pool_of(want).count("first") == 5 and lc.pool_of(want).count("second") == 10 and not want["podErrors"]
    assert lc.stages(got) == (0, 5)       # no list between "every type" and "none": no stage; the first exclusion with five claims open


def test_nodes_zero(oracle, emu):
    got, want = lc.check_engine(oracle, emu, lc.nodes_zero_problem())
    assert set(lc.pool_of(want)) == {"second"} and len(want["newNodeClaims"]) == 15
    assert lc.stages(got) == (0, None)


def test_two_resources(oracle, emu):
    prob = lc.two_resource_problem()
    got, want = lc.check_engine(oracle, emu, prob)
    cpus = lc.cpu_of(prob)
    limited = [c for c in want["newNodeClaims"] if c["nodePool"] == "limited"]
    # memory bound first: a claim that keeps 8-cpu types but not the 64 GiB ones; cpu later: a claim of at most 2 cpu
    assert any(lc.max_cpu(c, cpus) == 8 and not any(t.startswith("m-8x") for t in c["instanceTypes"]) for c in limited)
    assert any(lc.max_cpu(c, cpus) == 8 and any(t.startswith("m-8x") for t in c["instanceTypes"]) for c in limited)
    assert any(lc.max_cpu(c, cpus) <= 2 for c in limited)
    assert lc.stages(got)[0] == 2 and "open" in lc.pool_of(want)


def test_daemonsets(oracle, emu):
    got, want = lc.check_engine(oracle, emu, lc.daemonset_problem(30))
    assert len(want["newNodeClaims"]) == 5 and all(c["instanceTypes"] == ["cpu-8-mem-64"] for c in want["newNodeClaims"]) and not want["podErrors"]
    assert lc.stages(got) == (1, 3)       # 48 -> 40 -> 32 -> 24: the 32-cpu type leaves the list with three claims open
    # the ten pods of the existing test: the limit does not bind, engines 11 / 12 behave as 7 / 8
    ten = lc.daemonset_problem(10)
    loose = ec.solve(ten, "cursor-limits", emu)
    assert loose["counters"]["engine"] == "cursor" and lc.stages(loose) == (0, None)
    ec.same(loose, oracle.solve(ten), ten)
    got, want = lc.check_engine(oracle, emu, lc.daemonset_overhead_problem())
    assert lc.stages(got)[0] == 1 and set(lc.pool_of(want)) == {"first", "second"}


def test_early_stage_claims_keep_accepting(oracle, emu):
    prob = lc.early_stage_problem()
    got, want = lc.check_engine(oracle, emu, prob)
    assert lc.early_claim_took_a_pod_after_a_later_stage(prob, want)
    assert lc.stages(got) == (1, 4)


def test_four_rows_of_class_slots(oracle, emu):
    prob = lc.many_classes_problem()
    assert len({(str(p.get("nodeSelector")), str(p.get("tolerations"))) for p in prob["pods"][:90]}) == 90
    got, want = lc.check_engine(oracle, emu, prob)
    assert lc.rows(got) == 4              # the kernel says which instantiation ran: more than 64 classes were live at once
    assert lc.stages(got)[0] >= 3 and set(lc.pool_of(want)) == {"limited", "catch-all"}
    assert lc.rows(ec.solve(lc.early_stage_problem(), "cursor-limits", emu)) == 1   # ... and one row where two classes are


def test_memory_plan_1(oracle, emu):
    """More claims than the LDS plan holds: the attempt ends with reason 26 and the solve starts again with the claims' state in
    HBM (plan 1), setup() included — the stages of the first attempt are gone, the second builds its own."""
    got, want = lc.check_engine(oracle, emu, lc.escalation_problem(3200))
    assert (got["counters"]["cursorMemoryPlan"], got["counters"]["cursorAttempts"]) == (1, 2)
    assert lc.stages(got)[0] == 1 and lc.pool_of(want).count("first") > 80


def test_memory_plan_2(oracle, emu, monkeypatch):
    """The same problem with plan 1 shrunk below its claims by the test switch KSOLVE_TEST_WIDE_CAP, as
    test_cursor_engine.test_claim_order_in_hbm_above_the_wide_plan does: the second attempt runs with the claim order in HBM too
    (plan 2) — limit_stage, the stage's id in create_entry and the records' template index on that plan."""
    monkeypatch.setenv("KSOLVE_TEST_WIDE_CAP", "1024")
    got, want = lc.check_engine(oracle, emu, lc.escalation_problem(3200))
    assert (got["counters"]["cursorMemoryPlan"], got["counters"]["cursorAttempts"]) == (2, 2)
    assert lc.stages(got)[0] == 1 and lc.pool_of(want).count("first") > 80


def test_with_existing_nodes(oracle, emu):
    prob = fx.with_existing_nodes(lc.cpu_chain_problem(True), 4, seed=1)
    got, want = lc.check_engine(oracle, emu, prob, base="auto-nodes")
    on_nodes = sum(len(e["pods"]) for e in want.get("existingNodes", []))
    assert on_nodes > 0 and set(lc.pool_of(want)) == {"first", "second"}
    assert lc.stages(got)[1] is not None


def test_stage_exhaustion(oracle, emu):
    got, want = lc.check_engine(oracle, emu, lc.stage_chain_problem(3))
    assert lc.stages(got)[0] == 21 and all(lc.pool_of(want).count(f"pool-{i}") == 7 for i in range(3))
    lc.check_declined(oracle, emu, lc.stage_chain_problem(4), 29)


def test_a_hundred_solves_on_one_handle(oracle, emu):
    prob = lc.cpu_chain_problem(True)
    digests, last = ec.digests_of_repeated_solves(emu, prob, "auto-limits", 100, "cursor")
    assert len(digests) == 1
    ec.same(last, oracle.solve(prob), prob)
    # ... and with stages to forget
    prob = lc.stage_chain_problem(3)
    digests, last = ec.digests_of_repeated_solves(emu, prob, "cursor-limits", 20, "cursor")
    assert len(digests) == 1 and lc.stages(last)[0] == 21
    ec.same(last, oracle.solve(prob), prob)


def test_batch(oracle, emu):
    """ksolve_solve_batch over three handles, one of them "auto-limits" (it runs alone through solve()): the digests of solving each
    alone."""
    probs = [(fx.config2(pods=800, n_types=60, seed=91), "auto"), (lc.early_stage_problem(), "auto-limits"), (fx.config2(pods=600, n_types=60, seed=92), "auto")]
    scheds = [NewScheduler(dict(p, options=dict(p["options"], engine=e)), solver_lib=emu) for p, e in probs]
    try:
        for _ in range(2):
            got = SolveBatch(scheds)
            assert [g["counters"]["engine"] for g in got] == ["cursor"] * 3
            for g, (p, e) in zip(got, probs):
                assert parity.results_digest(g)[0] == parity.results_digest(ec.solve(p, e, emu))[0]
                ec.same(g, oracle.solve(p), p)
            assert lc.stages(got[1]) == (1, 4)
    finally:
        for s in scheds:
            s.close()


def test_engines_0_to_10_still_decline(oracle, emu):
    """The parent's behaviour, unchanged: "auto" / "auto-nodes" fall back with 24 and 23, "cursor" / "cursor-nodes" refuse and name the reason; and
    a problem without limits counts the same work under the new names."""
    for prob, reason in ((lc.cpu_chain_problem(True), 24), (lc.nodes_zero_problem(), 23)):
        for engine in ("auto", "auto-nodes"):
            c = ec.solve(prob, engine, emu)["counters"]
            assert (c["engine"], c["engineFallbackReason"]) == ("general", reason)
        for engine in ("cursor", "cursor-nodes"):
            with pytest.raises(Unsupported, match=rf"cursor engine declined the problem \(reason {reason}\)"):
                ec.solve(prob, engine, emu)
    a = ec.solve(fx.config1(), "auto", emu)["counters"]
    for engine in ("auto-limits", "cursor-limits"):
        r = ec.solve(fx.config1(), engine, emu)
        c = r["counters"]
        assert c["engine"] == "cursor" and lc.stages(r) == (0, None)
        assert (c["binEvaluations"], c["phaseCycles"][21], c["slowSorts"], c["referenceBinEvaluations"], c["pops"]) == \
               (a["binEvaluations"], a["phaseCycles"][21], a["slowSorts"], a["referenceBinEvaluations"], a["pops"])


def test_refusal_names_the_reason(emu):
    """A shape reason decided by create() (a host port beside an existing node: 34) is named by "cursor-limits" as by "cursor-nodes"."""
    its = fx.fake_instance_types(8)
    node = fx.state_node("node-0", its[5], "test-zone-1", "on-demand", "default", used={"cpu": "500m", "pods": "1"})
    pods = [fx.pod(requests={"cpu": "900m"}) for _ in range(8)] + [fx.pod(requests={"cpu": "1"}, host_ports=[8080]) for _ in range(2)]
    with pytest.raises(Unsupported, match=r"reason 34"):
        ec.solve(fx.problem(its, [fx.node_pool(limits={"cpu": "10"})], pods, state_nodes=[node]), "cursor-limits", emu)


def test_seeded_fuzz(oracle, emu):
    """lc.SEEDS: 24 seeds PICKED from the oracle's results over the seeds 0-1199 so that the issue's conditions hold (how stands
    beside the list). The shares asserted below are therefore a property of the selection and say nothing about the generator: the
    limit binds in 18 of the 24 — at least half —, and "auto-limits" keeps 12 of those 18 on the cursor engine — exactly two thirds;
    the other 6 end with reason 27 (the oracle leaves pods unschedulable), and in the 6 seeds where nothing binds the cursor engine
    runs under either setting. What the seeds do test: parity with the oracle, and the reason of every seed off the cursor engine."""
    binds, on_cursor, reasons = lc.run_fuzz(oracle, emu, lc.SEEDS)
    assert binds * 2 >= len(lc.SEEDS), (binds, reasons)
    assert on_cursor * 3 >= binds * 2, (binds, on_cursor, reasons)


def test_seeded_fuzz_with_an_open_pool(oracle, emu):
    """The same generator with the catch-all pool left without a limit, over a contiguous range of seeds: pods the limited pools turn
    away have somewhere to go, so far fewer draws end in reason 27 (of the seeds 0-23 the limit binds in 12, and 6 of those stay on
    the cursor engine). No share is asserted here: run_fuzz's own conditions are — equal to the oracle, and off the cursor engine only
    with pod errors in the oracle's result (27), 29 or a shape reason."""
    binds, on_cursor, _ = lc.run_fuzz(oracle, emu, lc.OPEN_SEEDS, open_catch_all=True)
    assert binds > 0 and on_cursor > 0
