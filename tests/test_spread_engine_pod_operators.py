"""CPU tests of the spread engine's pod operators (csrc/topo_engine.h "The spread engine's pod operators": the phantom layout under
topology, the widened filter terms of setup_filters, claim_cut's reading of a guard bit; csrc/fast_engine.h FastCold::setup; engines
"auto-pod-operators-spread" / "spread-pod-operators", 29 / 30): through the host emulation of the device code (tests/emu, test
infrastructure only), the real C ABI and the real flattener, against the oracle in claims, instance-type lists, claim requirements, pod
assignment, pod errors, queue pops and the reference-equivalent evaluation count. The problems are tests/spread_pod_operator_cases.py's;
the device run is tests/test_gpu_spread_pod_operators.py."""
import os
import subprocess

import engine_checks as ec
import pod_operator_cases as pc
import solve_many_cases as sm
import spread_filter_cases as sf
import spread_operator_cases as so
import spread_pod_operator_cases as sp
import test_engine_matrix as tem
from test_device_algorithm import emu  # noqa: F401  (fixture)

Z1, Z2, Z3 = sp.ZONES


def pair(oracle, lib, prob, twin):
    """A problem with negative pods through the common check and its positive twin under 30 against the oracle -> the oracle's spread
    pods per zone of each; the engine's equal them (the results are equal)."""
    _, want = sp.check_engine(oracle, lib, prob)
    want2 = oracle.solve(twin)
    got2 = ec.solve(twin, sp.ONLY, lib)
    assert ec.where(got2) == ("spread", 0), got2["counters"]
    sp.SWITCH.same(got2, want2, twin)
    return sp.by_zone(want, prob), sp.by_zone(want2, twin)


def test_lone_notin_pod_beside_a_spread(oracle, emu):
    sp.check_engine(oracle, emu, pc.spread_problem())


def test_spread_pods_carry_the_notin(oracle, emu):
    """Zones 1 and 2 only, and the skew over the two supported domains: 4 / 4."""
    prob = sp.own_notin_problem()
    want = oracle.solve(prob)
    assert sp.by_zone(want, prob) == {Z1: 4, Z2: 4}
    got, _ = sp.check_engine(oracle, emu, prob, want=want)
    assert sp.by_zone(got, prob) == {Z1: 4, Z2: 4}


def test_counted_but_not_concrete(oracle, emu):
    """A complement set that pods left — one dictionary value and the phantom bit — counts for nothing; In [test-zone-3] counts."""
    assert pair(oracle, emu, sp.counted_problem(), sp.counted_problem("In")) == ({Z1: 2, Z2: 2, Z3: 2}, {Z1: 3, Z2: 3})


def test_notin_term_on_an_undefined_key(oracle, emu):
    """capacity-type NotIn [spot] passes a claim that does not define the key; In [on-demand] fails there. The In twin is a filter
    problem of 24 / 25: it runs under 30 as well."""
    assert pair(oracle, emu, sp.undefined_term_problem(), sp.undefined_term_problem("In")) == (sf.COUNTED, sf.NOT_COUNTED)


def test_notin_pod_defines_the_key(oracle, emu):
    """claim_cut: a guard bit over a field narrower than all ones on a key the template leaves undefined is a defined key."""
    prob, twin = sp.defined_by_notin_problem(), sp.defined_by_notin_problem(False)
    want, want2 = oracle.solve(prob), oracle.solve(twin)
    assert sp.by_zone(want, prob) != sp.by_zone(want2, twin)
    assert sp.by_zone(want, prob) == {Z2: 2, Z3: 2}
    got, _ = sp.check_engine(oracle, emu, prob, want=want)
    assert sp.by_zone(got, prob) == {Z2: 2, Z3: 2}
    got2 = ec.solve(twin, sp.ONLY, emu)
    assert ec.where(got2) == ("spread", 0)
    sp.SWITCH.same(got2, want2, twin)


def test_two_dictionary_key_groups(oracle, emu):
    prob = sp.two_keys_problem()
    got, want = sp.check_engine(oracle, emu, prob)
    assert Z3 not in sp.by_zone(want, prob) and sum(sp.by_zone(got, prob).values()) == 30


def test_affinity_and_anti_affinity(oracle, emu):
    sp.check_engine(oracle, emu, sp.affinity_problem())


def test_does_not_exist_beside_a_spread(oracle, emu):
    got, want = sp.check_engine(oracle, emu, sp.dne_problem(), reason=8)
    assert ("DoesNotExist", ()) in pc.kinds(want, "special") and pc.kinds(got, "special") == pc.kinds(want, "special")


def test_does_not_exist_term(oracle, emu):
    """The owners' term is special DoesNotExist: it fails a claim that defines the key and passes one that leaves it undefined."""
    prob, twin = sp.dne_term_problem(), sp.dne_term_problem(False)
    got, want = sp.check_engine(oracle, emu, prob, reason=8)
    got2, want2 = sp.check_engine(oracle, emu, twin, reason=8)
    assert sp.by_zone(want, prob) == sf.NOT_COUNTED == sp.by_zone(got, prob)
    assert sp.by_zone(want2, twin) == sf.COUNTED == sp.by_zone(got2, twin)


def test_zone_exists_over_pools_that_define_the_zone(oracle, emu):
    sp.check_engine(oracle, emu, sp.exists_problem())


def errors_of(res):
    return sorted(e["code"] for e in res["podErrors"].values())


def test_unschedulable_pods(oracle, emu):
    """Topology (3) for a NotIn that excludes every zone and for a DoesNotExist owner; Incompatible (2) in front of Topology."""
    got, want = sp.check_unschedulable(oracle, emu, sp.no_zone_problem())
    assert errors_of(want) == [3, 3] == errors_of(got)
    got, want = sp.check_unschedulable(oracle, emu, sp.dne_owner_problem(), reason=8)
    assert errors_of(want) == [3, 3] == errors_of(got)
    got, want = sp.check_unschedulable(oracle, emu, sp.incompatible_problem())
    assert errors_of(want) == [2, 2, 2, 2] == errors_of(got)


def test_limit_stage(oracle, emu):
    got, want = sp.check_engine(oracle, emu, sp.limit_problem())
    assert ("NotIn", ("test-zone-1", "test-zone-2")) in pc.kinds(got, sp.fx.ZONE, "not-zone-1")


def test_daemonset_overhead(oracle, emu):
    sp.check_engine(oracle, emu, sp.daemonset_problem())


def test_still_declined(oracle, emu):
    """Existing nodes with negative pods (4), pod-side Gt (1), the by-design declines of the pod operators as topology batches
    (9-12), a filter beyond the slots (43). A filter TERM with Gt is a pod with Gt: the host names 1 before the kernel, whose 43 for a
    bounded term no batch can reach."""
    sp.check_declined(oracle, emu, sp.nodes_problem(), 4)
    sp.check_declined(oracle, emu, sp.pod_gt_problem(), 1)
    for make, reason in sp.BY_DESIGN:
        sp.check_declined(oracle, emu, sp.topology_twin(make()), reason)
    sp.check_declined(oracle, emu, sp.filter_gt_problem(), 1)
    sp.check_declined(oracle, emu, sp.too_many_slots_problem(), 43)
    sp.check_engine(oracle, emu, sp.too_many_slots_problem(32))   # (thirty-two fit)
    sp.check_declined(oracle, emu, sf.too_many_slots_problem(), 43)   # a positive batch keeps the sixteen slots of 24 / 25


def test_old_settings_stay_as_they_are(emu):
    """Values 0-28 keep every outcome: the two checks that name it."""
    assert sp.lone_cell(emu, pc.spread_problem(), "auto-pod-operators")[:2] == ("general", 4)
    for engine in ("auto-operators-spread", "auto-unschedulable-spread", "auto-filters-spread"):
        assert sp.lone_cell(emu, so.pod_notin_problem(), engine)[:2] == ("general", 4), engine
    assert "spread engine declined the problem (reason 4)" in ec.refusal(so.pod_notin_problem(), "spread-filters", emu)


def test_positive_batches_are_unchanged(emu):
    """No negative class, no negative term: the fields, the engine, the reason and the digest of 24 / 25."""
    for i, prob in enumerate(sp.positive_problems()):
        assert sp.lone_cell(emu, prob, sp.AUTO) == sp.lone_cell(emu, prob, "auto-filters-spread"), i
        assert sp.lone_cell(emu, prob, sp.ONLY) == sp.lone_cell(emu, prob, "spread-filters"), i


# rows 29 and 30 in test_engine_matrix.ENGINE_TABLE's columns (s-pod-ops in front of the name), the row a value past the table decodes
# to, and three engine_value lookups
ROWS_29_31 = """\
29 0 0 1 0 1 1 1 1 1 1 1 1 1 1 1 auto-pod-operators-spread
30 3 0 0 0 0 1 0 1 0 1 0 1 1 0 1 spread-pod-operators
31 2 0 0 0 0 0 0 0 0 0 0 0 0 0 0 -
29 30 0
"""   # (the last line: auto-pod-operators-spread, spread-pod-operators, no-such-name)


def test_rows_of_the_second_engine_table(tmp_path):
    """csrc/engine_setting.h from a small program, as test_engine_matrix reads it: values 0-28 print what ENGINE_TABLE pins — 28 stays
    the value without a row it was — and none of them carries the new switch; 29 / 30 are the rows behind it (26 and 25 with the
    switch), their names map back, 31 is past the table."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "rows.cpp"
    src.write_text('#include <cstdio>\n#include "engine_setting.h"\nstatic void row(int v, const ksi::EnginePolicy& p, bool more) {\n'
                   '  printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d ", v, (int)p.run, p.first_plan, p.pick_plan, p.pair, p.nodes, p.spread_nodes, p.limits, p.spread_limits,\n'
                   '         p.operators, p.spread_operators, p.unschedulable, p.spread_unschedulable, p.spread_filters, p.pod_operators);\n'
                   '  if (more) printf("%d ", p.spread_pod_operators);\n  printf("%s\\n", p.name ? p.name : "-");\n}\n'
                   'int main() { for (unsigned v = 0; v <= 28; ++v) { if (ksi::engine_policy(v).spread_pod_operators) return 1; row((int)v, ksi::engine_policy(v), true); }\n'
                   '  for (unsigned v = 29; v <= 31; ++v) row((int)v, ksi::engine_policy(v), true);\n'
                   '  printf("%u %u %u\\n", ksi::engine_value("auto-pod-operators-spread"), ksi::engine_value("spread-pod-operators"), ksi::engine_value("no-such-name")); }\n')
    exe = tmp_path / "rows"
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(root, "karpenter_amd", "csrc"), "-o", str(exe), str(src)])
    out = subprocess.check_output([str(exe)], text=True).splitlines()
    assert out[:29] == tem.ENGINE_TABLE.splitlines()[:29]
    assert out[29:] == ROWS_29_31.splitlines()
    # 29 is 26 and 30 is 25 but for the switch and the name
    for new, old in ((29, 26), (30, 25)):
        assert out[new].split()[1:15] == out[old].split()[1:15]


def test_repeated_solves(emu):
    for prob in (sp.defined_by_notin_problem(), sp.no_zone_problem()):
        digests, _ = ec.digests_of_repeated_solves(emu, prob, sp.ONLY, 3, "spread")
        assert len(digests) == 1


def test_members_of_one_solve_many(oracle, emu):
    """A member whose handle carries the switch runs in a launch of its own; its cell is the lone solve's."""
    members = sp.many_members()
    want = [sm.lone_cell(emu, p, s) for p, s in members]
    scheds = sm.open_members(members, emu)
    try:
        results, stats = sm.many(scheds)
    finally:
        sm.close_all(scheds)
    sm.assert_cells([sm.cell_of(r) for r in results], want, list(range(len(members))))
    assert [ec.where(r) for r in results] == [("spread", 0)] * 3 and stats["alone_members"] == 3, stats
    sm.same_as_oracle(oracle, members, results)


def test_seeded_fuzz(oracle, emu):
    """120 seeds of sp.fuzz_problem: each carries a negative pod, is ("general", 4) under "auto-pod-operators", and equals the oracle
    under "auto-pod-operators-spread" — pod errors and queue pops included; at least four of five end on the spread engine with
    reason 0, the others leave it with a reason of sp.FUZZ_REASONS."""
    for seed in sp.FUZZ_SEEDS:
        assert sp.lone_cell(emu, sp.fuzz_problem(seed), sp.BASE)[:2] == ("general", 4), seed
    on_spread, rest, errors = sp.run_fuzz(oracle, emu, sp.FUZZ_SEEDS)
    assert on_spread * 5 >= len(sp.FUZZ_SEEDS) * 4, (on_spread, rest)
    assert errors >= 5, errors
