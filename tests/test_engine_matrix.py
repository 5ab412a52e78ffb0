"""The engine option, pinned (CPU; tests/test_gpu_engine_matrix.py on the device): every problem of tests/tools/engine_matrix.py under
every value of ksolve_options.engine, alone and in a batch, through the host emulation and the real host library, against the record
in tests/golden/engine_matrix.json — taken from the commit before the option was decoded through csrc/engine_setting.h's table. Cell
by cell and field by field: outcome, full error text, engine, fallback reason, memory plan, attempts, Results digest. No cell is skipped.
The later settings (18-27, 29, 30, 32, 33) have a record of their own, tests/golden/engine_matrix_late.json, with SolveMany as a third
way beside alone and batch: taken from the commit before Solve, SolveBatch and SolveMany were put on the steps of csrc/solve_calls.h."""
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import engine_matrix as em  # noqa: E402
from test_device_algorithm import emu  # noqa: F401,E402  (fixture)


@pytest.fixture(scope="module")
def matrix(emu):
    return em.build_matrix(emu)


def test_every_cell_equals_the_record(matrix):
    want = em.load("emulation")
    assert len(want) == len(em.problems()) * len(em.SETTINGS) * 2
    diff = em.differences(matrix, want)
    assert not diff, f"{len(diff)} fields differ (cell, field, got, recorded): {diff[:12]}"


def test_a_value_past_the_table_is_the_cursor_engine_alone(matrix):
    """17 has no row of its own: the cursor engine only, as "cursor" (2) — the same outcome, error text, engine, reason and digest in
    every cell — except that the library does not choose its first memory plan, as before there was a table."""
    names = [n for n, _ in em.problems()]
    for n in names:
        for how in ("alone", "batch"):
            a, b = matrix[f"{n}|17|{how}"], matrix[f"{n}|cursor|{how}"]
            if (n, how) == ("escalation-open", "alone"):   # (in a batch both get to plan 1 before the solve that counts: one attempt each)
                assert (a["cursorAttempts"], b["cursorAttempts"]) == (2, 1)
                a = dict(a, cursorAttempts=1)
            assert a == b, (n, how, a, b)


def test_the_record_exercises_what_it_is_for():
    """Every run kind, each of the five switches changing an outcome, each refusal message family, the first-plan choice, and the
    batch path's "alone" and "handed back" branches have at least one recorded cell."""
    missing = [claim for claim, cells in em.coverage(em.load("emulation")).items() if not cells]
    assert not missing, missing


@pytest.fixture(scope="module")
def late_matrix(emu):
    return em.build_late(emu)


def test_every_late_cell_equals_the_record(late_matrix):
    """Settings 18-27, 29, 30, 32 and 33 over em.late_problems(), alone, in a batch and in one SolveMany, against
    tests/golden/engine_matrix_late.json — taken from the commit before the three call ladders were put on the steps of
    csrc/solve_calls.h. No cell is skipped."""
    want = em.load("emulation", em.LATE_FIXTURE)
    assert len(want) == len(em.late_problems()) * len(em.LATE_SETTINGS) * 3 == 462
    diff = em.differences(late_matrix, want)
    assert not diff, f"{len(diff)} fields differ (cell, field, got, recorded): {diff[:12]}"


def test_late_many_equals_alone_cell_for_cell(late_matrix):
    many = {k[:-len("many")] + "alone": v for k, v in late_matrix.items() if k.endswith("|many")}
    assert len(many) == 154
    diff = em.differences(many, {k: v for k, v in late_matrix.items() if k.endswith("|alone")})
    assert not diff, f"{len(diff)} fields differ (cell, field, as a member, alone): {diff[:12]}"


def test_the_late_record_exercises_what_it_is_for():
    missing = [claim for claim, cells in em.late_coverage(em.load("emulation", em.LATE_FIXTURE)).items() if not cells]
    assert not missing, missing


# every row of csrc/engine_setting.h's table, the row a value past the table decodes to, and six engine_value lookups
# (value, run, first plan, pick, pair, nodes, s-nodes, limits, s-limits, ops, s-ops, unsched, s-unsched, s-filters, pod-ops, s-pod-ops, name)
ENGINE_TABLE = """\
0 0 0 1 0 0 0 0 0 0 0 0 0 0 0 0 auto
1 1 0 0 0 0 0 0 0 0 0 0 0 0 0 0 general
2 2 0 1 0 0 0 0 0 0 0 0 0 0 0 0 cursor
3 2 1 0 0 0 0 0 0 0 0 0 0 0 0 0 cursor-wide
4 2 2 0 0 0 0 0 0 0 0 0 0 0 0 0 cursor-hbm
5 2 0 0 1 0 0 0 0 0 0 0 0 0 0 0 cursor-pair
6 3 0 0 0 0 0 0 0 0 0 0 0 0 0 0 spread
7 0 0 1 0 1 0 0 0 0 0 0 0 0 0 0 auto-nodes
8 2 0 1 0 1 0 0 0 0 0 0 0 0 0 0 cursor-nodes
9 0 0 1 0 1 1 0 0 0 0 0 0 0 0 0 auto-nodes-spread
10 3 0 0 0 0 1 0 0 0 0 0 0 0 0 0 spread-nodes
11 0 0 1 0 1 0 1 0 0 0 0 0 0 0 0 auto-limits
12 2 0 1 0 1 0 1 0 0 0 0 0 0 0 0 cursor-limits
13 0 0 1 0 1 1 1 1 0 0 0 0 0 0 0 auto-limits-spread
14 3 0 0 0 0 1 0 1 0 0 0 0 0 0 0 spread-limits
15 0 0 1 0 1 1 1 1 1 0 0 0 0 0 0 auto-operators
16 2 0 1 0 1 0 1 0 1 0 0 0 0 0 0 cursor-operators
17 2 0 0 0 0 0 0 0 0 0 0 0 0 0 0 -
18 0 0 1 0 1 1 1 1 1 1 0 0 0 0 0 auto-operators-spread
19 3 0 0 0 0 1 0 1 0 1 0 0 0 0 0 spread-operators
20 0 0 1 0 1 1 1 1 1 1 1 0 0 0 0 auto-unschedulable
21 2 0 1 0 1 0 1 0 1 0 1 0 0 0 0 cursor-unschedulable
22 0 0 1 0 1 1 1 1 1 1 1 1 0 0 0 auto-unschedulable-spread
23 3 0 0 0 0 1 0 1 0 1 0 1 0 0 0 spread-unschedulable
24 0 0 1 0 1 1 1 1 1 1 1 1 1 0 0 auto-filters-spread
25 3 0 0 0 0 1 0 1 0 1 0 1 1 0 0 spread-filters
26 0 0 1 0 1 1 1 1 1 1 1 1 1 1 0 auto-pod-operators
27 2 0 1 0 1 0 1 0 1 0 1 0 0 1 0 cursor-pod-operators
28 2 0 0 0 0 0 0 0 0 0 0 0 0 0 0 -
29 0 0 1 0 1 1 1 1 1 1 1 1 1 1 1 auto-pod-operators-spread
30 3 0 0 0 0 1 0 1 0 1 0 1 1 0 1 spread-pod-operators
31 2 0 0 0 0 0 0 0 0 0 0 0 0 0 0 -
26 27 25 29 30 0
"""   # (17, 28: no row of their own, 31: past the table — the cursor engine alone, no switch; the last line: auto-pod-operators,
#        cursor-pod-operators, spread-filters, auto-pod-operators-spread, spread-pod-operators, no-such-name)


def test_rows_of_the_engine_table(tmp_path):
    """Every row of csrc/engine_setting.h, 17, 28 and the policy of a value past the table included, printed by a program that includes
    the header."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "rows.cpp"
    src.write_text('#include <cstdio>\n#include "engine_setting.h"\nstatic void row(int v, const ksi::EnginePolicy& p) {\n'
                   '  printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %s\\n", v, (int)p.run, p.first_plan, p.pick_plan, p.pair, p.nodes, p.spread_nodes, p.limits, p.spread_limits,\n'
                   '         p.operators, p.spread_operators, p.unschedulable, p.spread_unschedulable, p.spread_filters, p.pod_operators, p.spread_pod_operators, p.name ? p.name : "-");\n}\n'
                   'int main() { for (unsigned v = 0; v <= 31; ++v) row((int)v, ksi::engine_policy(v));\n'
                   '  printf("%u %u %u %u %u %u\\n", ksi::engine_value("auto-pod-operators"), ksi::engine_value("cursor-pod-operators"), ksi::engine_value("spread-filters"),\n'
                   '         ksi::engine_value("auto-pod-operators-spread"), ksi::engine_value("spread-pod-operators"), ksi::engine_value("no-such-name")); }\n')
    exe = tmp_path / "rows"
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(root, "karpenter_amd", "csrc"), "-o", str(exe), str(src)])
    assert subprocess.check_output([str(exe)], text=True).splitlines() == ENGINE_TABLE.splitlines()
