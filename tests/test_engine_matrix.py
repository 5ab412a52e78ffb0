"""The engine option, pinned (CPU; tests/test_gpu_engine_matrix.py on the device): every problem of tests/tools/engine_matrix.py under
every value of ksolve_options.engine, alone and in a batch, through the host emulation and the real host library, against the record
in tests/golden/engine_matrix.json — taken from the commit before the option was decoded through csrc/engine_setting.h's table. Cell
by cell and field by field: outcome, full error text, engine, fallback reason, memory plan, attempts, Results digest. No cell is skipped."""
import os
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
