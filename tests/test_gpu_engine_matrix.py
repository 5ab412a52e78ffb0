"""The engine option, pinned on the device: tests/test_engine_matrix.py's matrix through the product library on the MI355X, one
setting per case, against the device record of tests/golden/engine_matrix.json (the emulation's record overlaid with the cells in
which the device differed at the recording commit: none did). Likewise the late matrix (settings 18-33; alone, batch and many)
against the device record of tests/golden/engine_matrix_late.json: none differed there either."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import engine_matrix as em  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("setting", em.SETTINGS)
def test_every_cell_of_a_setting_equals_the_record(setting):
    want = {k: v for k, v in em.load("device").items() if k.split("|")[1] == str(setting)}
    assert len(want) == len(em.problems()) * 2
    diff = em.differences(em.build_matrix(None, settings=[setting]), want)
    assert not diff, f"{len(diff)} fields differ (cell, field, got, recorded): {diff[:12]}"


@pytest.mark.parametrize("setting", em.LATE_SETTINGS)
def test_every_late_cell_of_a_setting_equals_the_record(setting):
    """The late matrix (tests/golden/engine_matrix_late.json, its device record): alone, batch and many, and many equal to alone."""
    want = {k: v for k, v in em.load("device", em.LATE_FIXTURE).items() if k.split("|")[1] == setting}
    assert len(want) == len(em.late_problems()) * 3
    got = em.build_late(None, settings=[setting])
    diff = em.differences(got, want)
    assert not diff, f"{len(diff)} fields differ (cell, field, got, recorded): {diff[:12]}"
    many = {k[:-len("many")] + "alone": v for k, v in got.items() if k.endswith("|many")}
    diff = em.differences(many, {k: v for k, v in got.items() if k.endswith("|alone")})
    assert not diff, f"{len(diff)} fields differ (cell, field, as a member, alone): {diff[:12]}"

