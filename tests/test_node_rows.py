"""The static (class, node) rows (ksolve_node_dead0) against their definition (tests/node_row_cases.py), on the host emulation:
generated problems over the grid of sizes (test A), single differences at the tail block's only lane / the second chunk's only class
and at node 0 / class 0 (test B), the same class row and the same node at several indices (test C). This file also holds the generator
to its conditions, computed from the definition alone, so that a degenerate generator fails instead of passing. The GPU run of the
same lists is tests/test_gpu_node_rows.py. Every comparison is exact."""
import numpy as np
import pytest

import node_row_cases as nr
import parity
from reqalg_cases import has_intersection, negative


@pytest.fixture(scope="module")
def emu():
    return parity.build_emu()


# ------------------------------------------------------------------------------------------------ what the case lists cover
def test_grid_is_the_one_stated():
    sizes = {(g[0], g[1]) for g in nr.GRID}
    assert sizes == {(1, 1), (63, 31), (64, 32), (65, 33), (130, 70)}
    for size in sizes:
        assert {g[3] for g in nr.GRID if (g[0], g[1]) == size} == {"small", "wide"}, size
    assert {g[2] for g in nr.GRID if (g[0], g[1]) == (65, 33)} >= {1, 4, 8} and {g[4] for g in nr.GRID} == {"on", "off", "none"}
    small, wide = nr.small_space(), nr.wide_space()
    assert (small.nk, small.rw) == (3, 3) and (wide.nk, wide.rw) == (6, 7) and list(wide.off) == [0, 1, 3, 4, 5, 6, 7]
    assert len(wide.values["wide"]) == 70 and all(v.isdigit() for v in wide.values["rack"]) and sum(v.isdigit() for v in wide.values["gen"]) == 6


@pytest.mark.parametrize("case", [g for g in nr.GRID if g[0] >= 65], ids=nr.grid_id)
def test_generated_problems_meet_their_conditions(case):
    p = nr.generated(*case)
    got = nr.shares(p)
    print(case, {k: round(v, 3) for k, v in got.items()})
    assert got["alive"] >= 0.20 and got["dead"] >= 0.20, got
    for reason in nr.REASONS:
        assert got[reason] >= 0.02, (reason, got)


def test_generated_problems_reach_the_branches_of_the_requirement_check():
    """What the pairs of the two (130, 70) problems make node_reqs_ok do, from the definition: every way in and out of its loop."""
    seen = set()
    for name in ("small", "wide"):
        p = nr.generated(130, 70, 2, name, "on")
        ops = {(type_, r.complement, r.gte is not None, r.lte is not None) for type_, rows in (("class", p["classes"]), ("node", p["nodes"])) for row in rows for r in row.values()}
        assert {("class", True, True, False), ("class", True, False, True), ("class", True, True, True), ("class", False, False, False), ("node", True, False, False)} <= ops, name
        assert not any(o[0] == "node" and (o[2] or o[3]) for o in ops)
        for k, cls in enumerate(p["classes"]):
            for e, node in enumerate(p["nodes"]):
                for key, q in cls.items():
                    bounded = q.gte is not None or q.lte is not None
                    if key not in node:
                        seen.add("undefined key, allowed" if negative(q) else "undefined key, refused")
                        continue
                    r = node[key]
                    hit = has_intersection(r, q)
                    if q.gte is not None and q.lte is not None and q.gte > q.lte:
                        seen.add("empty range against a complement node set" if r.complement else "empty range against a concrete node set")
                    elif bounded and not r.complement:
                        seen.add("bounded, a node value inside" if hit else "bounded, no node value inside")
                    elif r.complement and q.complement:
                        seen.add("two complement sets")
                    elif r.complement or q.complement:
                        seen.add("one complement set, values left" if hit else "one complement set, nothing left")
                    else:
                        seen.add("two concrete sets, shared value" if hit else "two concrete sets, disjoint")
                    if not hit and negative(q) and negative(r):
                        seen.add("no intersection, both negative")
                    if name == "wide" and key == "wide" and not r.complement and not q.complement and hit and all(wv in nr.WIDE[64:] for wv in r.values & q.values):
                        seen.add("shared value on the second word only")
    want = {"undefined key, allowed", "undefined key, refused", "empty range against a complement node set", "empty range against a concrete node set", "bounded, a node value inside",
            "bounded, no node value inside", "two complement sets", "one complement set, values left", "one complement set, nothing left", "two concrete sets, shared value",
            "two concrete sets, disjoint", "no intersection, both negative", "shared value on the second word only"}
    assert seen == want, want ^ seen


@pytest.mark.parametrize("e0,k0", nr.POSITIONS)
def test_single_differences_flip_what_they_claim(e0, k0):
    """From the definition alone: the base problem is alive everywhere, and every change flips exactly what its kind says."""
    base = nr.base_problem(e0, k0)
    table, why = nr.expected_rows(base)
    assert not any(why.values()) and nr.dead_pairs(table, 65) == (set(), True)
    assert (len(base["nodes"]), len(base["classes"]), base["n_res"]) == (65, 33, 8) and base["nodes"][e0]["rack"].complement and "team" not in base["nodes"][e0]
    kinds = [kind for _, kind in nr.CHANGES.values()]
    assert len(nr.CHANGES) == 27 and kinds.count("pair") == 14 and kinds.count("none") == 2 and kinds.count("column") == 10 and kinds.count("row") == 1
    for name, (_, kind) in nr.CHANGES.items():
        dead, past = nr.dead_pairs(nr.expected_rows(nr.changed_problem(e0, k0, name))[0], 65)
        assert past and dead == nr.flips_of(kind, e0, k0), (name, kind, sorted(dead)[:5])


def test_position_problem_repeats_one_class_and_one_node():
    p = nr.position_problem()
    assert len({repr(p["classes"][k]) for k in nr.CLASS_SPOTS}) == 1 and len({repr(p["nodes"][e]) for e in nr.NODE_SPOTS}) == 1
    assert p["classes"][nr.CLASS_SPOTS[0]] and len(p["nodes"][nr.NODE_SPOTS[0]]) >= 3
    dead, _ = nr.dead_pairs(p["expected"], 130)
    row = {e for k, e in dead if k == nr.CLASS_SPOTS[0]}
    col = {k for k, e in dead if e == nr.NODE_SPOTS[0]}
    assert 0 < len(row) < 130 and 0 < len(col) < 70          # neither all dead nor all alive: the verdicts can differ


# ------------------------------------------------------------------------------------------------ the product's kernel, emulated
@pytest.mark.parametrize("case", nr.GRID, ids=nr.grid_id)
def test_generated_problems(emu, case):
    nr.run_generated(emu, case)


@pytest.mark.parametrize("e0,k0", nr.POSITIONS)
def test_single_differences(emu, e0, k0):
    nr.run_single_differences(emu, e0, k0)


def test_position_independence(emu):
    nr.run_positions(emu)
