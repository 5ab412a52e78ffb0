"""The finalize kernel (with the sweep's claim gather and slot_of) and the fast engines' effective allocatable against their
definitions (tests/result_cases.py), on the host emulation — where a launch is the loop over the kernel body. This file also holds
the generated problems to what they must contain. The GPU run of the same lists is tests/test_gpu_result_kernels.py. Every comparison
is exact, prices by their bits."""
import numpy as np
import pytest

import parity
import result_cases as rc


@pytest.fixture(scope="module")
def emu(oracle):
    rc.use_oracle(oracle)
    return parity.build_emu()


# ------------------------------------------------------------------------------------------------ what the generated problems contain
def test_generated_problems_meet_every_condition(oracle, emu):
    """from the definition alone: each condition holds for at least 5 % of the generated claims"""
    facts = [f for name in rc.FINALIZE_CASES if rc.FINALIZE_CASES[name].get("truncate_n", 10) for f in rc.finalize_expected(oracle, name)["facts"]]
    shares = {k: np.mean([test(f) for f in facts]) for k, test in
              (("DBL_MAX cheapest", lambda f: f["dbl_max"]), ("tie across the truncation boundary", lambda f: f["boundary_tie"]), ("truncation failed", lambda f: f["failed"]),
               ("truncation succeeded under minValues", lambda f: f["minv_ok"]), ("two or more groups contribute", lambda f: f["groups"] >= 2))}
    print(f"{len(facts)} claims: " + ", ".join(f"{k} {100 * v:.1f} %" for k, v in shares.items()))
    assert all(v >= 0.05 for v in shares.values()), shares


def test_case_list_covers_what_it_claims(oracle, emu):
    sizes = rc.FINALIZE_SIZES
    assert {c for c, _ in sizes} == {1, 255, 256, 257} and {n for _, n in sizes} == {1, 12, 13, 49, 50, 51, 63, 64, 65, 257, 1000} and max(c * n for c, n in sizes) == 257 * 1000
    fams = set()
    for name in rc.FINALIZE_CASES:
        fams |= set(rc.finalize_problem(name)["zone_family"])
    assert fams == set(rc.FAMILIES) | {"killer"} and rc.finalize_problem("heapsort")["slots"][0]["its"] == set(range(1000))
    P = rc.finalize_problem("cell-63")
    assert {(z, c) for o in P["offers"] for z, c, _ in o} == {(15, 3)}
    e = rc.finalize_expected(oracle, "cell-63")
    assert 0 < sum(f["dbl_max"] for f in e["facts"]) < len(e["facts"])
    P = rc.finalize_problem("template-31")
    assert {s["template"] for s in P["slots"]} >= {5, 31} and len(P["groups"][31]) == 6 and not P["groups"][5]
    P = rc.finalize_problem("257x64")
    held = [s["held"] for s in P["slots"] if s["held"]]
    assert any(0 in h for h in held) and any(63 in h for h in held)
    assert any(r.min_values is not None and r.key == "family" for s in P["slots"] for r in s["reqs"].values()) and P["space"].off[4] - P["space"].off[3] == 2
    assert any(r.min_values is not None and r.key == "it" for s in P["slots"] for r in s["reqs"].values())
    assert any(r.complement for rs in P["it_reqs"] for r in rs.values())
    # a template whose groups are stored in another order than the order of first appearance, one with a group that holds no daemon pod
    assert any([min(g["its"] & P["t_its"][1]) for g in P["groups"][1] if g["its"] & P["t_its"][1]] != sorted(min(g["its"] & P["t_its"][1]) for g in P["groups"][1] if g["its"] & P["t_its"][1])
               for P in (rc.finalize_problem(n) for n in rc.FINALIZE_CASES))
    assert any(not g["nonempty"] for n in rc.FINALIZE_CASES for gs in rc.finalize_problem(n)["groups"] for g in gs)


# ------------------------------------------------------------------------------------------------ finalize
@pytest.mark.parametrize("name", list(rc.FINALIZE_CASES))
def test_finalize(oracle, emu, name):
    P, want = rc.finalize_problem(name), rc.finalize_expected(oracle, name)
    got = rc.run_finalize(emu, P)
    assert rc.mismatches(got, want) == [], name
    other = rc.run_finalize(emu, P, poison=rc.POISONS[1])
    assert rc.mismatches(other, got) == [], "the answers depend on the poison"


def test_finalize_reservation_tables_without_held_column(oracle, emu):
    """c_reserved null: the claims hold nothing, whatever the reservation tables say"""
    import copy
    P = copy.deepcopy(rc.finalize_problem("255x51"))
    got = rc.run_finalize(emu, P, c_reserved=False)
    for s in P["slots"]:
        s["held"] = set()
    assert rc.mismatches(got, rc.expected_finalize(oracle, P)) == []


@pytest.mark.parametrize("kind", ["identity", "permutation", "duplicates"])
def test_finalize_behind_slot_of(oracle, emu, kind):
    base = rc.finalize_problem("slots")
    P = rc.with_slots(base, kind)
    want = rc.expected_finalize(oracle, P)
    for poison in rc.POISONS:
        got = rc.run_finalize(emu, P, poison=poison)
        assert rc.mismatches(got, want) == [], (kind, hex(poison))
        assert rc.gather_mismatches(P, got) == [], (kind, hex(poison))
    if kind == "identity":
        assert rc.mismatches(got, rc.run_finalize(emu, base, poison=rc.POISONS[1])) == [], "the identity differs from the run without slot_of"
    if kind == "permutation":      # the same claims in the same order, wherever their records lie
        assert len(P["slots"]) > len(base["slots"]) and P["slot_of"] != sorted(P["slot_of"])
        assert rc.mismatches(got, rc.run_finalize(emu, base)) == [], "the answers depend on where the records lie"


def test_finalize_single_differences(oracle, emu):
    """one change to the problem alters what the definition says it alters, for the claim it concerns alone — and the kernel follows"""
    base = rc.single_base()
    want0 = rc.expected_finalize(oracle, base)
    assert rc.mismatches(rc.run_finalize(emu, base), want0) == []
    for name, Q, may, must in rc.single_changes(base):
        want = rc.expected_finalize(oracle, Q)
        diff = rc.mismatches(want, want0)
        assert diff and {c for _, c in diff} == {0} and {k for k, _ in diff} <= may and must in {k for k, _ in diff}, (name, diff)
        assert rc.mismatches(rc.run_finalize(emu, Q), want) == [], name


# ------------------------------------------------------------------------------------------------ the effective allocatable
@pytest.mark.parametrize("name", list(rc.EFF_CASES))
def test_eff_alloc(emu, name):
    E = rc.eff_case(name)
    want = rc.expected_eff(E)
    assert (want[[t for t in range(E["n_templates"]) if (E["tmpl_ov"] >> t) & 1]] == rc.K_EFF_NEVER).any() == any(len(g) > 1 for t, g in enumerate(E["groups"]) if (E["tmpl_ov"] >> t) & 1)
    assert np.array_equal(rc.run_eff(emu, E), want), name


def test_eff_case_list_covers_what_it_claims():
    cases = [rc.eff_case(n) for n in rc.EFF_CASES]
    assert {c["n_its"] for c in cases} == {1, 63, 64, 65, 257} and {c["n_templates"] for c in cases} == {1, 2, 32} and {c["n_res"] for c in cases} == {1, 4, 8}
    assert all(c["tmpl_ov"] == 1 << 31 for c in cases if c["n_templates"] == 32) and any(c["tmpl_ov"] == 0b10 for c in cases)
    big = rc.expected_eff(rc.eff_case("257its-2t-4r"))
    assert (big < rc.K_EFF_NEVER).any() and (big > (1 << 61)).any()      # overhead above allocatable; values near 2^62
    E = rc.eff_case("257its-2t-4r")
    assert any(sum(i in g["its"] for g in gs) == 2 for gs in E["groups"] for i in range(E["n_its"]))      # a type in two groups


# ------------------------------------------------------------------------------------------------ the cursor engine's claim records
@pytest.mark.parametrize("name", list(rc.RECORD_CASES))
def test_fast_records(emu, name):
    R = rc.records_case(name)
    want = rc.expected_records(R)
    got = rc.run_records(emu, R)
    assert rc.record_mismatches(got, want) == [], name
    assert got["c_hot"].shape[1] == R["space"].rw + (R["n_its"] + 63) // 64 + 2 * R["n_res"] + 4 and not (got["c_hot"] == np.uint64(R["poison"])).any()


def test_record_case_list_covers_what_it_claims():
    cases = {n: rc.records_case(n) for n in rc.RECORD_CASES}
    assert {len(R["claims"]) for R in cases.values()} >= {1, 63, 64, 65} and {R["n_its"] for R in cases.values()} == {63, 64, 65, 130}
    assert {len(R["var_keys"]) for R in cases.values()} == {0, 1, 3, 12} and {R["space"].nk % 2 for R in cases.values()} == {0, 1}
    assert cases["no-limits"]["real"] is None and any(c["stage"] >= 3 for c in cases["65-claims-130-types"]["claims"])
    R = cases["65-claims-130-types"]
    want = rc.expected_records(R)
    assert want["cold_written"].any() and not want["cold_written"].all()
    last = R["space"].nk - 1
    assert R["space"].kidx[R["var_keys"][-1]] == last and R["space"].off[last] == R["space"].rw - 1                       # a field in the last word
    guards = {(rc.record_reqs(R, c)[1], c["fields"]["zone"][0]) for c in R["claims"]}
    assert {(1, True), (1, False), (2, True), (2, False), (0, True), (0, False)} <= guards                               # complement / bounds kept and dropped, undefined kept
    assert any(R["ent_junk"]) and any(not s for s in R["ent_its"])
    kept = [bin(int(w)).count("1") for row in want["its"] for w in row]
    assert 0 in kept and max(kept) > 0
    assert (np.array(R["eff"]) == rc.K_EFF_NEVER).any() and R["tmpl_ov"] == 0b110


@pytest.mark.parametrize("name", ["63-claims-64-types", "65-claims-130-types", "no-limits"])
def test_records_feed_finalize(oracle, emu, name):
    """the chain: what the record kernel wrote, column for column into the finalize kernel, gives the definition's finalize answers"""
    R = rc.records_case(name)
    got = rc.run_records(emu, R)
    P = rc.chain_problem(R, got)
    want = rc.expected_finalize(oracle, P)
    for poison in rc.POISONS:
        assert rc.mismatches(rc.run_finalize(emu, P, poison=poison), want) == [], (name, hex(poison))
