"""The requirement algebra (csrc/reqalg.h) and the instance-type index (csrc/kernels.h it_index_body) against their definition
(tests/reqalg_cases.py), on the host emulation: the reference's own truth tables, generated pairs at every shape, the index cases.
This file also holds the case lists to what they claim — the shares of the interesting outcomes among the generated pairs (from
the definition alone, so a generator that drifts cannot hide a failure), the word boundaries, key 31, the null columns. The GPU
run of the same lists is tests/test_gpu_reqalg.py. Every comparison is exact."""
import numpy as np
import pytest

import parity
import reqalg_cases as rc


@pytest.fixture(scope="module")
def emu():
    return parity.build_emu()


@pytest.fixture(scope="module")
def golden():
    return rc.golden_tables()


# ------------------------------------------------------------------------------------------------ the definition itself
def test_definition_reproduces_the_reference_tables(golden):
    """The set-based definition against the reference's tables, before anything is held against the definition."""
    tables, compat = golden
    defs = tables["definitions"]
    assert (len(tables["intersection"]), len(tables["has"]), len(compat["loose"]), len(compat["strict"])) == (590, 70, 225, 225)
    for a, b, exp in tables["intersection"]:
        got = rc.intersection(rc.from_selector(defs[a]), rc.from_selector(defs[b]))
        assert got == rc.table_struct(defs, exp), (a, b, exp, got)
        assert rc.has_intersection(rc.from_selector(defs[a]), rc.from_selector(defs[b])) == (got.complement or len(got.values) > 0), (a, b)
    for name, value, exp in tables["has"]:
        assert rc.has(rc.from_selector(defs[name]), value) == exp, (name, value)
    for name, op in tables["operator"]:
        assert rc.operator(rc.from_selector(defs[name])) == op, name
    for name, ln in tables["len"]:
        assert rc.length(rc.from_selector(defs[name])) == ln, name
    cdefs = compat["definitions"]
    sets = lambda name: {} if cdefs[name] is None else {cdefs[name]["key"]: rc.from_selector(cdefs[name])}
    for mode, allow in (("loose", {rc.ZONE}), ("strict", set())):
        for a, b, exp in compat[mode]:
            assert (rc.compatible(sets(a), sets(b), allow) == rc.COMPAT_OK) == exp, (mode, a, b)


def test_definition_gte_lte_and_integer_extremes():
    """requirement_test.go:953-1084 as test_oracle_golden.py::test_gte_lte_operators states it, and what Go does at the ends of int."""
    r = lambda op, n: rc.new_requirement("key", op, None, str(n))
    assert rc.has(r("Gte", 5), "5") and rc.has(r("Gte", 5), "6") and not rc.has(r("Gte", 5), "4")
    assert rc.has(r("Lte", 5), "5") and rc.has(r("Lte", 5), "4") and not rc.has(r("Lte", 5), "6")
    x = rc.intersection(r("Gte", 3), r("Lte", 7))
    assert (x.gte, x.lte, x.complement) == (3, 7, True)
    assert r("Gt", 4) == r("Gte", 5) and r("Lt", 6) == r("Lte", 5)
    assert rc.intersection(r("Gte", 3), r("Gt", 5)).gte == 6 and rc.intersection(r("Gte", 8), r("Gt", 5)).gte == 8 and rc.intersection(r("Lte", 3), r("Lt", 9)).lte == 3
    assert rc.has(r("Gte", 0), "0") and not rc.has(r("Gte", 0), "-1") and rc.has(r("Lte", 0), "0") and not rc.has(r("Lte", 0), "1")
    assert rc.operator(r("Gt", rc.INT_MAX)) == "DoesNotExist" and not rc.has(r("Gte", 1), "abc")
    assert rc.new_requirement("key", "Gt", 2, str(rc.INT_MAX)).min_values is None      # requirement.go:91 goes through NewRequirement
    assert r("Lt", rc.INT_MIN).lte == rc.INT_MAX                                           # value-- wraps (requirement.go:98)
    # strconv.Atoi: a sign and decimal digits inside int64, nothing else
    assert [rc.go_atoi(s) for s in ("007", "+5", "-0", str(rc.INT_MAX), str(rc.INT_MIN))] == [7, 5, 0, rc.INT_MAX, rc.INT_MIN]
    assert all(rc.go_atoi(s) is None for s in ("9223372036854775808", "-9223372036854775809", "1e3", "0x10", " 1", "", "1_0", "abc", "+", "-"))


def test_encoder_and_decoder_round_trip():
    for name in ("b", "c", "d"):
        space, A, _ = rc.gen_pairs(name)
        t = rc.encode_sets(space, A[:50], junk=True)
        assert [rc.decode_sets(space, t, i) for i in range(50)] == A[:50], name
    space = rc.shape_space("c")
    assert list(space.off) == [0, 1, 3, 6, 7]
    assert [int(x) for x in space.value_valid] == [2**64 - 1, 2**64 - 1, 1, 2**64 - 1, 2**64 - 1, 3, 1]


# ------------------------------------------------------------------------------------------------ what the case lists cover
@pytest.mark.parametrize("name", list(rc.SHAPES))
def test_generated_pairs_meet_their_shares(name):
    space, A, B = rc.gen_pairs(name)
    got = rc.shares(space, A, B)
    print(name, {f: round(v, 3) for f, v in got.items()})
    assert len(A) == len(B) == rc.SHAPES[name]["pairs"]
    for fact, least in rc.SHARES.items():
        if name == "f" and fact in rc.BOUND_SHARES:
            assert got[fact] == 0
            continue
        assert got[fact] >= least, (name, fact, got[fact], least)


def test_case_lists_cover_what_they_claim():
    spaces = {name: rc.shape_space(name) for name in rc.SHAPES}
    sizes = {name: [len(spaces[name].values[k]) for k in spaces[name].keys] for name in rc.SHAPES}
    assert sizes["a"] == [8] and sizes["b"] == sizes["f"] == [5, 8, 3] and sizes["c"] == [64, 65, 130, 1] and sizes["e"] == [2048] * 3
    assert len(sizes["d"]) == 32 and set(sizes["d"]) == {1, 2, 3}
    assert [rc.SHAPES[n]["pairs"] for n in "abcde"] == [600, 1000, 400, 200, 60]
    # shape c: a key that ends at bit 63, one that starts a second word, one over three words; shape e: kMaxReqWords
    assert list(spaces["c"].off) == [0, 1, 3, 6, 7] and spaces["e"].rw == 96 and spaces["d"].nk == 32
    for name in rc.SHAPES:
        space, A, B = rc.gen_pairs(name)
        kinds = set()
        for row in A + B:
            for r in row.values():
                kinds.add((rc.operator(r), r.gte is not None, r.lte is not None, r.min_values is not None))
        ops = {k[0] for k in kinds}
        assert ops == {"In", "NotIn", "Exists", "DoesNotExist"}, name
        if rc.SHAPES[name]["null"]:
            assert all(not (k[1] or k[2] or k[3]) for k in kinds)
            assert rc.encode_sets(space, A, null_cols=True)["gte"] is None
            continue
        assert any(k[0] == "Exists" and k[1] and not k[2] for k in kinds) and any(k[0] == "Exists" and k[2] and not k[1] for k in kinds), name   # Gt / Gte, Lt / Lte
        assert any(k[0] == "NotIn" and (k[1] or k[2]) for k in kinds), name           # a bound and an excluded set together
        assert {r.min_values for row in A + B for r in row.values()} == {None, 0, 1, 2, 50}, name
        if name == "c":
            # values in the last bit of a word and the first of the next one are used, in every key that has them
            used = {(k, v) for row in A + B for k, r in row.items() for v in r.values}
            for k, j in (("key0", 63), ("key1", 63), ("key1", 64), ("key2", 63), ("key2", 64), ("key2", 127), ("key2", 128), ("key2", 129)):
                assert (k, space.values[k][j]) in used, (k, j)
        if name == "d":
            both = sum(1 for a, b in zip(A, B) if "key31" in a and "key31" in b)
            assert both >= 10 and any("key31" in b and "key31" not in a for a, b in zip(A, B))
        if name == "e":
            used = {space.bitpos[k][v] // 64 for row in A + B for k, r in row.items() for v in r.values}
            assert {0, 31, 32, 63, 64, 95} <= used
    bounds = {b for name in "abcde" for row in sum(rc.gen_pairs(name)[1:], []) for r in row.values() for b in (r.gte, r.lte) if b is not None}
    assert {rc.INT_MAX, rc.INT_MIN, rc.INT_MAX - 1, rc.INT_MIN + 1, 0, -1} <= bounds
    tspace = rc.table_space()
    tables, compat = rc.golden_tables()
    named = {v for d in list(tables["definitions"].values()) + [d for d in compat["definitions"].values() if d] for v in d["values"]} | {h[1] for h in tables["has"]}
    assert named <= set(rc.TABLE_VALUES) and tspace.well_known == {rc.ZONE}
    assert sorted(rc.INDEX_SIZES) == sorted((n, r) for n in (1, 63, 64, 65, 130) for r in (1, 4)) and rc.CONTENTION_SIZES == (64, 2048)


# ------------------------------------------------------------------------------------------------ the product's algebra
def test_reference_tables(emu, golden):
    rc.run_tables(emu, golden)


@pytest.mark.parametrize("name", list(rc.SHAPES))
def test_generated_pairs(emu, name):
    rc.run_shape(emu, name)


@pytest.mark.parametrize("n_its,n_res", rc.INDEX_SIZES)
def test_it_index(emu, n_its, n_res):
    got, want = rc.run_index(emu, n_its, n_res, "ordinary")
    # the case has what it is for: every table non-empty (from 63 types on), a type with a negative allocatable
    if n_its >= 63:
        assert all(want[f].any() for f in rc.INDEX_FIELDS) and bin(int(want["it_alloc_ok"][0])).count("1") < min(n_its, 64)
        assert want["kv_has"][64:64 + n_its].sum() == 0                        # rows of the instance-type key stay zero


@pytest.mark.parametrize("n_its", rc.CONTENTION_SIZES)
def test_it_index_contention(emu, n_its):
    got, want = rc.run_index(emu, n_its, 2, "contention")
    full = np.full(n_its // 64, 2**64 - 1, rc.U64)
    # every thread of a word ORs the same two words: the value's row of kv_has and the undefined key's row
    assert np.array_equal(want["kv_has"][1], full) and np.array_equal(want["key_undef"][2], full) and np.array_equal(want["it_alloc_ok"], full)


@pytest.mark.parametrize("kind", ["wrong-name", "bound"])
def test_it_index_errors(emu, kind):
    rc.run_index(emu, 65, 2, kind)


def test_lt_min_int_in_the_oracle(oracle):
    """Lt math.MinInt: Go's value-- wraps to MaxInt (requirement.go:98), and the oracle's restatement says the same (its arithmetic
    there is unsigned; the host flattener's too — both were a signed overflow)."""
    r = oracle.evaluate({"fn": "describe", "a": {"key": "key", "operator": "Lt", "values": [str(rc.INT_MIN)]}})
    want = rc.new_requirement("key", "Lt", None, str(rc.INT_MIN))
    assert (r["complement"], r["gte"], r["lte"], r["values"]) == (want.complement, want.gte, want.lte, [])
