"""Pod classing against its definition (tests/classing_cases.py), on the host emulation: the generator, the numpy reference,
row_hash_body / row_diff_far / row_class_body / class_gather_body(nl = 1) held against each other without a GPU. The emulation has
one classing "kernel", the loop over row_hash_body, so the variant axis of tests/test_gpu_classing.py collapses: every variant's
cases run through that loop. On every comparison the emulation also holds row_diff_far against rows_equal (collision == 2)."""
import pytest

import classing_cases as cc
import parity


@pytest.fixture(scope="module")
def emu():
    return parity.build_emu()


def test_case_lists_cover_the_boundaries():
    """Every variant's covering set holds every n_rows, every (req_words, n_keys) and n_res the variant accepts, the optional tables
    on and off, all rows equal and all rows distinct; test B reaches mask words 20 and up everywhere and 64 and up where one
    table of 65 words fits the kernel."""
    for name, v in cc.VARIANTS.items():
        sh = cc.shapes(name)
        assert {s["n_rows"] for s in sh} == set(cc.N_ROWS), name
        minvs = (v["minv"],) if v["minv"] is not None else (False, True)
        seps = (v["separate"],) if v["separate"] is not None else (False, True)
        can = {(rw, nk) for rw, nk in cc.WORDS_KEYS if any(cc.accepts(name, rw, nk, r, m, s) for r in v["n_res"] for m in minvs for s in seps)}
        assert {(s["rw"], s["nk"]) for s in sh} == can, name
        assert {s["n_res"] for s in sh} == set(v["n_res"]), name
        assert {s["minv"] for s in sh} == set(minvs) and {s["separate"] for s in sh} == set(seps), name
        assert {s["hp"] for s in sh} == {0, 1} and {s["vol"] for s in sh} == {0, 1} and {s["tw"] for s in sh} == {0, 1, 3}, name
        assert {0, 1} <= {s["pool"] for s in sh} and all(0 <= s["pool"] <= 40 for s in sh), name
        assert all(cc.accepts(name, s["rw"], s["nk"], s["n_res"], s["minv"], s["separate"]) for s in sh), name
        b = cc.b_shape(name)
        assert cc.accepts(name, b["rw"], b["nk"], b["n_res"], b["minv"], b["separate"]) and b["rw"] >= 41, name
    assert {cc.b_shape(n)["rw"] for n in cc.VARIANTS} == {41, 65, 96}
    assert {rw for rw, _ in cc.WORDS_KEYS} == {1, 2, 3, 20, 21, 41, 65, 96} and {nk for _, nk in cc.WORDS_KEYS} == {1, 5, 16, 17, 32}


@pytest.mark.parametrize("variant", list(cc.VARIANTS))
def test_partition_and_class_tables(emu, variant):
    """Test A: rows drawn from a pool of 1 to 40 row values (and all distinct), full hash — no collision, the definition's
    partition and representatives, every gathered table bit for bit."""
    for shape in cc.shapes(variant):
        case = cc.make_case(shape)
        got = cc.run(emu, case)
        assert got["kernel"] == cc.K_HOST
        cc.check_full(case, got, shape)


@pytest.mark.parametrize("variant", list(cc.VARIANTS))
def test_single_field_differences(emu, variant):
    """Test B: all rows the base row but one, which differs in exactly one place; with every hash forced equal the difference is
    reported iff the definition counts it, at full hash it makes two classes or one."""
    shape = cc.b_shape(variant)
    names = set()
    for name, counted, n, at, case in cc.b_cases(shape):
        what = (variant, name, n, at)
        forced = cc.run(emu, case, hash_keep=0)
        cc.check_forced(case, forced, counted, what)
        full = cc.run(emu, case)
        assert full["n_classes"] == (2 if counted else 1), what
        cc.check_full(case, full, what)
        names.add(name.split("[")[0].split(" ")[0] + ("" if counted else " (ignored)"))
    sets = ("reqs", "strict") if shape["separate"] else ("reqs",)
    want = {"request", "tolerates", "host_ports", "vol", "topo_owned", "topo_selected"}
    for s in sets:
        want |= {f"{s}.mask", f"{s}.defined", f"{s}.complement", f"{s}.has_gte", f"{s}.has_lte", f"{s}.gte", f"{s}.lte", f"{s}.mask (ignored)", f"{s}.gte (ignored)", f"{s}.lte (ignored)"}
        if shape["minv"]:
            want |= {f"{s}.minv", f"{s}.minv (ignored)"}
    assert names == want, (variant, names ^ want)
