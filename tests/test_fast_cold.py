"""The cold half of the cursor engine (fast_engine.h FastCold) against its definition (tests/fast_cold_cases.py), on the host
emulation in both lane orders — one wavefront over the product's LDS plan: setup(), then a script of create_entry / fast_lookup /
fast_fits / fast_fields_ok / offering_cells / compat_word / filter_diag / new_slot / new_claim / refresh_claim calls, every table they
leave downloaded and compared. This file also
holds the generated cases to what they must contain, from the definition alone. The GPU run of the same cases is
tests/test_gpu_fast_cold.py. Every comparison is exact; the fields left out are named in fast_cold_cases.py's docstring."""
import collections

import pytest

import fast_cold_cases as fc
import parity


@pytest.fixture(scope="module", params=["lanes ascending", "lanes descending"])
def emu(request):
    return parity.build_emu(reverse_lanes=request.param == "lanes descending")


_expected = {}


def expect(name):
    if name not in _expected:
        P, script = fc.load(name)
        _expected[name] = (P, script, fc.expected(P, script))
    return _expected[name]


@pytest.mark.parametrize("name", list(fc.CASES))
def test_against_definition(emu, name):
    P, script, want = expect(name)
    got = fc.run(emu, P, script, want)
    assert got["status"] == 0 and got["kernel"] == fc.kernel_id(P, emulation=True)
    assert fc.mismatches(got, want, P, script) == [], name


@pytest.mark.parametrize("name", list(fc.DECLINES))
def test_decline(emu, name):
    P, reason = fc.DECLINES[name]()
    want = fc.expected(P, [("CELLS", 0, ())])
    assert want["setup_ret"] == reason, (name, "the definition")
    got = fc.run(emu, P, [("CELLS", 0, ())], want)
    assert fc.mismatches(got, want, P, [("CELLS", 0, ())]) == [], name


@pytest.mark.parametrize("name", list(fc.REFUSED))
def test_hook_refuses_what_is_out_of_range(emu, name):
    P, script, edit = fc.REFUSED[name]()
    got = fc.run(emu, P, script, edit=edit)
    assert got["status"] == fc.KSOLVE_ERR_INVALID, name
    assert bytes(got["scal"]) == b"\xA5" * len(bytes(got["scal"])), "nothing was launched"


# ------------------------------------------------------------------------------------------------ what the cases contain
def test_cases_reach_every_outcome():
    """from the definition alone: the sizes the case list names, and how often the scripts reach each outcome"""
    cases = {n: expect(n) for n in fc.CASES}
    sizes = lambda f: {f(P) for P, _, _ in cases.values()}
    assert sizes(lambda P: P.n_its) >= {1, 63, 64, 65, 130, 2048} and sizes(lambda P: len(P.templates)) >= {1, 2, 31, 32}
    assert sizes(lambda P: len(P.classes)) >= {1, 64, 65, 130} and sizes(lambda P: P.n_res) == {1, 2, 3, 4}
    assert sizes(lambda P: P.n_zones) >= {1, 16} and sizes(lambda P: P.n_cts) >= {1, 4}
    assert {(P.plan, P.rows, P.flavour) for P, _, _ in cases.values()} == fc.DEVICE_KERNELS
    facts = collections.Counter(f for _, _, w in cases.values() if not w["setup_ret"] for f in w["facts"])
    fronts = collections.Counter((f[1], f[2]) for f in facts.elements() if f[0] == "front")
    print(sorted(fronts.items()))
    for size in (0, 1, 2, 16, 17):
        assert fronts[(size, "ok")] >= 1, size
    assert fronts[(18, "refused")] >= 1 and fronts[(17, "refused")] >= 1 and fronts[(1, "refused")] >= 1       # the front's bound, the pool's, the cache's gate
    assert sum(n for (s, _), n in fronts.items() if 3 <= s <= 15) >= 20
    looks = collections.Counter((f[1], f[2]) for f in facts.elements() if f[0] == "lookup")
    print(sorted(looks.items()))
    assert looks[("miss", 0)] >= 20 and looks[("first", 0)] >= 100 and looks[("first", 1)] >= 100 and looks[("later", 1)] + looks[("later", 0)] >= 10
    joins = collections.Counter((r["tmplok"], r["joins"]) for _, _, w in cases.values() if not w["setup_ret"] for r in w["res"] if "joins" in r)
    print(sorted(joins.items()))
    assert joins[(1, 1)] >= 100 and joins[(1, 0)] >= 50 and joins[(0, 0)] >= 50 and joins[(0, 1)] == 0
    # differences at lane 0 and lane 63 of the last word and on the first type past a word edge: the class that alone selects them
    for name, bits in (("63-types", {0, 62}), ("64-types", {0, 63}), ("65-types", {63, 64}), ("130-types", {0, 64, 128, 129}), ("2048-types", {0, 1984, 2047})):
        P, script, w = cases[name]
        D = w["D"]
        got = [D.F(t, D.merged(t, (0,))) for t in range(len(P.templates))]
        assert any(g and g <= bits for g in got), name
    # a type whose only available offering sits in the last cell, admitted by some set and not by another
    P, script, w = cases["65-types"]
    lone = P.n_its // 2
    assert P.offers[lone] == {(15, 3)}
    held = [lone in s["F"] for s in w["cache"].slots.values()]
    assert any(held) and not all(held)
    # negative effective allocatables, and K_EFF_NEVER, inside cached fronts
    P, script, w = cases["overhead"]
    vals = [x for s in w["cache"].slots.values() for v in s["front"] for x in v]
    assert min(fc.eff(P, t, r, it) for t in range(len(P.templates)) for r in range(P.n_res) for it in range(P.n_its)) == fc.K_EFF_NEVER and min(vals) < 0
    # ties in the first resources decided by the last
    P, script, w = cases["front-ties"]
    front = next(iter(w["cache"].slots.values()))["front"]
    assert len(front) == 6 and len({v[0] for v in front}) == 1 and len({v[3] for v in front}) == 6
    # the run of sets with one hash, the sets at slot 1,023, the gate and the pool's last row
    P, script, w = cases["hash-runs"]
    slots = sorted(w["cache"].slots)
    assert {1023, 0, 1} <= set(slots) and any(all(h + i in slots for i in range(5)) for h in slots)
    assert cases["cache-gate"][2]["n_ent"] == fc.K_GATE and len(cases["cache-gate"][2]["res"]) == len(cases["cache-gate"][1]) - 1
    assert cases["pool-full"][2]["n_pool"] == fc.K_POOL and [r["ret"] >= 0 for r in cases["pool-full"][2]["res"] if "ret" in r and "fits" not in r][-2:] == [True, False]


def test_loop_cases_reach_every_outcome():
    """from the definition alone: what the scripts of class slots, new claims and joining pods reach"""
    cases = {n: expect(n) for n in fc.CASES}
    facts = collections.Counter(f for _, _, w in cases.values() if not w["setup_ret"] for f in w["facts"])
    made = collections.Counter((f[1], f[2]) for f in facts.elements() if f[0] == "new_claim")
    print(sorted(made.items(), key=str))
    assert made[(1, 0)] >= 100                                                         # claims created
    errors = collections.Counter(v[0] for (ret, v), n in made.items() if ret == 2 for _ in range(n))
    assert errors[fc.E_TAINTS] >= 20 and errors[fc.E_INCOMPATIBLE] >= 20 and errors[fc.E_INSTANCE_TYPES] >= 10 and errors[fc.E_NO_TEMPLATES] >= 2
    for stop in (fc.DECLINE_KERNEL_CAPACITY, fc.DECLINE_CLAIM_SLOTS, fc.DECLINE_UNSCHEDULABLE_POD):
        assert made[(0, stop)] >= 1, stop
    flags = collections.Counter(f[1] for f in facts.elements() if f[0] == "diag") + collections.Counter(v[1] for (ret, v), n in made.items() if ret == 2 for _ in range(n))
    print(sorted(flags.items()))
    for bit in (1, 2, 4, 16, 32):
        assert sum(n for f, n in flags.items() if f & bit) >= 2 and sum(n for f, n in flags.items() if not f & bit) >= 2, bit
    # a verdict kept and used again: the second walk of a class that failed adds the templates it had tried, without walking
    P, script, w = cases["verdict-reused"]
    assert [r["ret"] for r in w["res"]] == [2, 2, 2, 1, 2] and w["M"].host_seq == 4 * w["M"].us_cls[3][2] + w["M"].hostseq[0] - w["M"].us_cls[3][2] * 3 and w["M"].us_cls[3][2] >= 1
    # the retry's net on both sides, the pool's last row inside a refresh, every slot dropped at once
    assert [r["ret"] for r in cases["retry-net"][2]["res"]] == [2, 0] and cases["retry-net"][2]["M"].bail == fc.DECLINE_UNSCHEDULABLE_POD
    assert cases["loop-keep-4-rows"][2]["M"].bail == fc.DECLINE_CACHE_FULL and cases["loop-keep-4-rows"][2]["M"].cache.n_pool == fc.K_POOL
    assert cases["evict-1-row"][2]["res"][65]["ret"] == 1 << 16 and cases["evict-4-rows"][2]["res"][257]["ret"] == 1 << 16 and cases["evict-4-rows"][2]["res"][256]["ret"] >> 6 in (0, 1, 2, 3)
    # four rows: classes go to more than one row while the first still has room
    M = cases["loop-keep-4-rows"][2]["M"]
    used = [sum(c != fc.FREE for c in row) for row in M.scls]
    assert sum(u > 0 for u in used) >= 2 and used[0] < 64, used
    # claims that hold several classes, words with accepted and rejected classes side by side
    M = cases["loop-keep"][2]["M"]
    assert max(len(c[1]) for c in M.claims) >= 3 and any(0 < bin(a[0]).count("1") < sum(c != fc.FREE for c in M.scls[0]) for a in M.acc)


def test_limit_cases_reach_every_outcome():
    """from the definition alone: what the cases with NodePool limits reach"""
    cases = {n: expect(n) for n in fc.CASES}
    made = collections.Counter((f[1], f[2]) for _, _, w in cases.values() if not w["setup_ret"] for f in w["facts"] if f[0] == "new_claim")
    assert sum(n for (ret, v), n in made.items() if ret == 2 and v[0] == fc.E_LIMITS) >= 10
    for stop in (fc.DECLINE_LIMIT_NODES, fc.DECLINE_LIMIT_EXCLUDES_TYPE, fc.DECLINE_LIMIT_STAGES, fc.DECLINE_CACHE_FULL_NEW_CLAIM):
        assert made[(0, stop)] >= 1, stop
    lf = collections.Counter(f[0] for _, _, w in cases.values() if not w["setup_ret"] for f in w["M"].limit_facts)
    print(sorted(lf.items()))
    assert lf["stage"] >= 40 and lf["skipped"] >= 20 and lf["verdict reused"] >= 20 and lf["verdict invalidated"] >= 10
    # the 33rd id: 31 stages behind the one template, one per claim from the first claim on, then no id left
    P, script, w = cases["limit-stages-33"]
    M, D = w["M"], w["D"]
    assert M.bail == fc.DECLINE_LIMIT_STAGES and len(D.real) == 32 and M.first_claim == 0 and [f[2] for f in M.limit_facts] == list(range(31)) and M.cur[0] == 31
    assert all(D.t_its[s] < D.t_its[s - 1] for s in range(1, 32)) and M.remaining[0][0] == 58 - 31 and all((c["tmplok"] >> 31) & 1 == c["tmplok"] & 1 for c in D.cls)
    # a limit that excludes its first type at a middle claim and at the last one; remaining counted down by the largest capacity that holds the pod
    assert cases["limit-middle-claim"][2]["M"].first_claim == 4 and cases["limit-last-claim"][2]["M"].first_claim == 3 == len(cases["limit-last-claim"][2]["M"].claims) - 1
    M = cases["limit-middle-claim"][2]["M"]
    assert M.remaining[0][0] < 25 and M.epoch == 1 + len(M.claims) and {f[0] for f in M.limit_facts} == {"stage", "skipped", "verdict reused", "verdict invalidated"}
    # two NodePools exhausting alternately: the stages' templates interleave
    D = cases["limit-two-pools"][2]["D"]
    assert D.real[3:15] == [0, 1] * 6
    # the nodes used up: skipped with limit stages, the engine's end without; a node left: no skip
    assert [r["aux"] & 0xFF for r in cases["limit-nodes-used-up"][2]["res"]] == [fc.E_LIMITS] * 3 and len(cases["limit-nodes-left"][2]["M"].claims) == 3
    assert cases["limit-nodes-used-up-without-stages"][2]["M"].bail == fc.DECLINE_LIMIT_NODES and cases["limit-excludes-without-stages"][2]["M"].bail == fc.DECLINE_LIMIT_EXCLUDES_TYPE
    # generated problems: limits on the first, the last and every resource, stages and skips among ordinary events
    for name in ("loop-limits", "loop-limits-4-rows"):
        M = cases[name][2]["M"]
        assert {"stage", "skipped", "verdict invalidated"} <= {f[0] for f in M.limit_facts} and M.claims, name
    assert cases["cache-full-new-claim"][2]["M"].bail == fc.DECLINE_CACHE_FULL_NEW_CLAIM and cases["cache-full-new-claim"][2]["n_ent"] == fc.K_GATE


def test_declines_cover_every_reason_on_both_sides():
    reasons = collections.Counter(f()[1] for f in fc.DECLINES.values())
    assert set(reasons) == {0, 1, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12}
    assert reasons[0] >= 10 and reasons[1] >= 4 and reasons[6] >= 3 and reasons[7] >= 6 and reasons[5] >= 2
