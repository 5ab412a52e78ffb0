"""The kernels behind the pack loop against their definitions: finalize (csrc/kernels.h finalize_body over csrc/go_sort.h, with the
sweep's claim_gather_body and slot_of indirection) and the fast engines' effective allocatable (eff_alloc_body).

THE DEFINITION is written here on plain Python values — sets, dicts, floats — from the reference's text, not from kernels.h:
  cheapest price   cloudprovider/types.go:336-355 (the comparator key of OrderByPrice: the cheapest available offering compatible with
                   the requirements) and scheduling/nodeclaim.go:391-403 (a claim that holds reservations launches only into them);
                   whether a requirement admits a zone or a capacity type is requirement.go:275-280 Has (reqalg_cases.has)
  order            types.go:338 sort.Slice: an unstable sort whose tie order is part of the result. The permutation comes from the
                   oracle's restatement of Go's pdqsort (sort_by_key) on the dense ranks of the prices, which make the same comparisons
  truncate         types.go:437-449 Truncate and :399-433 SatisfiesMinValues
  daemon requests  nodeclaim.go:353-377 addDaemonRequests over resources.MinResources (the intersection of keys: a group without any
                   daemon pod empties the running minimum); the groups in the order scheduler.go:985-1003 builds them
  effective allocatable   nodeclaim.go:558-566: a type stays iff requests + its group's overhead <= allocatable

A problem (make_problem) is a dict of such values; flat() turns it into the tables ksolve_test_finalize takes, run_finalize() drives
the entry point of a test build of the solver library (tests/emu/libksolve_emu.so on the host, tests/emu/libksolve_hooks.so on the
GPU), expected_finalize() is the definition's answer in the same shape, and mismatches() lists every field that differs. Nothing is
compared with a tolerance: no arithmetic happens on a price, so prices are compared as their 64 bits."""
import ctypes
import functools
import json
import os
import random

import numpy as np

import reqalg_cases as ra

U64, I64, U32, I32, U8, F64 = np.uint64, np.int64, np.uint32, np.int32, np.uint8, np.float64
DBL_MAX = 1.7976931348623157e308
OUT_FILL = 0xA5                       # the hook's outputs start as bytes of this
FILL_U32, FILL_U64 = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5
POISONS = (0xDEADBEEFCAFEF00D, 0x00000000FFFFFFFF)   # what unused slots and unwritten cold records hold; the answers must not depend on it
K_EFF_NEVER = -((1 << 30) - 1)
CT_VALUES = ("spot", "on-demand", "reserved", "burst")


# ------------------------------------------------------------------------------------------------ the definition: finalize
def admitted(space, reqs, key, n):
    """indices i < n of the key's dictionary values that the requirement set admits: Has(value), every value without the key"""
    r = reqs.get(key)
    return [i for i, v in enumerate(space.values[key][:n]) if r is None or ra.has(r, v)]


def type_prices(P, claim):
    """the claim's types in ascending index with the price OrderByPrice compares them by"""
    zones, cts = set(admitted(P["space"], claim["reqs"], "zone", P["n_zones"])), set(admitted(P["space"], claim["reqs"], "ct", P["n_cts"]))
    held = claim["held"]
    out = []
    for it in sorted(claim["its"]):
        if held:      # nodeclaim.go:391-403: only the reserved offerings it holds; their capacity type is `reserved` whatever the claim asked
            cands = [p for z, rid, p in P["resv"][it] if rid in held and z in zones]
        else:
            cands = [p for z, c, p in P["offers"][it] if z in zones and c in cts]
        out.append((it, min(cands, default=DBL_MAX)))
    return out


def dense_ranks(prices):
    rank = {p: i for i, p in enumerate(sorted(set(prices)))}
    return [rank[p] for p in prices]


def order_by_price(oracle, prices):
    """sort.Slice(its, price[i] < price[j]) as a permutation of positions"""
    if len(prices) < 2:
        return list(range(len(prices)))
    return oracle.evaluate({"fn": "sort_by_key", "keys": dense_ranks(prices)})


def values_count(P, kept, key):
    """SatisfiesMinValues' len(valuesForKey[key]): the distinct values of the kept types' requirements on the key (Values(): the stored
    set, whatever the complement flag)"""
    if key == "it":
        return len(kept)
    vals = set()
    for it in kept:
        r = P["it_reqs"][it].get(key)
        if r is not None:
            vals |= r.values
    return len(vals)


def truncate(P, claim, ordered):
    """-> (ordered_count, failed)"""
    n = len(ordered)
    keep = min(n, P["truncate_n"])
    failed = False
    if claim["minv_flag"] and not P["best_effort"]:
        for key, r in claim["reqs"].items():
            if r.min_values is not None and values_count(P, ordered[:keep], key) < r.min_values:
                failed = True
    return (n if failed else keep), failed


def daemon_requests(P, claim):
    t = claim["template"]
    t_its = sorted(P["t_its"][t])
    groups = [g for g in P["groups"][t] if g["its"] & P["t_its"][t]]
    groups.sort(key=lambda g: min(t_its.index(i) for i in g["its"] & P["t_its"][t]))      # first appearance over the prefiltered types
    cur = None
    for g in groups:
        if not (g["its"] & claim["its"]):
            continue
        ov = list(g["ov"]) if g["nonempty"] else None
        cur = ov if cur is None or ov is None else [min(a, b) for a, b in zip(cur, ov)]
    return cur if cur is not None else [0] * P["n_res"]


def expected_finalize(oracle, P):
    """What ksolve_test_finalize downloads for the problem's claims, from the definition alone."""
    C, n_its, nr = len(P["claim_slots"]), P["n_its"], P["n_res"]
    e = dict(cheapest=np.zeros(C, F64), daemon_requests=np.zeros((C, nr), I64))
    if P["truncate_n"]:
        e.update(sort_idx=np.full((C, n_its), FILL_U32, U32).view(I32), sort_price=np.full((C, n_its), FILL_U64, U64).view(F64),
                 ordered_count=np.zeros(C, U32), trunc_failed=np.zeros(C, U8))
    e["facts"] = []
    for c, s in enumerate(P["claim_slots"]):
        claim = P["slots"][s]
        tp = type_prices(P, claim)
        prices = [p for _, p in tp]
        e["cheapest"][c] = min(prices, default=DBL_MAX)
        e["daemon_requests"][c] = daemon_requests(P, claim)
        fact = dict(dbl_max=e["cheapest"][c] == DBL_MAX, n=len(tp))
        if P["truncate_n"]:
            perm = order_by_price(oracle, prices)
            ordered = [tp[i][0] for i in perm]
            sp = [prices[i] for i in perm]
            assert sp == sorted(sp)
            e["sort_idx"][c, :len(tp)] = ordered
            e["sort_price"][c, :len(tp)] = sp
            e["ordered_count"][c], e["trunc_failed"][c] = truncate(P, claim, ordered)
            tn = P["truncate_n"]
            fact.update(boundary_tie=len(sp) > tn and sp[tn - 1] == sp[tn], failed=bool(e["trunc_failed"][c]),
                        minv_ok=claim["minv_flag"] and not P["best_effort"] and not e["trunc_failed"][c])
        t = claim["template"]
        fact["groups"] = sum(1 for g in P["groups"][t] if g["its"] & claim["its"] and g["its"] & P["t_its"][t])
        e["facts"].append(fact)
    return e


# ------------------------------------------------------------------------------------------------ price families
def _family(name, n, i, rng_keys):
    if name == "ties":
        return rng_keys[i] % max(1, n // 8)
    if name == "sorted":
        return i // 3
    if name == "reversed":
        return (n - i) // 3
    if name == "three":
        return rng_keys[i] % 3
    if name == "period7":
        return i % 7
    if name == "two-runs":
        return i if i < n // 2 else i - n // 2
    if name == "organ-pipe":
        return min(i, n - i)
    if name == "mod13":
        return (i * 7919) % 13
    if name == "boundary":      # pairs of equal prices: one of them straddles any truncation boundary of the other parity
        return (rng_keys[i] % n + 1) // 2
    raise KeyError(name)


FAMILIES = ("ties", "sorted", "reversed", "three", "period7", "two-runs", "organ-pipe", "mod13", "boundary", "none")   # none: no offering at all in the zone


def zone_forms(space, n_zones, rng):
    """the requirement on the zone key in every form; int_bound only tells something on integer zones, and refuses everything on others"""
    vals = space.values["zone"][:n_zones]
    pick = lambda: rng.sample(vals, rng.randint(1, max(1, len(vals) - 1)))
    mid = str(10 * rng.randrange(n_zones))
    return {"undefined": None, "in": ra.new_requirement("zone", "In", None, *pick()), "notin": ra.new_requirement("zone", "NotIn", None, *pick()),
            "exists": ra.new_requirement("zone", "Exists", None), "dne": ra.new_requirement("zone", "DoesNotExist", None),
            "gt": ra.new_requirement("zone", "Gt", None, mid), "lt": ra.new_requirement("zone", "Lt", None, str(int(mid) + 11))}


FORMS = ("undefined", "in", "notin", "exists", "dne", "gt", "lt")


def make_problem(seed, n_claims, n_its, n_zones=4, n_cts=2, int_zones=True, truncate_n=10, best_effort=False, n_templates=3, resv=True, n_res=3, only_cell=None,
                 plain_claims=False, killer=False):
    """A finalize problem on plain values. Claim i takes the zone i % n_zones as its price family's (In [that zone]) in half of the claims and
    one of FORMS otherwise. only_cell: the one (zone, capacity type) any type is offered in."""
    rng = random.Random(seed * 7919 + n_claims * 31 + n_its)
    zone_vals = [str(10 * z) if int_zones else f"zone-{z}" for z in range(n_zones)] + ["5", "other"]    # (two values that are no zone)
    n_fam = 70 if n_its >= 70 else max(2, n_its)
    space = ra.Space([("zone", zone_vals), ("ct", CT_VALUES), ("it", [f"t{i}" for i in range(n_its)]), ("family", [f"f{i}" for i in range(max(n_fam, 70))]),
                      ("arch", ["a", "b"])], key_it="it")
    P = dict(space=space, n_its=n_its, n_zones=n_zones, n_cts=n_cts, n_res=n_res, truncate_n=truncate_n, best_effort=best_effort, n_templates=n_templates)
    fams = [FAMILIES[(seed * 3 + z) % len(FAMILIES)] for z in range(n_zones)]
    if killer:      # zone 0: keys on which pdqsort uses up its bad partitions and heap-sorts (tests/tools/pdqsort_killer.cpp), every type offered
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"pdqsort_killer_{n_its}.json")) as fh:
            killer_keys = json.load(fh)
        fams[0] = "killer"
    P["zone_family"] = fams
    rk = [rng.randrange(1 << 30) for _ in range(n_its)]
    offers, it_reqs = [], []
    for it in range(n_its):
        o = []
        for z in range(n_zones):
            if fams[z] == "none" or (rng.random() < 0.1 and n_its > 3 and fams[z] != "killer"):
                continue
            base = 0.25 * (killer_keys[it] if fams[z] == "killer" else _family(fams[z], n_its, it, rk)) + 1.0 + 64.0 * z
            o.append((z, it % n_cts, base))
            if n_cts > 1 and rng.random() < 0.5:
                o.append((z, (it + 1) % n_cts, base + 4096.0))
        if only_cell is not None:
            o = [(only_cell[0], only_cell[1], 2.5 + it)] if it % 2 == 0 or n_its == 1 else []
        offers.append(o)
        r = {"it": ra.new_requirement("it", "In", None, f"t{it}")}
        if it % 5 != 4:
            r["family"] = ra.new_requirement("family", "NotIn" if it % 7 == 3 else "In", None, f"f{(it * 3) % n_fam}")
        it_reqs.append(r)
    P["offers"], P["it_reqs"] = offers, it_reqs
    # reservation offerings: ids 0 and 63 among them, cheaper and dearer than any ordinary offering
    ids = (0, 63, 5, 31)
    P["resv"] = [[(rng.randrange(n_zones), rng.choice(ids), rng.choice((0.001, 0.5, 7.75, 1e6))) for _ in range(rng.choice((0, 0, 1, 3)))] for _ in range(n_its)] if resv else None
    # templates, their prefiltered types and their daemon-overhead groups (stored in an order that is not the order of first appearance)
    P["t_its"], P["groups"] = [], []
    n_groups = {0: 2, 1: 5, 2: 1, 31: 5}
    for t in range(n_templates):
        tits = {i for i in range(n_its) if t == 0 or (i + t) % 3 != 0 or n_its < 3}
        k = n_groups.get(t, 0)
        gs = []
        if k:
            order = list(range(k))
            rng.shuffle(order)
            for j in order:
                members = {i for i in tits if ((i * 7 + 3) % k == j) and (k == 1 or i % 11 != 5)}
                gs.append(dict(its=members, ov=[rng.choice((0, 100, 250, 1 << 40)) for _ in range(n_res)], nonempty=rng.random() < 0.7))
            if k > 1:
                gs.insert(rng.randrange(len(gs) + 1), dict(its=set(range(n_its)) - tits, ov=[1] * n_res, nonempty=True))    # a group with no prefiltered type
        P["t_its"].append(tits)
        P["groups"].append(gs)
    claims = []
    templates = [t for t in range(n_templates) if t in n_groups or n_templates <= 3 or t == 5]      # (template 5 of 32: no group at all)
    for i in range(n_claims):
        t = rng.choice(templates)
        tits = sorted(P["t_its"][t])
        dens = rng.choice((1.0, 0.9, 0.5, 0.1))
        its = {x for x in tits if rng.random() < dens}
        if rng.random() < 0.05 and tits:
            its = {x for x in tits if x % 11 == 5}      # only types no group of a several-group template holds
        reqs = {}
        zf = zone_forms(space, n_zones, rng)
        form = "in-family" if i % 2 == 0 else FORMS[(i // 2) % len(FORMS)]
        if plain_claims:
            form = "in-family"
        if form == "in-family":
            reqs["zone"] = ra.new_requirement("zone", "In", None, zone_vals[(i // 2) % n_zones])
        elif zf[form] is not None:
            reqs["zone"] = zf[form]
        cform = FORMS[(i // 3) % len(FORMS)] if not plain_claims else "undefined"
        ctv = list(CT_VALUES[:n_cts])
        creq = {"undefined": None, "in": ra.new_requirement("ct", "In", None, *rng.sample(ctv, rng.randint(1, n_cts))), "notin": ra.new_requirement("ct", "NotIn", None, rng.choice(ctv)),
                "exists": ra.new_requirement("ct", "Exists", None), "dne": ra.new_requirement("ct", "DoesNotExist", None),
                "gt": ra.new_requirement("ct", "Gt", None, "0"), "lt": ra.new_requirement("ct", "Lt", None, "9")}[cform]
        if creq is not None and (i % 5 == 0 or cform not in ("dne", "gt", "lt")):
            reqs["ct"] = creq
        if rng.random() < 0.3:
            reqs["arch"] = ra.new_requirement("arch", "Gt", None, "3")      # a bound on a key finalize never looks at: a cold record all the same
        held = set(rng.sample(ids, rng.randint(1, 3))) if resv and rng.random() < 0.2 and not plain_claims else set()
        claim = dict(reqs=reqs, its=its, template=t, held=held, minv_flag=False)
        if truncate_n and rng.random() < 0.4 and not plain_claims:
            # minValues on the instance-type key or on the two-word family key: met exactly or short by one for what the definition keeps
            key = rng.choice(("it", "family"))
            tp = type_prices(P, claim)
            prices = [p for _, p in tp]
            ordered = [tp[j][0] for j in _host_order(prices)]
            have = values_count(P, ordered[:min(len(ordered), truncate_n)], key)
            mv = max(0, have + rng.choice((0, 0, 1)))
            reqs[key] = ra.Req(key, [f"t{x}" for x in its] if key == "it" else [], key != "it", None, None, mv)
            claim["minv_flag"] = True
        claims.append(claim)
    if killer:      # claim 0: every type, in zone 0 alone
        claims[0] = dict(reqs={"zone": ra.new_requirement("zone", "In", None, zone_vals[0])}, its=set(range(n_its)), template=0, held=set(), minv_flag=False)
    P["slots"], P["claim_slots"] = claims, list(range(n_claims))
    return P


_order_fn = [None]


def _host_order(prices):
    return _order_fn[0](prices)


def use_oracle(oracle):
    """the generator places minValues next to what the definition keeps, and the definition's order is the oracle's"""
    _order_fn[0] = lambda prices: order_by_price(oracle, prices)


def with_slots(P, kind, seed=1):
    """the problem's claims behind a slot_of indirection: `identity`, a random `permutation` into a larger array whose other slots are
    unused, or `duplicates` (several claims read the same slot)"""
    Q = dict(P)
    n = len(P["slots"])
    rng = random.Random(seed)
    if kind == "identity":
        Q["slot_of"] = list(range(n))
    elif kind == "permutation":
        S = n + n // 3 + 2
        where = rng.sample(range(S), n)
        slots = [None] * S
        for c, s in enumerate(where):
            slots[s] = P["slots"][c]
        Q["slots"], Q["slot_of"] = slots, where
    elif kind == "duplicates":
        Q["slot_of"] = [rng.randrange(n) for _ in range(n + 3)]
    Q["claim_slots"] = Q["slot_of"]
    return Q


# ------------------------------------------------------------------------------------------------ the flat form and the entry point
def _bits(words, members):
    out = np.zeros(words, U64)
    for i in members:
        out[i >> 6] |= U64(1 << (i & 63))
    return out


class _Reqsets(ctypes.Structure):
    _fields_ = [("n", ctypes.c_uint32)] + [(f, ctypes.c_void_p) for f in ("mask", "defined", "complement", "has_gte", "has_lte", "gte", "lte", "min_values")]


def _reqsets(t, n, keep):
    cols = [np.ascontiguousarray(t[f]) if t[f] is not None else None for f in ("mask", "defined", "complement", "has_gte", "has_lte", "gte", "lte", "minv")]
    keep += cols
    return _Reqsets(n, *[c.ctypes.data if c is not None else None for c in cols])


class _FinalizeIn(ctypes.Structure):
    _fields_ = [("n_keys", ctypes.c_uint32), ("key_word_off", ctypes.c_void_p), ("value_int", ctypes.c_void_p), ("value_is_int", ctypes.c_void_p), ("value_valid", ctypes.c_void_p),
                ("key_zone", ctypes.c_int32), ("key_ct", ctypes.c_int32), ("key_it", ctypes.c_int32),
                ("n_its", ctypes.c_uint32), ("n_zones", ctypes.c_uint32), ("n_cts", ctypes.c_uint32), ("n_res", ctypes.c_uint32), ("n_templates", ctypes.c_uint32),
                ("it_off_avail", ctypes.c_void_p), ("it_off_price", ctypes.c_void_p), ("it_reqs", ctypes.POINTER(_Reqsets)),
                ("dg_first", ctypes.c_void_p), ("dg_ov", ctypes.c_void_p), ("dg_its", ctypes.c_void_p), ("dg_nonempty", ctypes.c_uint64), ("t_its", ctypes.c_void_p),
                ("it_resv_first", ctypes.c_void_p), ("resv_zone", ctypes.c_void_p), ("resv_id", ctypes.c_void_p), ("resv_price", ctypes.c_void_p),
                ("truncate_n", ctypes.c_uint32), ("best_effort", ctypes.c_uint32), ("n_claims", ctypes.c_uint32), ("n_slots", ctypes.c_uint32),
                ("slot_of", ctypes.c_void_p), ("slot_used", ctypes.c_void_p), ("c_reqs", ctypes.POINTER(_Reqsets)), ("c_minv_flag", ctypes.c_void_p),
                ("c_its", ctypes.c_void_p), ("c_template", ctypes.c_void_p), ("c_reserved", ctypes.c_void_p), ("poison", ctypes.c_uint64)]


class _FinalizeOut(ctypes.Structure):
    _fields_ = [(f, ctypes.c_void_p) for f in ("cheapest", "daemon_requests", "sort_idx", "sort_price", "ordered_count", "trunc_failed")] + \
               [("hot_words", ctypes.c_uint32), ("cold_words", ctypes.c_uint32)] + [(f, ctypes.c_void_p) for f in ("rec_hot", "rec_cold", "g_hot", "g_cold", "g_reserved")]


class _EffIo(ctypes.Structure):
    _fields_ = [("n_templates", ctypes.c_uint32), ("n_its", ctypes.c_uint32), ("n_res", ctypes.c_uint32), ("tmpl_ov", ctypes.c_uint32)] + \
               [(f, ctypes.c_void_p) for f in ("it_alloc", "dg_first", "dg_ov", "dg_its", "it_eff")]


_libs = {}


def _lib(path):
    if path not in _libs:
        lib = ctypes.CDLL(os.path.abspath(path))
        lib.ksolve_test_finalize.restype = ctypes.c_int
        lib.ksolve_test_finalize.argtypes = [ctypes.POINTER(_FinalizeIn), ctypes.POINTER(_FinalizeOut)]
        lib.ksolve_test_eff_alloc.restype = ctypes.c_int
        lib.ksolve_test_eff_alloc.argtypes = [ctypes.POINTER(_EffIo)]
        _libs[path] = lib
    return _libs[path]


JUNK_PRICE = 1e-9      # what the price table holds in a cell that is not available: below every price


def flat(P):
    """the tables of ksolve_test_finalize_in but for the poison"""
    sp, n_its, nr, nt = P["space"], P["n_its"], P["n_res"], P["n_templates"]
    iw = (n_its + 63) // 64
    f = dict(iw=iw)
    f["avail"] = np.zeros(n_its, U64)
    f["price"] = np.full((n_its, 64), JUNK_PRICE, F64)
    for it, o in enumerate(P["offers"]):
        for z, c, p in o:
            f["avail"][it] |= U64(1 << (z * 4 + c))
            f["price"][it, z * 4 + c] = p
    f["it_reqs"] = ra.encode_sets(sp, P["it_reqs"])
    first, ov, gits, nonempty = [0], [], [], 0
    for t in range(nt):
        for g in P["groups"][t]:
            if g["nonempty"]:
                nonempty |= 1 << len(ov)
            ov.append(g["ov"])
            gits.append(_bits(iw, g["its"]))
        first.append(len(ov))
    f["dg_first"], f["dg_nonempty"] = np.array(first, I32), nonempty
    f["dg_ov"] = np.array(ov or [[0] * nr], I64).reshape(-1, nr)
    f["dg_its"] = np.array(gits or [np.zeros(iw, U64)], U64).reshape(-1, iw)
    f["t_its"] = np.array([_bits(iw, s) for s in P["t_its"]], U64).reshape(nt, iw)
    if P["resv"] is not None:
        rf, rz, ri, rp = [0], [], [], []
        for it in range(n_its):
            for z, rid, p in P["resv"][it]:
                rz.append(z), ri.append(rid), rp.append(p)
            rf.append(len(rz))
        f["resv"] = (np.array(rf, U32), np.array(rz + [0], U8), np.array(ri + [0], U8), np.array(rp + [0.0], F64))
    else:
        f["resv"] = None
    slots = P["slots"]
    S = len(slots)
    f["slot_used"] = np.array([s is not None for s in slots], U8)
    f["c_reqs"] = ra.encode_sets(sp, [s["reqs"] if s else {} for s in slots], junk=True)
    f["c_minv_flag"] = np.array([bool(s and s["minv_flag"]) for s in slots], U8)
    f["c_its"] = np.array([_bits(iw, s["its"] if s else ()) for s in slots], U64).reshape(S, iw)
    f["c_template"] = np.array([s["template"] if s else 0 for s in slots], U32)
    f["c_reserved"] = np.array([sum(1 << r for r in s["held"]) if s else 0 for s in slots], U64) if P["resv"] is not None else None
    f["slot_of"] = np.array(P["slot_of"], U32) if P.get("slot_of") is not None else None
    if "raw_claims" in P:      # the claims as downloaded columns (chain_problem)
        f.update(P["raw_claims"])
    return f


FINALIZE_FIELDS = ("cheapest", "daemon_requests", "sort_idx", "sort_price", "ordered_count", "trunc_failed")


def run_finalize(lib_path, P, poison=POISONS[0], c_reserved=True):
    """ksolve_test_finalize on the problem: one be_launch_finalize (and one be_launch_claim_gather behind a slot_of). Every output
    starts as bytes of OUT_FILL. c_reserved False: the reservation tables without the claims' column."""
    f, sp = flat(P), P["space"]
    keep = []
    C, S, n_its, nr = len(P["claim_slots"]), len(P["slots"]), P["n_its"], P["n_res"]
    it_reqs, c_reqs = _reqsets(f["it_reqs"], n_its, keep), _reqsets(f["c_reqs"], S, keep)
    rv = f["resv"]
    a = _FinalizeIn(sp.nk, sp.off.ctypes.data, sp.value_int.ctypes.data, sp.value_is_int.ctypes.data, sp.value_valid.ctypes.data,
                    sp.kidx["zone"], sp.kidx["ct"], sp.kidx["it"], n_its, P["n_zones"], P["n_cts"], nr, P["n_templates"],
                    f["avail"].ctypes.data, f["price"].ctypes.data, ctypes.pointer(it_reqs),
                    f["dg_first"].ctypes.data, f["dg_ov"].ctypes.data, f["dg_its"].ctypes.data, f["dg_nonempty"], f["t_its"].ctypes.data,
                    *([x.ctypes.data for x in rv] if rv else [None] * 4),
                    P["truncate_n"], int(P["best_effort"]), C, S, f["slot_of"].ctypes.data if f["slot_of"] is not None else None, f["slot_used"].ctypes.data,
                    ctypes.pointer(c_reqs), f["c_minv_flag"].ctypes.data, f["c_its"].ctypes.data, f["c_template"].ctypes.data,
                    f["c_reserved"].ctypes.data if rv and c_reserved else None, poison)
    g = dict(cheapest=np.zeros(C, F64), daemon_requests=np.zeros((C, nr), I64), sort_idx=np.zeros((C, n_its), I32), sort_price=np.zeros((C, n_its), F64),
             ordered_count=np.zeros(C, U32), trunc_failed=np.zeros(C, U8))
    o = _FinalizeOut(*[g[k].ctypes.data for k in FINALIZE_FIELDS])
    # the record sizes are the hook's to say: room for the largest layout the library takes
    rec_hot, rec_cold = np.zeros(S * (sp.rw + f["iw"] + 2 * nr + 4), U64), np.zeros(S * (3 * sp.nk), U64)
    g_hot, g_cold, g_resv = np.zeros(C * (sp.rw + f["iw"] + 2 * nr + 4), U64), np.zeros(C * (3 * sp.nk), U64), np.zeros(C, U64)
    o.rec_hot, o.rec_cold, o.g_hot, o.g_cold, o.g_reserved = rec_hot.ctypes.data, rec_cold.ctypes.data, g_hot.ctypes.data, g_cold.ctypes.data, g_resv.ctypes.data
    st = _lib(lib_path).ksolve_test_finalize(ctypes.byref(a), ctypes.byref(o))
    assert st == 0, f"ksolve_test_finalize: status {st}"
    if not P["truncate_n"]:
        for k in ("sort_idx", "sort_price", "ordered_count", "trunc_failed"):
            del g[k]
    hw, cw = o.hot_words, o.cold_words
    g["rec_hot"], g["rec_cold"] = rec_hot[:S * hw].reshape(S, hw), rec_cold[:S * cw].reshape(S, cw)
    if f["slot_of"] is not None:
        g["g_hot"], g["g_cold"], g["g_reserved"] = g_hot[:C * hw].reshape(C, hw), g_cold[:C * cw].reshape(C, cw), g_resv
        g["held_by_slot"] = f["c_reserved"] if f["c_reserved"] is not None and c_reserved else np.zeros(S, U64)
    return g


def _bits_of(a):
    a = np.ascontiguousarray(a)
    return a.view(U64) if a.dtype == F64 else a


def mismatches(got, want, fields=FINALIZE_FIELDS):
    """every field and claim in which two answers differ (prices by their bits)"""
    bad = []
    for k in fields:
        if k not in want and k not in got:
            continue
        g, w = _bits_of(got[k]), _bits_of(want[k])
        if g.shape != w.shape:
            bad.append((k, "shape", g.shape, w.shape))
            continue
        rows = np.nonzero((g != w).reshape(len(g), -1).any(axis=1))[0]
        bad += [(k, int(c)) for c in rows]
    return bad


def gather_mismatches(P, got):
    """the gathered records are the packed records of the slots the claims name, word for word"""
    so = np.array(P["slot_of"])
    bad = [k for k, src in (("g_hot", got["rec_hot"][so]), ("g_cold", got["rec_cold"][so])) if not np.array_equal(got[k], src)]
    if not np.array_equal(got["g_reserved"], np.asarray(got["held_by_slot"], U64)[so]):
        bad.append("g_reserved")
    return bad


# ------------------------------------------------------------------------------------------------ the case lists
# (claims, instance types): the launch is 256 threads per block; 12 and 50 are pdqsort's thresholds, 64 the type word
FINALIZE_SIZES = ((1, 1), (255, 12), (256, 13), (257, 49), (1, 50), (255, 51), (256, 63), (257, 64), (255, 65), (256, 257), (257, 1000), (1, 1000))
FINALIZE_CASES = {f"{c}x{n}": dict(seed=i, n_claims=c, n_its=n, int_zones=i % 2 == 0, truncate_n=(10, 60, 4)[i % 3] if n > 1 else 1) for i, (c, n) in enumerate(FINALIZE_SIZES)}
FINALIZE_CASES.update({
    "cell-63": dict(seed=20, n_claims=40, n_its=9, n_zones=16, n_cts=4, only_cell=(15, 3)),
    "zones-16": dict(seed=21, n_claims=64, n_its=65, n_zones=16, n_cts=4, int_zones=False, truncate_n=12),
    "template-31": dict(seed=22, n_claims=30, n_its=40, n_templates=32),
    "best-effort": dict(seed=23, n_claims=80, n_its=51, best_effort=True, truncate_n=7),
    "no-truncate": dict(seed=24, n_claims=33, n_its=20, truncate_n=0),
    "no-reservations": dict(seed=25, n_claims=33, n_its=20, resv=False),
    "one-resource": dict(seed=26, n_claims=33, n_its=20, n_res=1),
    "eight-resources": dict(seed=27, n_claims=33, n_its=70, n_res=8),
    "heapsort": dict(seed=28, n_claims=3, n_its=1000, killer=True, truncate_n=600),
})
SLOT_CASE = dict(seed=30, n_claims=70, n_its=66, truncate_n=9)


@functools.lru_cache(maxsize=None)
def finalize_problem(name):
    return make_problem(**(SLOT_CASE if name == "slots" else FINALIZE_CASES[name]))


_expected = {}


def finalize_expected(oracle, name):
    """computed once per session and left alone"""
    if name not in _expected:
        _expected[name] = expected_finalize(oracle, finalize_problem(name))
    return _expected[name]


# ------------------------------------------------------------------------------------------------ single differences
def single_base():
    """16 claims of which claim 0 alone admits zone 0 and alone uses template 2; no minValues, no reservations held"""
    P = make_problem(seed=40, n_claims=16, n_its=30, truncate_n=8, plain_claims=True, resv=False)
    fams = P["zone_family"]
    assert fams[0] != "none"
    zv = P["space"].values["zone"]
    for i, c in enumerate(P["slots"]):
        c["reqs"]["zone"] = ra.new_requirement("zone", "In", None, zv[0] if i == 0 else zv[1 + i % 3])
        c["template"] = 2 if i == 0 else i % 2
        c["its"] = set(sorted(P["t_its"][c["template"]])[i % 3::2])
    P["groups"][2][0]["nonempty"] = True
    return P


def single_changes(P):
    """(name, changed problem, the fields that may differ for claim 0, the field that must)"""
    import copy
    c0 = P["slots"][0]
    tp = [(it, p) for it, p in type_prices(P, c0) if p < DBL_MAX]
    out = []
    Q = copy.deepcopy(P)                                        # one price lowered below the minimum
    it = max(tp, key=lambda x: x[1])[0]
    Q["offers"][it] = [(z, c, 0.125 if z == 0 else p) for z, c, p in Q["offers"][it]]
    out.append(("price lowered", Q, {"cheapest", "sort_idx", "sort_price"}, "cheapest"))
    Q = copy.deepcopy(P)                                        # one availability bit cleared: the cheapest type's offering in the zone
    it = min(tp, key=lambda x: x[1])[0]
    Q["offers"][it] = [(z, c, p) for z, c, p in Q["offers"][it] if z != 0]
    out.append(("availability cleared", Q, {"cheapest", "sort_idx", "sort_price"}, "sort_price"))
    Q = copy.deepcopy(P)                                        # one type removed from the claim
    Q["slots"][0]["its"].discard(it)
    out.append(("type removed", Q, {"cheapest", "sort_idx", "sort_price", "ordered_count", "daemon_requests"}, "sort_idx"))
    Q = copy.deepcopy(P)                                        # one group's overhead lowered in one resource
    g = Q["groups"][2][0]
    g["ov"] = list(g["ov"])
    g["ov"][1] = -7
    out.append(("overhead lowered", Q, {"daemon_requests"}, "daemon_requests"))
    return out


# ------------------------------------------------------------------------------------------------ the effective allocatable
def expected_eff(E):
    """allocatable less the overhead of the type's group in the template; rows outside tmpl_ov keep what they held"""
    nt, n_its, nr = E["n_templates"], E["n_its"], E["n_res"]
    out = E["fill"].copy()
    for t in range(nt):
        if not (E["tmpl_ov"] >> t) & 1:
            continue
        gs = E["groups"][t]
        for it in range(n_its):
            g = gs[0] if len(gs) == 1 else next((g for g in gs if it in g["its"]), None)
            for r in range(nr):
                out[t, r, it] = K_EFF_NEVER if g is None else E["alloc"][r][it] - g["ov"][r]
    return out


EFF_CASES = {f"{n}its-{nt}t-{nr}r": (n, nt, nr) for n, nt, nr in ((1, 1, 1), (63, 2, 4), (64, 1, 8), (65, 2, 1), (257, 2, 4), (257, 32, 4), (64, 32, 8), (63, 1, 4))}


@functools.lru_cache(maxsize=None)
def eff_case(name):
    n_its, nt, nr = EFF_CASES[name]
    rng = random.Random(n_its * 1000 + nt * 10 + nr)
    big = 1 << 62
    alloc = [[rng.choice((0, 1, 4000, big - 3, -5, rng.randrange(1 << 40))) for _ in range(n_its)] for _ in range(nr)]
    groups = []
    for t in range(nt):
        k = 1 if (t % 3 == 0 or nt == 32 and t != 31) else 3
        gs = []
        for j in range(k):
            # a type in two groups (the first one counts), types in none; a one-group template whose group does not hold every type
            members = {i for i in range(n_its) if (i % 4 == j or i % 8 == j + 1) and i % 9 != 7} if k > 1 else {i for i in range(n_its) if i % 2}
            gs.append(dict(its=members, ov=[rng.choice((0, 7, 5000, big, 1 << 41)) for _ in range(nr)]))
        groups.append(gs)
    tmpl_ov = 1 << 31 if nt == 32 else (0b10 if nt == 2 and n_its == 65 else (1 << nt) - 1)
    fill = np.full((nt, nr, n_its), 0x5EEDFACE5EEDFACE, I64)
    return dict(n_templates=nt, n_its=n_its, n_res=nr, tmpl_ov=tmpl_ov, alloc=alloc, groups=groups, fill=fill)


def run_eff(lib_path, E):
    nt, n_its, nr = E["n_templates"], E["n_its"], E["n_res"]
    iw = (n_its + 63) // 64
    alloc = np.array(E["alloc"], I64).reshape(nr, n_its)
    first, ov, gits = [0], [], []
    for gs in E["groups"]:
        for g in gs:
            ov.append(g["ov"]), gits.append(_bits(iw, g["its"]))
        first.append(len(ov))
    first, ov, gits = np.array(first, I32), np.array(ov, I64).reshape(-1, nr), np.array(gits, U64).reshape(-1, iw)
    eff = E["fill"].copy()
    io = _EffIo(nt, n_its, nr, E["tmpl_ov"], alloc.ctypes.data, first.ctypes.data, ov.ctypes.data, gits.ctypes.data, eff.ctypes.data)
    st = _lib(lib_path).ksolve_test_eff_alloc(ctypes.byref(io))
    assert st == 0, f"ksolve_test_eff_alloc: status {st}"
    return eff


# ------------------------------------------------------------------------------------------------ the cursor engine's claim records
# THE DEFINITION, from the comment block of FastRecordArgs (fast_engine.h) and requirement.go:181-214 (Intersection of concrete sets:
# an In set that meets anything is an In set again, complement off, bounds dropped): a claim's requirement set is its template's, but
# for the keys pods select on (the VARIABLE keys). Such a key with its guard bit CLEAR is a concrete set — the values of its field;
# with the guard bit SET the claim still holds what the template has on the key, or nothing. The claim's types are those of its
# requirement-set cache entry that exist and whose effective allocatable (of the REAL template behind a limit stage) holds the requests.
NOT_PLACED = 0xFFFFFFFF


def make_records(seed, n_claims, n_its, nv, wide=False, extra_key=False, lim=True, n_pods=200):
    """wide: a dictionary of twelve small keys behind zone / ct / it (the most variable keys the 56 bits hold); otherwise the finalize
    problems' dictionary, so that the records can go on into ksolve_test_finalize"""
    rng = random.Random(seed * 131 + n_claims * 7 + n_its)
    P = make_problem(seed, 1, n_its, truncate_n=5, plain_claims=True, resv=False)
    P["t_its"] = [set(range(n_its)) for _ in P["t_its"]]      # (a cache entry's types are not cut to a template's here)
    if wide or extra_key:
        keys = [(k, P["space"].values[k]) for k in P["space"].keys]
        keys += [(f"k{j}", ["1", "2", "x"]) for j in range(12)] if wide else [("extra", ["p", "q", "r"])]
        P["space"] = ra.Space(keys, key_it="it")
    sp, nt, nr = P["space"], 3, P["n_res"]
    zv = sp.values["zone"]
    small = [k for k in sp.keys if k not in ("it", "family")]
    var_keys = {0: [], 1: ["zone"], 3: ["zone", "ct", small[-1]], 12: [f"k{j}" for j in range(12)]}[nv]      # (small[-1]: a field in the last word)
    R = dict(P=P, space=sp, n_its=n_its, n_res=nr, n_templates=nt, var_keys=var_keys, poison=POISONS[0])
    last = small[-1]
    R["templates"] = [
        {},
        {"zone": ra.new_requirement("zone", "NotIn", None, zv[1]), last: ra.new_requirement(last, "Exists", None)},       # complement keys
        {"zone": ra.new_requirement("zone", "Gt", None, "5"), "ct": ra.new_requirement("ct", "In", None, "spot", "on-demand"), last: ra.new_requirement(last, "Lt", None, "2")},   # bounds
    ]
    R["alloc"] = [[rng.randrange(20, 100) for _ in range(n_its)] for _ in range(nr)]
    R["tmpl_ov"] = 0b110      # template 0 reads it_alloc itself
    R["eff"] = [[[(K_EFF_NEVER if (it + t) % 9 == 4 else R["alloc"][r][it] - 3 * t - r) for it in range(n_its)] for r in range(nr)] for t in range(nt)]
    R["real"] = ([0, 1, 2, 1, 2, 0, 2] + [0] * 25) if lim else None
    n_ent = 7
    iw = (n_its + 63) // 64
    R["ent_its"] = [{i for i in range(n_its) if rng.random() < (0.0 if e == 3 else 0.8)} for e in range(n_ent)]      # (entry 3: all-zero words)
    R["ent_junk"] = [set(range(n_its, iw * 64)) if e % 2 == 0 else set() for e in range(n_ent)]                      # bits past n_its that must not survive
    claims = []
    for c in range(n_claims):
        stage = rng.randrange(7 if lim else nt)
        t = R["real"][stage] if lim else stage
        ent = rng.randrange(n_ent)
        fields = {k: (rng.random() < 0.4, set(rng.sample(sp.values[k], rng.randint(1, len(sp.values[k]))))) for k in var_keys}
        eff = R["eff"][t] if (R["tmpl_ov"] >> t) & 1 else R["alloc"]
        cand = sorted(i for i in R["ent_its"][ent] if eff[0][i] != K_EFF_NEVER)
        if cand and c % 3 != 2:      # a request equal to one type's effective allocatable, or above it by one in one resource
            it = cand[c % len(cand)]
            req = [eff[r][it] for r in range(nr)]
            if c % 3 == 1:
                req[c % nr] += 1
        else:
            req = [rng.randrange(0, 60) for _ in range(nr)]
        claims.append(dict(stage=stage, ent=ent, fields=fields, req=req + [0x7A7A7A7 for _ in range(4 - nr)], npods=rng.randrange(1, 1 << 31), hostseq=rng.randrange(1 << 32)))
    R["claims"] = claims
    R["sorted"] = rng.sample(range(n_pods), n_pods)
    R["q_claim"] = [NOT_PLACED if rng.random() < 0.3 else rng.randrange(n_claims) for _ in range(n_pods)]
    R["q_cnt"] = [rng.randrange(1 << 20) for _ in range(n_pods)]
    return R


def record_reqs(R, claim):
    """the claim's requirement set, and its template"""
    t = R["real"][claim["stage"]] if R["real"] is not None else claim["stage"]
    reqs = dict(R["templates"][t])
    for key in R["var_keys"]:
        guard, values = claim["fields"][key]
        if not guard:
            reqs[key] = ra.Req(key, values, False)
    return reqs, t


def expected_records(R):
    sp, n_its, nr, C = R["space"], R["n_its"], R["n_res"], len(R["claims"])
    iw = (n_its + 63) // 64
    rows, e = [], dict(its=np.zeros((C, iw), U64), total=np.zeros((C, nr), I64), head=np.zeros((C, nr), I64), tmpl=np.zeros(C, U32), npods=np.zeros(C, U32),
                       host_seq=np.zeros(C, U32), flags=np.zeros(C, U32))
    for c, claim in enumerate(R["claims"]):
        reqs, t = record_reqs(R, claim)
        rows.append(reqs)
        eff = R["eff"][t] if (R["tmpl_ov"] >> t) & 1 else R["alloc"]
        e["its"][c] = _bits(iw, [i for i in R["ent_its"][claim["ent"]] if i < n_its and all(claim["req"][r] <= eff[r][i] for r in range(nr))])
        e["total"][c], e["tmpl"][c], e["npods"][c], e["host_seq"][c] = claim["req"][:nr], t, claim["npods"], claim["hostseq"]
    t = ra.encode_sets(sp, rows)
    e.update(mask=t["mask"], defined=t["defined"], complement=t["complement"], has_gte=t["has_gte"], has_lte=t["has_lte"], gte=t["gte"], lte=t["lte"], minv=t["minv"])
    e["cold_written"] = (t["has_gte"] | t["has_lte"]) != 0
    n_pods = len(R["sorted"])
    e["assign"], e["slot"] = np.full(n_pods, R["poison"] & 0xFFFFFFFF, U32).view(I32), np.full(n_pods, R["poison"] & 0xFFFFFFFF, U32)
    for i, p in enumerate(R["sorted"]):
        if R["q_claim"][i] != NOT_PLACED:
            e["assign"][p], e["slot"][p] = R["q_claim"][i], R["q_cnt"][i]
    e["rows"] = rows
    return e


class _RecordsIn(ctypes.Structure):
    _fields_ = [("n_keys", ctypes.c_uint32), ("key_word_off", ctypes.c_void_p), ("value_int", ctypes.c_void_p), ("value_is_int", ctypes.c_void_p), ("value_valid", ctypes.c_void_p),
                ("n_its", ctypes.c_uint32), ("n_res", ctypes.c_uint32), ("n_templates", ctypes.c_uint32), ("tmpl_reqs", ctypes.POINTER(_Reqsets)),
                ("it_alloc", ctypes.c_void_p), ("it_eff", ctypes.c_void_p), ("tmpl_ov", ctypes.c_uint32), ("nv", ctypes.c_uint32),
                ("vkey", ctypes.c_void_p), ("voff", ctypes.c_void_p), ("vwidth", ctypes.c_void_p), ("vword", ctypes.c_void_p), ("lim_real", ctypes.c_void_p),
                ("n_claims", ctypes.c_uint32), ("n_ent", ctypes.c_uint32), ("c_vmask", ctypes.c_void_p), ("c_req", ctypes.c_void_p), ("c_ent", ctypes.c_void_p), ("ent_its", ctypes.c_void_p),
                ("c_npods", ctypes.c_void_p), ("c_hostseq", ctypes.c_void_p), ("n_pods", ctypes.c_uint32), ("sorted", ctypes.c_void_p), ("q_claim", ctypes.c_void_p), ("q_cnt", ctypes.c_void_p),
                ("poison", ctypes.c_uint64)]


RECORD_COLS = ("mask", "its", "total", "head", "defined", "complement", "has_gte", "has_lte", "tmpl", "npods", "host_seq", "flags", "gte", "lte", "minv", "assign", "slot")


class _RecordsOut(ctypes.Structure):
    _fields_ = [("hot_words", ctypes.c_uint32), ("cold_words", ctypes.c_uint32), ("c_hot", ctypes.c_void_p), ("c_cold", ctypes.c_void_p)] + [(f, ctypes.c_void_p) for f in RECORD_COLS]


def run_records(lib_path, R, poison=None):
    """ksolve_test_fast_records: one be_launch_fast_records (ksolve_fast_records, then ksolve_fast_scatter)"""
    lib = _lib(lib_path)
    if not hasattr(lib, "_records_ready"):
        lib.ksolve_test_fast_records.restype = ctypes.c_int
        lib.ksolve_test_fast_records.argtypes = [ctypes.POINTER(_RecordsIn), ctypes.POINTER(_RecordsOut)]
        lib._records_ready = True
    poison = R["poison"] if poison is None else poison
    sp, n_its, nr, nt, C, n_pods = R["space"], R["n_its"], R["n_res"], R["n_templates"], len(R["claims"]), len(R["sorted"])
    iw = (n_its + 63) // 64
    keep = []
    tmpl = _reqsets(ra.encode_sets(sp, R["templates"], junk=True), nt, keep)
    alloc, eff = np.array(R["alloc"], I64).reshape(nr, n_its), np.array(R["eff"], I64).reshape(nt, nr, n_its)
    off, vkey, voff, vwidth, vword, vmask = 0, [], [], [], [], [c["stage"] << 56 for c in R["claims"]]
    for key in R["var_keys"]:
        k, width = sp.kidx[key], len(sp.values[key])
        assert sp.off[k + 1] - sp.off[k] == 1
        vkey.append(k), voff.append(off), vwidth.append(width), vword.append(int(sp.off[k]))
        for c, claim in enumerate(R["claims"]):
            guard, values = claim["fields"][key]
            vmask[c] |= sum(1 << (off + sp.values[key].index(v)) for v in values) | (int(guard) << (off + width))
        off += width + 1
    assert off <= 56
    nv = len(vkey)
    vkey, voff, vwidth, vword = np.array(vkey + [0], U8), np.array(voff + [0], U8), np.array(vwidth + [0], U8), np.array(vword + [0], np.uint16)
    real = np.array(R["real"], U8) if R["real"] is not None else None
    c_vmask, c_req = np.array(vmask, U64), np.array([c["req"] for c in R["claims"]], I32).reshape(C, 4)
    c_ent, c_npods, c_hostseq = np.array([c["ent"] for c in R["claims"]], np.uint16), np.array([c["npods"] for c in R["claims"]], U32), np.array([c["hostseq"] for c in R["claims"]], U32)
    ent_its = np.array([_bits(iw, s | j) for s, j in zip(R["ent_its"], R["ent_junk"])], U64).reshape(-1, iw)
    sorted_, q_claim, q_cnt = np.array(R["sorted"], U32), np.array(R["q_claim"], U32), np.array(R["q_cnt"], U32)
    a = _RecordsIn(sp.nk, sp.off.ctypes.data, sp.value_int.ctypes.data, sp.value_is_int.ctypes.data, sp.value_valid.ctypes.data, n_its, nr, nt, ctypes.pointer(tmpl),
                   alloc.ctypes.data, eff.ctypes.data, R["tmpl_ov"], nv, vkey.ctypes.data, voff.ctypes.data, vwidth.ctypes.data, vword.ctypes.data,
                   real.ctypes.data if real is not None else None, C, len(ent_its), c_vmask.ctypes.data, c_req.ctypes.data, c_ent.ctypes.data, ent_its.ctypes.data,
                   c_npods.ctypes.data, c_hostseq.ctypes.data, n_pods, sorted_.ctypes.data, q_claim.ctypes.data, q_cnt.ctypes.data, poison)
    hw_max, cw_max = sp.rw + iw + 2 * nr + 4, 3 * sp.nk
    g = dict(c_hot=np.zeros(C * hw_max, U64), c_cold=np.zeros(C * cw_max, U64), mask=np.zeros((C, sp.rw), U64), its=np.zeros((C, iw), U64), total=np.zeros((C, nr), I64), head=np.zeros((C, nr), I64),
             gte=np.zeros((C, sp.nk), I64), lte=np.zeros((C, sp.nk), I64), minv=np.zeros((C, sp.nk), I32), assign=np.zeros(n_pods, I32), slot=np.zeros(n_pods, U32))
    for f in ("defined", "complement", "has_gte", "has_lte", "tmpl", "npods", "host_seq", "flags"):
        g[f] = np.zeros(C, U32)
    o = _RecordsOut(0, 0, g["c_hot"].ctypes.data, g["c_cold"].ctypes.data, *[g[f].ctypes.data for f in RECORD_COLS])
    st = lib.ksolve_test_fast_records(ctypes.byref(a), ctypes.byref(o))
    assert st == 0, f"ksolve_test_fast_records: status {st}"
    g["c_hot"], g["c_cold"] = g["c_hot"][:C * o.hot_words].reshape(C, o.hot_words), g["c_cold"][:C * o.cold_words].reshape(C, o.cold_words)
    g["poison"] = poison
    return g


def record_mismatches(got, want):
    """every column and claim (or pod) that differs from the definition; the cold record of a claim without bounds must be poison still"""
    bad = []
    for k in ("mask", "its", "total", "head", "defined", "complement", "has_gte", "has_lte", "tmpl", "npods", "host_seq", "flags", "assign", "slot"):
        g, w = np.asarray(got[k]), np.asarray(want[k])
        rows = np.nonzero((g != w).reshape(len(g), -1).any(axis=1))[0]
        bad += [(k, int(c)) for c in rows]
    for c, written in enumerate(want["cold_written"]):
        if written:
            bad += [(k, c) for k in ("gte", "lte", "minv") if not np.array_equal(got[k][c], want[k][c])]
        elif not (got["c_cold"][c] == U64(got["poison"])).all():
            bad.append(("cold written", c))
    return bad


RECORD_CASES = {
    "1-claim-63-types": dict(seed=1, n_claims=1, n_its=63, nv=1),
    "63-claims-64-types": dict(seed=2, n_claims=63, n_its=64, nv=3),
    "64-claims-65-types": dict(seed=3, n_claims=64, n_its=65, nv=3, extra_key=True),       # an even number of keys: minValues two to a word
    "65-claims-130-types": dict(seed=4, n_claims=65, n_its=130, nv=3),
    "no-variable-key": dict(seed=5, n_claims=20, n_its=65, nv=0),
    "twelve-variable-keys": dict(seed=6, n_claims=65, n_its=64, nv=12, wide=True),
    "no-limits": dict(seed=7, n_claims=65, n_its=130, nv=3, lim=False),
}


@functools.lru_cache(maxsize=None)
def records_case(name):
    return make_records(**RECORD_CASES[name])


def chain_problem(R, got):
    """the finalize problem whose claims are the records the hook returned: the definition's requirement sets and types as plain values,
    and the downloaded columns as they are for the finalize hook (junk in the cold columns where none was written)"""
    want = expected_records(R)
    P = dict(R["P"])
    P["space"], P["truncate_n"] = R["space"], 5
    it_reqs = P["it_reqs"]
    P["slots"] = [dict(reqs=want["rows"][c], its={i for i in range(R["n_its"]) if (int(want["its"][c][i >> 6]) >> (i & 63)) & 1}, template=int(want["tmpl"][c]), held=set(), minv_flag=False)
                  for c in range(len(R["claims"]))]
    P["claim_slots"] = list(range(len(P["slots"])))
    P["it_reqs"] = it_reqs
    cols = dict(mask=got["mask"], defined=got["defined"], complement=got["complement"], has_gte=got["has_gte"], has_lte=got["has_lte"], gte=got["gte"], lte=got["lte"], minv=None)
    P["raw_claims"] = dict(c_reqs=cols, c_its=got["its"], c_template=got["tmpl"])
    return P
