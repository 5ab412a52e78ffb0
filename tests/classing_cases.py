"""Pod classing (csrc/kernels.h row_hash / row_class / class_gather, csrc/ksolve.hip ksolve_row_hash_coop2 and its predecessors)
against its definition, restated here once in plain numpy — no project C++ is involved in the expected answers.

THE DEFINITION. Two pod rows are the same class iff they agree in
  * every request dimension below n_res;
  * both requirement sets (requirements and strict requirements; a shared strict table is the requirement table):
      - the four flag words (defined, complement, has_gte, has_lte);
      - for every DEFINED key: its mask words, gte / lte where the corresponding bit is set, and minValues (an absent
        table means -1 everywhere);
  * the toleration mask;
  * both host-port words, the volume word and every topology word (owned and selected) where the tables exist.
Mask words of undefined keys, bounds without their bit and minValues of undefined keys do not count. (The generator keeps
has_gte / has_lte inside `defined`, as the flattener does.)

The class tables are taken from the class's smallest row (copy_reqset / class_gather_body): all mask words verbatim, gte / lte
zero without their bit, minValues -1 without a table, the hot record `masks | requests | f0 | f1 | tolerates | meta` with meta
bit 0 set iff a defined key has minValues >= 0, the cold record `gte | lte | minv` (minv as packed int32).

A case is a dict of numpy tables (see make_case). run() drives the test-only entry point ksolve_test_classify of a test build of
the solver library (tests/emu/libksolve_emu.so on the host, tests/emu/libksolve_hooks.so on the GPU); check_full() and
check_forced() hold its answer against the definition."""
import ctypes
import os

import numpy as np

SEED = 0x6B73703176310A01          # the seed ksolve_create starts with
FULL = 0xFFFFFFFFFFFFFFFF
U64, I64, U32, I32 = np.uint64, np.int64, np.uint32, np.int32

# ------------------------------------------------------------------------------------------------ kernel variants
K_COOP2_MINV_SAME, K_COOP2_MINV, K_COOP2_SAME_4, K_COOP2_SAME_8, K_COOP2_4, K_COOP2_8, K_COOP1, K_PLAIN, K_HOST = range(1, 10)
KERNEL_NAMES = {1: "coop2<minv,same,8>", 2: "coop2<minv,-,8>", 3: "coop2<-,same,4>", 4: "coop2<-,same,8>", 5: "coop2<-,-,4>",
                6: "coop2<-,-,8>", 7: "coop1", 8: "plain", 9: "host loop"}
SWITCHES = ("KSOLVE_ROWHASH_KERNEL", "KSOLVE_TEST_NO_SHARED_STRICT", "KSOLVE_TEST_ROWS_PER_BLOCK", "KSOLVE_TEST_LDS_PAD")

# name -> kernel id expected (None: the coop2 instantiation that fits the case, at 60 rows per block), switches, and what the tables
# of its cases look like: minv (minValues tables), separate (a strict table of its own), n_res values
VARIANTS = {
    "coop2_minv_same": dict(kernel=K_COOP2_MINV_SAME, env={}, minv=True, separate=False, n_res=(1, 4, 5, 8)),
    "coop2_minv": dict(kernel=K_COOP2_MINV, env={}, minv=True, separate=True, n_res=(1, 4, 5, 8)),
    "coop2_same_4": dict(kernel=K_COOP2_SAME_4, env={}, minv=False, separate=False, n_res=(1, 4)),
    "coop2_same_8": dict(kernel=K_COOP2_SAME_8, env={}, minv=False, separate=False, n_res=(5, 8)),
    "coop2_4": dict(kernel=K_COOP2_4, env={}, minv=False, separate=True, n_res=(1, 4)),
    "coop2_8": dict(kernel=K_COOP2_8, env={}, minv=False, separate=True, n_res=(5, 8)),
    "coop2_rows60": dict(kernel=None, env={"KSOLVE_TEST_ROWS_PER_BLOCK": "60"}, minv=None, separate=None, n_res=(1, 4, 5, 8)),
    "coop1": dict(kernel=K_COOP1, env={"KSOLVE_ROWHASH_KERNEL": "coop1"}, minv=None, separate=None, n_res=(1, 4, 5, 8)),
    "plain_forced": dict(kernel=K_PLAIN, env={"KSOLVE_ROWHASH_KERNEL": "plain"}, minv=None, separate=None, n_res=(1, 4, 5, 8)),
    "plain_lds": dict(kernel=K_PLAIN, env={}, minv=None, separate=True, n_res=(1, 4, 5, 8)),   # reached on its own: the LDS need passes 64 KiB
}

N_ROWS = (165, 64, 65, 63, 2, 1)        # 165: two full blocks and a 37-row tail
POOLS = (17, 1, 0, 40, 3, 7, 2)
# (req_words, n_keys): every req_words and n_keys of the issue's table; a key needs a word, so the small dictionaries have one key
WORDS_KEYS = ((1, 1), (2, 1), (3, 1), (20, 5), (21, 16), (41, 17), (41, 32), (65, 5), (65, 17), (96, 32))
EXTRAS = ((0, 0, 0), (1, 1, 1), (1, 0, 3), (0, 1, 0), (0, 0, 3))   # host ports, volumes, topology words


def lds_coop2(rw, nk, minv, separate, rpb=64):
    t = 2 if separate else 1
    return t * rpb * (rw | 1) * 8 + (t * rpb * (nk | 1) * 4 if minv else 0)


def lds_coop1(rw, nk, n_res):
    return 2 * 64 * (rw | 1) * 8 + 2 * 64 * (nk | 1) * 4 + 8 + 64 * (n_res + 1) * 8


def accepts(variant, rw, nk, n_res, minv, separate):
    """Whether the launcher, with the variant's switches, runs the variant's kernel on such tables (the launcher's own
    conditions, restated to lay the cases out; the tests assert on the kernel the library REPORTS)."""
    v = VARIANTS[variant]
    if variant == "plain_forced":
        return True
    if variant == "coop1":
        return lds_coop1(rw, nk, n_res) <= 65536
    if variant == "plain_lds":
        return separate and lds_coop2(rw, nk, minv, True) > 65536 and lds_coop1(rw, nk, n_res) > 65536
    return lds_coop2(rw, nk, minv, separate, 60 if variant == "coop2_rows60" else 64) <= 65536 and n_res in v["n_res"]


def coop2_kernel(minv, separate, n_res):
    if minv:
        return K_COOP2_MINV if separate else K_COOP2_MINV_SAME
    if separate:
        return K_COOP2_4 if n_res <= 4 else K_COOP2_8
    return K_COOP2_SAME_4 if n_res <= 4 else K_COOP2_SAME_8


def shapes(variant):
    """The covering set of test A for one variant: every n_rows, every (req_words, n_keys) the variant accepts, every n_res it
    accepts and every optional table on and off; where the variant leaves them open, shared and separate strict tables, with and
    without minValues. pool: distinct row values the rows are drawn from (0: every row distinct, 1: all rows equal)."""
    v = VARIANTS[variant]
    out = []
    for rep in range(2):
        for j, (rw, nk) in enumerate(WORDS_KEYS):
            i = len(out)
            minv = v["minv"] if v["minv"] is not None else bool((j + rep) & 1)
            separate = v["separate"] if v["separate"] is not None else bool(((j >> 1) + rep) & 1)
            n_res = v["n_res"][i % len(v["n_res"])]
            if not accepts(variant, rw, nk, n_res, minv, separate):
                if v["separate"] is not None or not accepts(variant, rw, nk, n_res, minv, False):
                    continue
                separate = False
            hp, vol, tw = EXTRAS[i % len(EXTRAS)]
            out.append(dict(n_rows=N_ROWS[i % len(N_ROWS)], rw=rw, nk=nk, n_res=n_res, minv=minv, separate=separate, hp=hp, vol=vol, tw=tw,
                            pool=POOLS[i % len(POOLS)], seed=1000 + 37 * i + rw))
    return out


# ------------------------------------------------------------------------------------------------ tables
def key_offsets(rw, nk, rng):
    """key_word_off for nk keys over rw words; no key starts at word 20, 40, 60, 64 or 80 where that can be avoided, so key ranges
    cross the staging rounds, the batches of row_diff_far and the second word of word_defined_mask."""
    cand = [c for c in range(1, rw) if c not in (20, 40, 60, 64, 80)]
    if len(cand) < nk - 1:
        cand = list(range(1, rw))
    cuts = sorted(rng.choice(cand, size=nk - 1, replace=False).tolist()) if nk > 1 else []
    return np.array([0] + cuts + [rw], dtype=U32)


def _rand_u64(rng, shape):
    return rng.integers(0, 1 << 63, size=shape, dtype=U64) * U64(2) + rng.integers(0, 2, size=shape, dtype=U64)


def base_row(shape, rng):
    """One row value (every field of the definition), as a dict of 1-row tables."""
    rw, nk, nr = shape["rw"], shape["nk"], shape["n_res"]
    off = key_offsets(rw, nk, rng)

    def reqset():
        # every third key stays undefined (when there are several); bounds on two defined keys; minValues on every other defined key
        undefined = [k for k in range(nk) if nk > 1 and k % 3 == 1]
        defined = sum(1 << k for k in range(nk) if k not in undefined)
        dk = [k for k in range(nk) if (defined >> k) & 1]
        s = dict(mask=_rand_u64(rng, (1, rw)), defined=np.array([defined], U32), complement=np.array([defined & int(rng.integers(0, 1 << 32))], U32),
                 has_gte=np.array([1 << dk[0]], U32), has_lte=np.array([1 << dk[-1]], U32),
                 gte=rng.integers(-1000, 1000, size=(1, nk), dtype=I64), lte=rng.integers(-1000, 1000, size=(1, nk), dtype=I64), minv=None)
        if shape["minv"]:
            s["minv"] = np.where(np.arange(nk) % 2 == 0, rng.integers(0, 50, size=(1, nk)), -1).astype(I32)
        return s
    row = dict(key_word_off=off, n_res=nr, requests=rng.integers(1, 1 << 40, size=(nr, 1), dtype=I64), reqs=reqset(),
               strict=reqset() if shape["separate"] else None, tolerates=_rand_u64(rng, (1,)),
               host_ports=_rand_u64(rng, (1, 2)) if shape["hp"] else None, vol=_rand_u64(rng, (1,)) if shape["vol"] else None,
               topo_owned=_rand_u64(rng, (1, shape["tw"])) if shape["tw"] else None, topo_selected=_rand_u64(rng, (1, shape["tw"])) if shape["tw"] else None)
    return row


def take(tab, idx):
    """The case whose row i is row idx[i] of `tab` (copies)."""
    idx = np.asarray(idx)

    def rs(s):
        return None if s is None else {k: (None if v is None else v[idx].copy()) for k, v in s.items()}
    return dict(key_word_off=tab["key_word_off"], n_res=tab["n_res"], requests=tab["requests"][:, idx].copy(), reqs=rs(tab["reqs"]), strict=rs(tab["strict"]),
                tolerates=tab["tolerates"][idx].copy(), **{k: (None if tab[k] is None else tab[k][idx].copy()) for k in ("host_ports", "vol", "topo_owned", "topo_selected")})


def n_rows_of(case):
    return case["tolerates"].shape[0]


def _sets(case):
    return [("reqs", case["reqs"])] + ([("strict", case["strict"])] if case["strict"] is not None else [])


def _words_of_key(off, k):
    return range(int(off[k]), int(off[k + 1]))


def differences(case):
    """Single-field differences for a row of `case`: (name, counted, apply) with apply(case, row) changing exactly one place.
    counted: the definition tells the rows apart; not counted: it ignores the place."""
    off = case["key_word_off"]
    nk, rw = len(off) - 1, int(off[-1])
    out = []

    def add(name, counted, fn):
        out.append((name, counted, fn))
    for r in range(case["n_res"]):
        add(f"request[{r}]", True, lambda c, row, r=r: c["requests"].__setitem__((r, row), c["requests"][r, row] + 1))
    for sname, s in _sets(case):
        defined = int(s["defined"][0])
        dk = [k for k in range(nk) if (defined >> k) & 1]
        uk = [k for k in range(nk) if not (defined >> k) & 1]
        widest = max(dk, key=lambda k: int(off[k + 1]) - int(off[k]))
        words = {int(off[dk[0]]), (int(off[widest]) + int(off[widest + 1]) - 1) // 2, int(off[dk[-1] + 1]) - 1}
        key_of = {w: k for k in range(nk) for w in _words_of_key(off, k)}
        words |= {w for w in (19, 20, 21, 39, 40, 41, 63, 64, 65, rw - 1) if w < rw and key_of[w] in dk}
        for w in sorted(words):
            add(f"{sname}.mask[{w}]", True, lambda c, row, s=sname, w=w: c[s]["mask"].__setitem__((row, w), c[s]["mask"][row, w] ^ U64(1 << (w % 64))))
        kf = uk[0] if uk else dk[-1]
        add(f"{sname}.defined", True, lambda c, row, s=sname, k=kf: c[s]["defined"].__setitem__(row, c[s]["defined"][row] ^ U32(1 << k)))
        add(f"{sname}.complement", True, lambda c, row, s=sname, k=dk[0]: c[s]["complement"].__setitem__(row, c[s]["complement"][row] ^ U32(1 << k)))
        kb = dk[len(dk) // 2]   # (a key whose bound bit the flip sets or clears; the bound VALUES stay as they are)
        add(f"{sname}.has_gte", True, lambda c, row, s=sname, k=kb: c[s]["has_gte"].__setitem__(row, c[s]["has_gte"][row] ^ U32(1 << k)))
        add(f"{sname}.has_lte", True, lambda c, row, s=sname, k=kb: c[s]["has_lte"].__setitem__(row, c[s]["has_lte"][row] ^ U32(1 << k)))
        kg = int(s["has_gte"][0]).bit_length() - 1
        kl = int(s["has_lte"][0]).bit_length() - 1
        add(f"{sname}.gte[{kg}]", True, lambda c, row, s=sname, k=kg: c[s]["gte"].__setitem__((row, k), c[s]["gte"][row, k] + 1))
        add(f"{sname}.lte[{kl}]", True, lambda c, row, s=sname, k=kl: c[s]["lte"].__setitem__((row, k), c[s]["lte"][row, k] - 1))
        nb = [k for k in range(nk) if k != kg and k != kl and k != kb]
        if nb:
            add(f"{sname}.gte[{nb[0]}] without its bit", False, lambda c, row, s=sname, k=nb[0]: c[s]["gte"].__setitem__((row, k), c[s]["gte"][row, k] + 1))
            add(f"{sname}.lte[{nb[-1]}] without its bit", False, lambda c, row, s=sname, k=nb[-1]: c[s]["lte"].__setitem__((row, k), c[s]["lte"][row, k] + 1))
        if s["minv"] is not None:
            for k in sorted({dk[0], dk[-1]}):   # (dk[-1] >= 16 where there are more than kRowFarKeys keys)
                add(f"{sname}.minv[{k}]", True, lambda c, row, s=sname, k=k: c[s]["minv"].__setitem__((row, k), c[s]["minv"][row, k] + 1))
            if uk:
                add(f"{sname}.minv[{uk[-1]}] of an undefined key", False, lambda c, row, s=sname, k=uk[-1]: c[s]["minv"].__setitem__((row, k), c[s]["minv"][row, k] + 1))
        if uk:
            w = int(off[uk[-1]])
            add(f"{sname}.mask[{w}] of an undefined key", False, lambda c, row, s=sname, w=w: c[s]["mask"].__setitem__((row, w), c[s]["mask"][row, w] ^ U64(2)))
    add("tolerates", True, lambda c, row: c["tolerates"].__setitem__(row, c["tolerates"][row] ^ U64(1 << 33)))
    if case["host_ports"] is not None:
        for i in (0, 1):
            add(f"host_ports[{i}]", True, lambda c, row, i=i: c["host_ports"].__setitem__((row, i), c["host_ports"][row, i] ^ U64(4)))
    if case["vol"] is not None:
        add("vol", True, lambda c, row: c["vol"].__setitem__(row, c["vol"][row] ^ U64(1 << 32)))
    if case["topo_owned"] is not None:
        tw = case["topo_owned"].shape[1]
        for t in ("topo_owned", "topo_selected"):
            for w in sorted({0, tw - 1}):
                add(f"{t}[{w}]", True, lambda c, row, t=t, w=w: c[t].__setitem__((row, w), c[t][row, w] ^ U64(1 << 17)))
    return out


def make_case(shape):
    """Test A's rows: shape['n_rows'] rows drawn from a pool of shape['pool'] row values (0: every row distinct), each pool value
    the base row with one to three counted single-field differences applied, so that classes differ in few places; then, row by row,
    noise in every place the definition ignores."""
    rng = np.random.default_rng(shape["seed"])
    n = shape["n_rows"]
    b = base_row(shape, rng)
    pool_n = shape["pool"] or n
    pool = take(b, np.zeros(pool_n, dtype=np.int64))
    # (with one key, a row that loses `defined` would keep that key's bound bits: the flattener never writes such a row)
    counted = [d for d in differences(b) if d[1] and not (d[0].endswith(".defined") and shape["nk"] == 1)]
    for p in range(1, pool_n):
        for j in rng.choice(len(counted), size=int(rng.integers(1, 4)), replace=False):
            counted[j][2](pool, p)
    idx = rng.integers(0, pool_n, size=n) if shape["pool"] else rng.permutation(n)
    case = take(pool, idx)
    if not shape["pool"]:
        case["requests"][0, :] = np.arange(n, dtype=I64) * 3 + 1 + (case["requests"][0, :] & I64(0))   # distinct whatever the pool drew
    off = case["key_word_off"]
    nk = len(off) - 1
    for _, s in _sets(case):
        d = _bits(s["defined"], nk)
        s["mask"] = np.where(d[:, _key_of_word(off)], s["mask"], _rand_u64(rng, s["mask"].shape))
        if s["minv"] is not None:
            s["minv"] = np.where(d, s["minv"], rng.integers(-1, 9, size=d.shape)).astype(I32)
        s["gte"] = np.where(_bits(s["has_gte"], nk), s["gte"], rng.integers(-99, 99, size=d.shape)).astype(I64)
        s["lte"] = np.where(_bits(s["has_lte"], nk), s["lte"], rng.integers(-99, 99, size=d.shape)).astype(I64)
    return case


B_PLACES = ((165, 0), (165, 5), (165, 64), (165, 128), (165, 135), (2, 1))   # (n_rows, the row that holds the variant V)


def b_shape(variant):
    """Test B's tables for one variant: the largest dictionary the variant accepts (mask words 20 and up, 64 and up where it can),
    every optional table on, as many request dimensions as the variant has."""
    v = VARIANTS[variant]
    minv = v["minv"] if v["minv"] is not None else True
    separate = v["separate"] if v["separate"] is not None else True
    n_res = v["n_res"][-1]
    rw, nk = [p for p in WORDS_KEYS if accepts(variant, p[0], p[1], n_res, minv, separate)][-1]
    return dict(rw=rw, nk=nk, n_res=n_res, minv=minv, separate=separate, hp=1, vol=1, tw=3, seed=77)


def b_cases(shape):
    """Yields (name, counted, n_rows, v_row, case) — all rows the base row B, row v_row the variant V."""
    rng = np.random.default_rng(shape["seed"])
    b = base_row(shape, rng)
    for name, counted, fn in differences(b):
        for n, at in B_PLACES:
            case = take(b, np.zeros(n, dtype=np.int64))
            fn(case, at)
            yield name, counted, n, at, case


# ------------------------------------------------------------------------------------------------ the definition
def _minv_eff(s, n, nk):
    return s["minv"].astype(I64) if s["minv"] is not None else np.full((n, nk), -1, dtype=I64)


def _key_of_word(off):
    return np.repeat(np.arange(len(off) - 1), np.diff(off.astype(np.int64)))


def _bits(flags, nk):
    return ((flags.astype(np.int64)[:, None] >> np.arange(nk)[None, :]) & 1).astype(bool)


def canonical_rows(case):
    """[n_rows][*] uint64: the places that count, the places that do not zeroed. Two rows are one class iff their lines are equal."""
    off = case["key_word_off"]
    nk, n = len(off) - 1, n_rows_of(case)
    cols = [case["requests"].T.view(U64)]
    for _, s in [("reqs", case["reqs"]), ("strict", case["strict"] if case["strict"] is not None else case["reqs"])]:
        d = _bits(s["defined"], nk)
        cols += [np.stack([s["defined"], s["complement"], s["has_gte"], s["has_lte"]], axis=1).astype(U64)]
        cols += [np.where(d[:, _key_of_word(off)], s["mask"], U64(0))]
        cols += [np.where(d & _bits(s["has_gte"], nk), s["gte"], 0).view(U64), np.where(d & _bits(s["has_lte"], nk), s["lte"], 0).view(U64)]
        cols += [np.where(d, _minv_eff(s, n, nk), 0).view(U64)]
    cols += [case["tolerates"][:, None]]
    for k in ("host_ports", "vol", "topo_owned", "topo_selected"):
        if case[k] is not None:
            cols += [case[k].reshape(n, -1)]
    return np.ascontiguousarray(np.concatenate(cols, axis=1))


def partition(case):
    """rep[r] = the smallest row of r's class."""
    first = {}
    canon = canonical_rows(case)
    return np.array([first.setdefault(canon[r].tobytes(), r) for r in range(canon.shape[0])], dtype=np.int64)


def class_tables(case, reps):
    """What class_gather leaves for classes whose representatives are rows `reps` (in that order)."""
    off = case["key_word_off"]
    nk, rw, nr, n = len(off) - 1, int(off[-1]), case["n_res"], n_rows_of(case)
    reps = np.asarray(reps, dtype=np.int64)
    t = dict(cls_requests=case["requests"][:, reps].T.copy(), cls_tolerates=case["tolerates"][reps])
    for name in ("reqs", "strict"):
        s = case[name] if case[name] is not None else case["reqs"]
        t[name + "_mask"] = s["mask"][reps]
        t[name + "_flags"] = np.stack([s["defined"][reps], s["complement"][reps], s["has_gte"][reps], s["has_lte"][reps]])
        t[name + "_gte"] = np.where(_bits(s["has_gte"][reps], nk), s["gte"][reps], 0)
        t[name + "_lte"] = np.where(_bits(s["has_lte"][reps], nk), s["lte"][reps], 0)
        t[name + "_minv"] = _minv_eff(s, n, nk)[reps].astype(I32)
    if case["host_ports"] is not None:
        t["cls_host_ports"] = case["host_ports"][reps]
    if case["vol"] is not None:
        t["cls_vol"] = case["vol"][reps]
    if case["topo_owned"] is not None:
        t["cls_topo"] = np.concatenate([case["topo_owned"][reps], case["topo_selected"][reps]], axis=1)
    q = case["reqs"]
    f0 = q["defined"][reps].astype(U64) | (q["complement"][reps].astype(U64) << U64(32))
    f1 = q["has_gte"][reps].astype(U64) | (q["has_lte"][reps].astype(U64) << U64(32))
    meta = (_bits(q["defined"][reps], nk) & (t["reqs_minv"] >= 0)).any(axis=1).astype(U64)
    t["cls_hot"] = np.concatenate([q["mask"][reps], t["cls_requests"].view(U64), f0[:, None], f1[:, None], t["cls_tolerates"][:, None], meta[:, None]], axis=1)
    mv = np.zeros((len(reps), 2 * ((nk + 1) // 2)), dtype=I32)
    mv[:, :nk] = t["reqs_minv"]
    t["cls_cold"] = np.concatenate([t["reqs_gte"].view(U64), t["reqs_lte"].view(U64), np.ascontiguousarray(mv).view(U64)], axis=1)
    t["lay"] = np.array([0, rw, rw + nr, rw + nr + 1, rw + nr + 2, rw + nr + 3, rw + nr + 4, 2 * nk + (nk + 1) // 2], dtype=I32)
    t["min_request"] = case["requests"].min(axis=1)
    return t


# ------------------------------------------------------------------------------------------------ the library
class _ReqSets(ctypes.Structure):
    _fields_ = [("n", ctypes.c_uint32)] + [(f, ctypes.c_void_p) for f in ("mask", "defined", "complement", "has_gte", "has_lte", "gte", "lte", "min_values")]


class _In(ctypes.Structure):
    _fields_ = [("n_keys", ctypes.c_uint32), ("key_word_off", ctypes.c_void_p), ("n_rows", ctypes.c_uint32), ("n_res", ctypes.c_uint32),
                ("requests", ctypes.c_void_p), ("reqs", ctypes.POINTER(_ReqSets)), ("strict", ctypes.POINTER(_ReqSets)), ("tolerates", ctypes.c_void_p),
                ("host_ports", ctypes.c_void_p), ("vol", ctypes.c_void_p), ("topo_owned", ctypes.c_void_p), ("topo_selected", ctypes.c_void_p),
                ("topo_words", ctypes.c_uint32), ("hash_keep", ctypes.c_uint64), ("seed", ctypes.c_uint64)]


_OUT_TABLES = ("row_class", "class_rep", "min_request", "cls_requests", "cls_tolerates", "reqs_mask", "strict_mask", "reqs_flags", "strict_flags",
               "reqs_gte", "reqs_lte", "strict_gte", "strict_lte", "reqs_minv", "strict_minv", "cls_host_ports", "cls_vol", "cls_topo", "cls_hot", "cls_cold")


class _Out(ctypes.Structure):
    _fields_ = [(f, ctypes.c_uint32) for f in ("n_classes", "collision", "kernel", "rows_per_block")] + [(f, ctypes.c_void_p) for f in _OUT_TABLES] + [("lay", ctypes.c_int32 * 8)]


_libs = {}


def _lib(path):
    if path not in _libs:
        lib = ctypes.CDLL(os.path.abspath(path))
        lib.ksolve_test_classify.restype = ctypes.c_int
        lib.ksolve_test_classify.argtypes = [ctypes.POINTER(_In), ctypes.POINTER(_Out)]
        _libs[path] = lib
    return _libs[path]


def run(lib_path, case, hash_keep=FULL, seed=SEED):
    """ksolve_test_classify on `case`: dict with n_classes, collision, kernel, rows_per_block, lay and every downloaded table cut to n_classes."""
    off = np.ascontiguousarray(case["key_word_off"], dtype=U32)
    nk, rw, nr, n = len(off) - 1, int(off[-1]), case["n_res"], n_rows_of(case)
    keep = []

    def ptr(a, dtype):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=dtype)
        keep.append(a)
        return a.ctypes.data

    def reqsets(s):
        r = _ReqSets(n, ptr(s["mask"], U64), ptr(s["defined"], U32), ptr(s["complement"], U32), ptr(s["has_gte"], U32), ptr(s["has_lte"], U32),
                     ptr(s["gte"], I64), ptr(s["lte"], I64), ptr(s["minv"], I32))
        keep.append(r)
        return ctypes.pointer(r)
    tw = case["topo_owned"].shape[1] if case["topo_owned"] is not None else 0
    arg = _In(nk, off.ctypes.data, n, nr, ptr(case["requests"], I64), reqsets(case["reqs"]), reqsets(case["strict"]) if case["strict"] is not None else None,
              ptr(case["tolerates"], U64), ptr(case["host_ports"], U64), ptr(case["vol"], U64), ptr(case["topo_owned"], U64), ptr(case["topo_selected"], U64),
              tw, hash_keep, seed)
    hot, cold = rw + nr + 4, 2 * nk + (nk + 1) // 2
    bufs = dict(row_class=np.full(n, 0xFFFFFFFF, U32), class_rep=np.full(n, 0xFFFFFFFF, U32), min_request=np.zeros(nr, I64), cls_requests=np.zeros((n, nr), I64),
                cls_tolerates=np.zeros(n, U64), reqs_mask=np.zeros((n, rw), U64), strict_mask=np.zeros((n, rw), U64), reqs_flags=np.zeros(4 * n, U32),
                strict_flags=np.zeros(4 * n, U32), reqs_gte=np.zeros((n, nk), I64), reqs_lte=np.zeros((n, nk), I64), strict_gte=np.zeros((n, nk), I64),
                strict_lte=np.zeros((n, nk), I64), reqs_minv=np.zeros((n, nk), I32), strict_minv=np.zeros((n, nk), I32), cls_host_ports=np.zeros((n, 2), U64),
                cls_vol=np.zeros(n, U64), cls_topo=np.zeros((n, 2 * max(tw, 1)), U64), cls_hot=np.zeros(n * hot, U64), cls_cold=np.zeros(n * cold, U64))
    out = _Out()
    for f in _OUT_TABLES:
        setattr(out, f, bufs[f].ctypes.data)
    st = _lib(lib_path).ksolve_test_classify(ctypes.byref(arg), ctypes.byref(out))
    assert st == 0, f"ksolve_test_classify: status {st}"
    nc = int(out.n_classes)
    assert 1 <= nc <= n
    res = dict(n_classes=nc, collision=int(out.collision), kernel=int(out.kernel), rows_per_block=int(out.rows_per_block), lay=np.array(list(out.lay), dtype=I32),
               row_class=bufs["row_class"], min_request=bufs["min_request"])
    for f in _OUT_TABLES[1:]:
        if f in ("min_request",):
            continue
        a = bufs[f]
        if f.endswith("_flags"):
            a = a[:4 * nc].reshape(4, nc)
        elif f == "cls_hot":
            a = a[:nc * hot].reshape(nc, hot)
        elif f == "cls_cold":
            a = a[:nc * cold].reshape(nc, cold)
        elif f == "cls_topo":
            a = a.reshape(-1)[:nc * 2 * tw].reshape(nc, 2 * tw)
        else:
            a = a[:nc]
        res[f] = a
    return res


# ------------------------------------------------------------------------------------------------ the checks
def check_full(case, got, what=""):
    """The answer at full hash: no collision, the definition's partition and representatives, every gathered table bit for bit."""
    want_rep = partition(case)
    n = n_rows_of(case)
    assert got["collision"] == 0, (what, "collision", got["collision"])
    assert got["n_classes"] == len(set(want_rep.tolist())), (what, "n_classes", got["n_classes"], len(set(want_rep.tolist())))
    rc = got["row_class"].astype(np.int64)
    assert sorted(set(rc.tolist())) == list(range(got["n_classes"])), (what, "class ids are not a permutation of range(n_classes)")
    got_rep = got["class_rep"].astype(np.int64)[rc]
    bad = np.nonzero(got_rep != want_rep)[0]
    assert bad.size == 0, (what, "rows with another representative than the definition's", bad[:8].tolist(), got_rep[bad[:8]].tolist(), want_rep[bad[:8]].tolist())
    want = class_tables(case, got["class_rep"])
    for name, w in want.items():
        if name not in got:
            continue
        g = got[name]
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        assert np.array_equal(g, w), (what, name, "first differences at", np.argwhere(g != w)[:6].tolist())
    for name in ("cls_host_ports", "cls_vol", "cls_topo"):
        assert (name in want) == (case[{"cls_host_ports": "host_ports", "cls_vol": "vol", "cls_topo": "topo_owned"}[name]] is not None)
    return n


def check_forced(case, got, counted, what=""):
    """The answer with every hash forced equal (hash_keep = 0): one slot, and the collision word tells whether it holds two distinct rows."""
    assert got["n_classes"] == 1, (what, got["n_classes"])
    assert got["collision"] == (1 if counted else 0), (what, "collision", got["collision"], "expected", 1 if counted else 0)
