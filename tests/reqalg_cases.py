"""The requirement algebra (csrc/reqalg.h) and the instance-type index (csrc/kernels.h it_index_body) against their definition,
restated here once on Python sets of strings and Python ints — no bitmasks, nothing shared with the oracle or the product.

THE DEFINITION is the reference's pkg/scheduling/requirement.go and requirements.go, function by function (cited at each one
below). A requirement is (key, set of strings, complement, gte, lte, minValues); a requirement set is a dict key -> requirement.

THE FLAT FORM is what the product computes on (include/ksolve.h ksolve_reqsets): every key has a dictionary of values, a value is
one bit of the key's mask words, the flag words carry one bit per key. Space is the dictionary (order, word offsets, value_int,
value_is_int, value_valid), encode_sets() / decode_sets() go between the two forms.

run_reqalg() and run_it_index() drive the test-only entry points ksolve_test_reqalg and ksolve_test_it_index of a test build of the
solver library (tests/emu/libksolve_emu.so on the host, tests/emu/libksolve_hooks.so on the GPU); expected_reqalg() and
expected_it_index() are the same answers from the definition; mismatches() lists every word that differs. Nothing is compared
with a tolerance, and no output field is left out: the fields of a built requirement set that belong to keys it does not define
are fixed by reqbuf_load (mask words as the input has them, bounds 0, minValues as the input has them, -1 without a column), and
the expected tables say so."""
import ctypes
import functools
import json
import os
import random
import re

import numpy as np

U64, I64, U32, I32, U8 = np.uint64, np.int64, np.uint32, np.int32, np.uint8
INT_MAX, INT_MIN = 2**63 - 1, -2**63        # Go's int on the platforms the reference runs on
OP_IN, OP_NOTIN, OP_EXISTS, OP_DNE = 0, 1, 2, 3     # reqalg.h's numbering of Operator()
OP_NAMES = {"In": OP_IN, "NotIn": OP_NOTIN, "Exists": OP_EXISTS, "DoesNotExist": OP_DNE}
COMPAT_OK, COMPAT_UNDEFINED_KEY, COMPAT_NO_INTERSECTION = 0, 1, 2


# ------------------------------------------------------------------------------------------------ the definition
@functools.lru_cache(maxsize=None)
def go_atoi(s):
    """strconv.Atoi as withinBounds uses it (requirement.go:339-342): an optional sign and decimal digits that fit an int;
    None for everything else (a syntax or a range error)."""
    if not re.fullmatch(r"[+-]?[0-9]+", s):
        return None
    v = int(s)
    return v if INT_MIN <= v <= INT_MAX else None


def _wrap(v):
    """Go's int arithmetic wraps (value-- on math.MinInt, requirement.go:98)."""
    return (v - INT_MIN) % 2**64 + INT_MIN


class Req:
    """Requirement — requirement.go:35-43."""
    __slots__ = ("key", "values", "complement", "gte", "lte", "min_values")

    def __init__(self, key, values, complement, gte=None, lte=None, min_values=None):
        self.key, self.values, self.complement, self.gte, self.lte, self.min_values = key, frozenset(values), bool(complement), gte, lte, min_values

    def struct(self):
        return (self.key, self.values, self.complement, self.gte, self.lte, self.min_values)

    def __eq__(self, other):
        return isinstance(other, Req) and self.struct() == other.struct()

    def __hash__(self):
        return hash(self.struct())

    def __repr__(self):
        return f"Req({self.key!r}, {'not ' if self.complement else ''}{sorted(self.values)}, gte={self.gte}, lte={self.lte}, minValues={self.min_values})"


def new_requirement(key, operator, min_values, *values):
    """NewRequirementWithFlexibility — requirement.go:48-110 (without the label normalisation of lines 49-59: keys here are
    already normalised)."""
    if operator == "In":                                                    # :62-73
        return Req(key, values, False, min_values=min_values)
    complement = operator not in ("In", "DoesNotExist")                     # :75-83
    vals = values if operator in ("In", "NotIn") else ()                    # :84-86
    gte = lte = None
    if operator == "Gt":                                                    # :87-95
        v = go_atoi(values[0])
        if v == INT_MAX:
            return new_requirement(key, "DoesNotExist", None)               # :91 NewRequirement: minValues is dropped
        gte = v + 1
    if operator == "Lt":                                                    # :96-100
        lte = _wrap(go_atoi(values[0]) - 1)
    if operator == "Gte":                                                   # :101-104
        gte = go_atoi(values[0])
    if operator == "Lte":                                                   # :105-108
        lte = go_atoi(values[0])
    return Req(key, vals, complement, gte, lte, min_values)


def _max_ptr(a, b):
    """maxIntPtr — requirement.go:365-376"""
    return b if a is None else a if b is None else max(a, b)


def _min_ptr(a, b):
    """minIntPtr — requirement.go:352-363"""
    return b if a is None else a if b is None else min(a, b)


def within_bounds(value, gte, lte):
    """withinBounds — requirement.go:334-350"""
    if gte is None and lte is None:
        return True
    v = go_atoi(value)
    if v is None:
        return False
    return not (gte is not None and v < gte) and not (lte is not None and v > lte)


def intersection(r, q):
    """Requirement.Intersection — requirement.go:181-214"""
    complement = r.complement and q.complement
    gte, lte = _max_ptr(r.gte, q.gte), _min_ptr(r.lte, q.lte)
    min_values = _max_ptr(r.min_values, q.min_values)
    if gte is not None and lte is not None and gte > lte:
        return new_requirement(r.key, "DoesNotExist", min_values)
    if r.complement and q.complement:
        values = r.values | q.values
    elif r.complement:
        values = q.values - r.values
    elif q.complement:
        values = r.values - q.values
    else:
        values = r.values & q.values
    values = {v for v in values if within_bounds(v, gte, lte)}
    if not complement:
        gte = lte = None
    return Req(r.key, values, complement, gte, lte, min_values)


def has_intersection(r, q):
    """Requirement.HasIntersection — requirement.go:220-254"""
    gte, lte = _max_ptr(r.gte, q.gte), _min_ptr(r.lte, q.lte)
    if gte is not None and lte is not None and gte > lte:
        return False
    if r.complement and q.complement:
        return True
    if r.complement:
        return any(v not in r.values and within_bounds(v, gte, lte) for v in q.values)
    if q.complement:
        return any(v not in q.values and within_bounds(v, gte, lte) for v in r.values)
    return any(v in q.values and within_bounds(v, gte, lte) for v in r.values)


def has(r, value):
    """Requirement.Has — requirement.go:275-280"""
    if r.complement:
        return value not in r.values and within_bounds(value, r.gte, r.lte)
    return value in r.values and within_bounds(value, r.gte, r.lte)


def length(r):
    """Requirement.Len — requirement.go:303-308"""
    return INT_MAX - len(r.values) if r.complement else len(r.values)


def operator(r):
    """Requirement.Operator — requirement.go:290-301"""
    if r.complement:
        return "NotIn" if length(r) < INT_MAX else "Exists"
    return "In" if length(r) > 0 else "DoesNotExist"


def negative(r):
    return operator(r) in ("NotIn", "DoesNotExist")


def add(reqs, *incoming):
    """Requirements.Add — requirements.go:133-140 (mutates reqs)"""
    for q in incoming:
        if q.key in reqs:
            q = intersection(q, reqs[q.key])
        reqs[q.key] = q


def bad_keys(r, q):
    """Requirements.Intersects — requirements.go:254-274: the keys it reports (none = nil error). r existing, q incoming."""
    bad = []
    for key in r:
        if key not in q:
            continue
        existing, incoming = r[key], q[key]
        if not has_intersection(existing, incoming):
            if negative(incoming) and negative(existing):                    # :260-265
                continue
            bad.append(key)
    return bad


def compatible(r, q, allow_undefined=frozenset()):
    """Requirements.Compatible — requirements.go:181-197, as the outcome: 0 nil, 1 the error of line 193 (a key of q that r does
    not define), 2 the error of Intersects."""
    for key in q:
        if key in allow_undefined:
            continue
        if key in r or negative(q[key]):
            continue
        return COMPAT_UNDEFINED_KEY
    return COMPAT_NO_INTERSECTION if bad_keys(r, q) else COMPAT_OK


def from_selector(d):
    """A NodeSelectorRequirement as the golden tables write it."""
    return new_requirement(d["key"], d["operator"], d.get("minValues"), *d["values"])


# ------------------------------------------------------------------------------------------------ encoder and decoder
class Space:
    """The dictionary: keys in order, each with its values in order. Key k takes ceil(len(values) / 64) mask words from
    off[k]; value j of the key is bit j of those words. value_valid marks the bits that are values. The bits past a key's last
    value are set in value_is_int (with value_int 0) and clear in value_valid: only value_valid may keep them out of an answer."""

    def __init__(self, keys, well_known=(), key_it=None):
        self.keys = [k for k, _ in keys]
        self.values = {k: list(v) for k, v in keys}
        assert len(set(self.keys)) == len(self.keys) and all(len(set(v)) == len(v) >= 1 for v in self.values.values())
        self.kidx = {k: i for i, k in enumerate(self.keys)}
        self.nk = len(self.keys)
        off = [0]
        for k in self.keys:
            off.append(off[-1] + (len(self.values[k]) + 63) // 64)
        self.off = np.array(off, U32)
        self.rw = off[-1]
        self.bitpos = {k: {v: off[i] * 64 + j for j, v in enumerate(self.values[k])} for i, k in enumerate(self.keys)}
        self.well_known = frozenset(well_known)
        self.well_known_mask = sum(1 << self.kidx[k] for k in self.well_known)
        self.key_it = -1 if key_it is None else self.kidx[key_it]
        self.value_int = np.zeros(self.rw * 64, I64)
        is_int, valid = (1 << (self.rw * 64)) - 1, 0
        for k in self.keys:
            for v, p in self.bitpos[k].items():
                valid |= 1 << p
                iv = go_atoi(v)
                if iv is None:
                    is_int &= ~(1 << p)
                else:
                    self.value_int[p] = iv
        self.value_is_int, self.value_valid = self.words(is_int), self.words(valid)

    def words(self, bits):
        """a Python int of rw * 64 bits as the rw mask words"""
        return np.frombuffer(bits.to_bytes(self.rw * 8, "little"), U64).copy()

    def bits_of(self, key, values):
        pos = self.bitpos[key]
        b = 0
        for v in values:
            b |= 1 << pos[v]
        return b

    def has_bits(self, r):
        """the dictionary values of r's key that r Has(), as bits"""
        return self.bits_of(r.key, [v for v in self.values[r.key] if has(r, v)])


JUNK = 0x5A5AA5A55A5AA5A5       # what an input table holds in a gte / lte slot whose has_gte / has_lte bit is clear


def encode_sets(space, rows, null_cols=False, junk=False):
    """rows: requirement sets (dict key -> Req) -> the tables of a ksolve_reqsets. null_cols: no gte / lte / min_values columns
    (the rows must not need them). junk: bound slots without their flag bit hold JUNK instead of 0."""
    n, nk, rw = len(rows), space.nk, space.rw
    t = dict(mask=np.zeros((n, rw), U64), defined=np.zeros(n, U32), complement=np.zeros(n, U32), has_gte=np.zeros(n, U32), has_lte=np.zeros(n, U32),
             gte=np.full((n, nk), JUNK if junk else 0, I64), lte=np.full((n, nk), JUNK if junk else 0, I64), minv=np.full((n, nk), -1, I32))
    for i, row in enumerate(rows):
        bits = 0
        for key, r in row.items():
            assert r.key == key
            k = space.kidx[key]
            bits |= space.bits_of(key, r.values)
            t["defined"][i] |= U32(1 << k)
            if r.complement:
                t["complement"][i] |= U32(1 << k)
            if r.gte is not None:
                t["has_gte"][i] |= U32(1 << k)
                t["gte"][i, k] = r.gte
            if r.lte is not None:
                t["has_lte"][i] |= U32(1 << k)
                t["lte"][i, k] = r.lte
            if r.min_values is not None:
                t["minv"][i, k] = r.min_values
        t["mask"][i] = space.words(bits)
    if null_cols:
        assert not t["has_gte"].any() and not t["has_lte"].any() and (t["minv"] == -1).all()
        t["gte"] = t["lte"] = t["minv"] = None
    return t


def decode_sets(space, t, i):
    """row i of flat tables (the fields of encode_sets; `minv` may be None) -> dict key -> Req"""
    out = {}
    bits = int.from_bytes(np.ascontiguousarray(t["mask"][i]).tobytes(), "little")
    for k, key in enumerate(space.keys):
        if not (int(t["defined"][i]) >> k) & 1:
            continue
        vals = [v for v, p in space.bitpos[key].items() if (bits >> p) & 1]
        gte = int(t["gte"][i, k]) if (int(t["has_gte"][i]) >> k) & 1 else None
        lte = int(t["lte"][i, k]) if (int(t["has_lte"][i]) >> k) & 1 else None
        mv = int(t["minv"][i, k]) if t.get("minv") is not None and t["minv"][i, k] >= 0 else None
        out[key] = Req(key, vals, (int(t["complement"][i]) >> k) & 1, gte, lte, mv)
    return out


# ------------------------------------------------------------------------------------------------ expected answers
REQALG_FIELDS = ("has_intersection", "intersects", "compatible", "op", "values_word", "has_word", "buf_mask", "buf_flags", "buf_gte", "buf_lte", "buf_minv")


def expected_reqalg(space, A, B):
    """What ksolve_test_reqalg answers for the pairs (A[i], B[i]), from the definition alone."""
    n, nk, rw = len(A), space.nk, space.rw
    e = dict(has_intersection=np.zeros(n, U32), intersects=np.zeros(n, U8), compatible=np.zeros((2, n), U8), op=np.full((n, nk), 0xFF, U8),
             values_word=np.zeros((n, rw), U64), buf_flags=np.zeros((6, n), U32))
    results = []
    for i, (a, b) in enumerate(zip(A, B)):
        e["has_intersection"][i] = sum(1 << space.kidx[k] for k in a if k in b and has_intersection(a[k], b[k]))
        e["intersects"][i] = 0 if bad_keys(a, b) else 1
        e["compatible"][0, i] = compatible(a, b)
        e["compatible"][1, i] = compatible(a, b, space.well_known)
        bits = 0
        for key, r in a.items():
            e["op"][i, space.kidx[key]] = OP_NAMES[operator(r)]
            bits |= space.has_bits(r)
        e["values_word"][i] = space.words(bits)
        res = dict(a)
        add(res, *b.values())
        results.append(res)
        e["buf_flags"][5, i] = 1 if res != a else 0       # `changed`: the requirement set is not what it was
    e["has_word"] = e["values_word"]
    t = encode_sets(space, results)
    e["buf_mask"], e["buf_gte"], e["buf_lte"], e["buf_minv"] = t["mask"], t["gte"], t["lte"], t["minv"]
    for j, f in enumerate(("defined", "complement", "has_gte", "has_lte")):
        e["buf_flags"][j] = t[f]
    e["buf_flags"][4] = [sum(1 << space.kidx[k] for k, r in res.items() if r.min_values is not None) for res in results]
    e["results"] = results
    return e


def mismatches(got, want, fields, limit=8):
    """(field, index) of every word that differs, the first `limit` per field with both values."""
    out = []
    for f in fields:
        g, w = np.asarray(got[f]), np.asarray(want[f])
        if g.shape != w.shape:
            out.append((f, "shape", g.shape, w.shape))
            continue
        for idx in list(zip(*np.nonzero(g != w)))[:limit]:
            out.append((f, tuple(int(x) for x in idx), int(g[idx]), int(w[idx])))
    return out


def check_reqalg(space, A, B, got, want=None, what=""):
    want = want or expected_reqalg(space, A, B)
    bad = mismatches(got, want, REQALG_FIELDS)
    if bad:
        i = next((b[1][-1] if b[0] in ("compatible", "buf_flags") else b[1][0]) for b in bad if b[1] != "shape")
        raise AssertionError(f"{what}: {len(bad)} words differ from the definition, e.g. {bad[:4]}; pair {i}: A = {A[i]}, B = {B[i]}, Add -> {want['results'][i]}")
    return want


# ------------------------------------------------------------------------------------------------ the entry points
class _ReqSets(ctypes.Structure):
    _fields_ = [("n", ctypes.c_uint32)] + [(f, ctypes.c_void_p) for f in ("mask", "defined", "complement", "has_gte", "has_lte", "gte", "lte", "min_values")]


class _ReqalgIn(ctypes.Structure):
    _fields_ = [("n_keys", ctypes.c_uint32), ("key_word_off", ctypes.c_void_p), ("well_known_mask", ctypes.c_uint32), ("value_int", ctypes.c_void_p),
                ("value_is_int", ctypes.c_void_p), ("value_valid", ctypes.c_void_p), ("n", ctypes.c_uint32), ("a", ctypes.POINTER(_ReqSets)), ("b", ctypes.POINTER(_ReqSets))]


class _ReqalgOut(ctypes.Structure):
    _fields_ = [(f, ctypes.c_void_p) for f in REQALG_FIELDS]


INDEX_FIELDS = ("kv_has", "key_undef", "key_compl", "key_neg", "it_alloc_ok")


class _IndexIn(ctypes.Structure):
    _fields_ = [("n_keys", ctypes.c_uint32), ("key_word_off", ctypes.c_void_p), ("key_it", ctypes.c_int32), ("value_int", ctypes.c_void_p), ("value_is_int", ctypes.c_void_p),
                ("value_valid", ctypes.c_void_p), ("n_its", ctypes.c_uint32), ("n_res", ctypes.c_uint32), ("it_reqs", ctypes.POINTER(_ReqSets)), ("it_allocatable", ctypes.c_void_p)]


class _IndexOut(ctypes.Structure):
    _fields_ = [(f, ctypes.c_void_p) for f in INDEX_FIELDS] + [("error", ctypes.c_uint32), ("it_words", ctypes.c_uint32)]


_libs = {}


def _lib(path):
    if path not in _libs:
        lib = ctypes.CDLL(os.path.abspath(path))
        lib.ksolve_test_reqalg.restype = ctypes.c_int
        lib.ksolve_test_reqalg.argtypes = [ctypes.POINTER(_ReqalgIn), ctypes.POINTER(_ReqalgOut)]
        lib.ksolve_test_it_index.restype = ctypes.c_int
        lib.ksolve_test_it_index.argtypes = [ctypes.POINTER(_IndexIn), ctypes.POINTER(_IndexOut)]
        _libs[path] = lib
    return _libs[path]


def _reqsets(t, n, keep):
    cols = {}
    for f in ("mask", "defined", "complement", "has_gte", "has_lte", "gte", "lte", "minv"):
        if t[f] is None:
            cols[f] = None
        else:
            a = np.ascontiguousarray(t[f])
            keep.append(a)
            cols[f] = a.ctypes.data
    return _ReqSets(n, cols["mask"], cols["defined"], cols["complement"], cols["has_gte"], cols["has_lte"], cols["gte"], cols["lte"], cols["minv"])


def run_reqalg(lib_path, space, A, B, null_cols=False):
    """ksolve_test_reqalg on the pairs (A[i], B[i]): one launch. The input tables hold JUNK in bound slots without their flag."""
    n, nk, rw = len(A), space.nk, space.rw
    assert len(B) == n >= 1
    keep = []
    ta, tb = encode_sets(space, A, null_cols, junk=True), encode_sets(space, B, null_cols, junk=True)
    ra, rb = _reqsets(ta, n, keep), _reqsets(tb, n, keep)
    arg = _ReqalgIn(nk, space.off.ctypes.data, space.well_known_mask, space.value_int.ctypes.data, space.value_is_int.ctypes.data, space.value_valid.ctypes.data,
                    n, ctypes.pointer(ra), ctypes.pointer(rb))
    # filled with a pattern no answer has, so that a word the entry point does not write is seen
    out = dict(has_intersection=np.full(n, 0xEEEEEEEE, U32), intersects=np.full(n, 0xEE, U8), compatible=np.full((2, n), 0xEE, U8), op=np.full((n, nk), 0xEE, U8),
               values_word=np.full((n, rw), 0xEEEEEEEEEEEEEEEE, U64), has_word=np.full((n, rw), 0xEEEEEEEEEEEEEEEE, U64), buf_mask=np.full((n, rw), 0xEEEEEEEEEEEEEEEE, U64),
               buf_flags=np.full((6, n), 0xEEEEEEEE, U32), buf_gte=np.full((n, nk), 0x6E6E6E6E6E6E6E6E, I64), buf_lte=np.full((n, nk), 0x6E6E6E6E6E6E6E6E, I64),
               buf_minv=np.full((n, nk), 0x6E6E6E6E, I32))
    o = _ReqalgOut(*[out[f].ctypes.data for f in REQALG_FIELDS])
    st = _lib(lib_path).ksolve_test_reqalg(ctypes.byref(arg), ctypes.byref(o))
    assert st == 0, f"ksolve_test_reqalg: status {st}"
    return out


# ------------------------------------------------------------------------------------------------ table cases
_G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ZONE = "topology.kubernetes.io/zone"
# every value the tables and the Gt / Lt / Gte / Lte cases name, and a few spare ones
TABLE_VALUES = ["A", "B", "1", "2", "9", "C", "10", "0", "-1", "3", "4", "5", "6", "7", "8", "abc", "test"]


def table_space():
    return Space([("key", TABLE_VALUES), (ZONE, TABLE_VALUES)], well_known=[ZONE])


def golden_tables():
    with open(os.path.join(_G, "requirement_tables.json")) as f:
        tables = json.load(f)
    with open(os.path.join(_G, "requirements_compatible.json")) as f:
        compat = json.load(f)
    return tables, compat


def table_struct(defs, exp):
    """the expected column of an Intersection row: a definition's name, or the struct itself"""
    if isinstance(exp, dict):
        return Req(exp["key"], exp["values"], exp["complement"], exp["gte"], exp["lte"], exp["minValues"])
    return from_selector(defs[exp])


def gte_lte_pairs():
    """The requirements of test_oracle_golden.py::test_gte_lte_operators (requirement_test.go:953-1084), as pairs."""
    r = lambda op, n: new_requirement("key", op, None, str(n))
    gte, lte, gt, lt = (lambda n: r("Gte", n)), (lambda n: r("Lte", n)), (lambda n: r("Gt", n)), (lambda n: r("Lt", n))
    return [(gte(5), gte(5)), (lte(5), lte(5)), (gte(3), lte(7)), (gt(4), gte(5)), (lt(6), lte(5)), (gte(3), gt(5)), (gte(8), gt(5)), (lte(3), lt(9)),
            (gte(0), lte(0)), (gt(INT_MAX), gte(1)), (gte(1), new_requirement("key", "In", None, "abc", "1")), (lte(7), gte(8)), (lt(INT_MIN), gt(INT_MAX - 1))]


# ------------------------------------------------------------------------------------------------ generated pairs
INT_SPELLINGS = ["0", "1", "-1", "2", "9", "10", "007", "+5", "-0", str(INT_MAX), str(INT_MAX - 1), str(INT_MIN), str(INT_MIN + 1)]
NON_INTEGERS = ["9223372036854775808", "-9223372036854775809", "1e3", "0x10", " 1", "", "A", "B", "abc", "zone-a", "1_0"]
BOUNDS = sorted({go_atoi(s) for s in INT_SPELLINGS} | {3, 5, 7, 100})
MIN_VALUES = [None, None, None, None, 0, 1, 2, 50]

# name -> dictionary sizes per key, pairs, null columns, and the generator's knobs: pa = share of the keys A defines (or `few`: A and
# B define 0 to `few` keys), pshare = chance that B takes a key of A, pextra = chance that B takes a key A does not define, pempty =
# chance that A is empty
SHAPES = {
    "a": dict(sizes=[8], pairs=600, null=False, pa=1.0, pshare=1.0, pextra=0.0, pempty=0.22),
    "b": dict(sizes=[5, 8, 3], pairs=1000, null=False, pa=0.7, pshare=0.6, pextra=0.25, pempty=0.03),
    "c": dict(sizes=[64, 65, 130, 1], pairs=400, null=False, pa=0.6, pshare=0.55, pextra=0.2, pempty=0.03),
    "d": dict(sizes=[1 + i % 3 for i in range(32)], pairs=200, null=False, few=3, pshare=0.6, pextra=0.012, pempty=0.03),
    "e": dict(sizes=[2048, 2048, 2048], pairs=60, null=False, pa=0.7, pshare=0.6, pextra=0.25, pempty=0.03),
    "f": dict(sizes=[5, 8, 3], pairs=1000, null=True, pa=0.7, pshare=0.6, pextra=0.25, pempty=0.03),
}
# the shares the definition must report over the pairs of each of shapes a to e (f has no bounds: the bound-related ones do not apply)
SHARES = {"shared key without intersection": 0.10, "escape of requirements.go:260-265": 0.02, "gte > lte collapse": 0.01, "complement result keeps a bound": 0.05,
          "concrete result from bounded operands": 0.02, "strict Compatible nil": 0.10, "strict Compatible undefined key": 0.10, "strict Compatible no intersection": 0.10,
          "loose differs from strict": 0.05}
BOUND_SHARES = ("gte > lte collapse", "complement result keeps a bound", "concrete result from bounded operands")


def shape_space(name):
    """The dictionary of a shape: the spellings first (shuffled), then plain numbers and names. Even keys are well-known."""
    rng = random.Random(f"space {name}")
    keys = []
    for k, size in enumerate(SHAPES[name]["sizes"]):
        pool = INT_SPELLINGS + NON_INTEGERS
        rng.shuffle(pool)
        more = [f"v{j}" if j % 4 == 3 else str(j) for j in range(11, 11 + size)]
        keys.append((f"key{k}", (pool + more)[:size]))
    return Space(keys, well_known=[k for i, (k, _) in enumerate(keys) if i % 2 == 0])


def _bound(rng, ints):
    return rng.choice(ints) if ints and rng.random() < 0.75 else rng.choice(BOUNDS)


def _some(rng, vals):
    if rng.random() < 0.12:
        return rng.sample(vals, rng.randint(0, len(vals)))                  # up to the whole dictionary, or nothing
    return rng.sample(vals, min(len(vals), rng.randint(1, 3)))


def gen_requirement(rng, key, vals, bounds=True):
    ints = sorted({go_atoi(v) for v in vals} - {None})
    mv = rng.choice(MIN_VALUES) if bounds else None
    kinds = ["In"] * 5 + ["NotIn"] * 3 + ["Exists"] * 2 + ["DoesNotExist"] * 3 + (["Gt", "Lt", "Gte", "Lte"] * 2 + ["mixed"] * 4 if bounds else [])
    kind = rng.choice(kinds)
    if kind in ("In", "NotIn"):
        return new_requirement(key, kind, mv, *_some(rng, vals))
    if kind in ("Exists", "DoesNotExist"):
        return new_requirement(key, kind, mv)
    if kind != "mixed":
        return new_requirement(key, kind, mv, str(_bound(rng, ints)))
    # a complement set with a bound and an excluded set together: built in the definition
    r = new_requirement(key, "NotIn", mv, *_some(rng, vals))
    for op in rng.sample(["Gt", "Lt", "Gte", "Lte"], rng.randint(1, 2)):
        r = intersection(r, new_requirement(key, op, rng.choice(MIN_VALUES), str(_bound(rng, ints))))
    return r


def gen_pairs(name):
    """The pairs of a shape: (space, A, B). Seeded: the same lists on every machine."""
    sh = SHAPES[name]
    space = shape_space(name)
    rng = random.Random(f"pairs {name}")
    A, B = [], []
    for _ in range(sh["pairs"]):
        if "few" in sh:
            ka = rng.sample(space.keys, rng.randint(1, sh["few"])) if rng.random() < 0.9 else list(space.keys)
            if rng.random() < 0.25:
                ka.append(space.keys[-1])                                    # bit 31 of the flag words
        else:
            ka = [k for k in space.keys if rng.random() < sh["pa"]] or [rng.choice(space.keys)]
        if rng.random() < sh["pempty"]:
            ka = []
        kb = [k for k in space.keys if rng.random() < (sh["pshare"] if k in ka else sh["pextra"])]
        if not ka and not kb:
            kb = [rng.choice(space.keys)]
        gen = lambda keys: {k: gen_requirement(rng, k, space.values[k], not sh["null"]) for k in dict.fromkeys(keys)}
        A.append(gen(ka))
        B.append(gen(kb))
    return space, A, B


def pair_facts(space, a, b):
    """What the definition reports about one pair: the names of SHARES that hold for it."""
    facts = set()
    for k in a:
        if k not in b:
            continue
        r, q = a[k], b[k]
        if not has_intersection(r, q):
            facts.add("shared key without intersection")
            if negative(r) and negative(q):
                facts.add("escape of requirements.go:260-265")
        gte, lte = _max_ptr(r.gte, q.gte), _min_ptr(r.lte, q.lte)
        res = intersection(q, r)
        bounded = any(x is not None for x in (r.gte, r.lte, q.gte, q.lte))
        if gte is not None and lte is not None and gte > lte:
            facts.add("gte > lte collapse")
        elif res.complement and (res.gte is not None or res.lte is not None):
            facts.add("complement result keeps a bound")
        elif not res.complement and bounded:
            facts.add("concrete result from bounded operands")
    strict, loose = compatible(a, b), compatible(a, b, space.well_known)
    facts.add(("strict Compatible nil", "strict Compatible undefined key", "strict Compatible no intersection")[strict])
    if strict != loose:
        facts.add("loose differs from strict")
    return facts


def shares(space, A, B):
    count = dict.fromkeys(SHARES, 0)
    for a, b in zip(A, B):
        for f in pair_facts(space, a, b):
            count[f] += 1
    return {f: c / len(A) for f, c in count.items()}


# ------------------------------------------------------------------------------------------------ the instance-type index
IT_KEY = "node.kubernetes.io/instance-type"
INDEX_SIZES = [(n, r) for n in (1, 63, 64, 65, 130) for r in (1, 4)]
CONTENTION_SIZES = (64, 2048)


def index_space(n_its):
    """label keys of 3, 65 and 1 values around the instance-type key, whose dictionary is the type list"""
    return Space([("label3", ["x", "y", "z"]), (IT_KEY, [f"type-{i}" for i in range(n_its)]), ("label65", [f"w{i}" for i in range(65)]), ("label1", ["only"])], key_it=IT_KEY)


def index_case(n_its, n_res, kind="ordinary"):
    """(space, types, allocatable [n_res][n_its]). kind: ordinary | contention | wrong-name | bound."""
    space = index_space(n_its)
    rng = random.Random(f"index {n_its} {n_res} {kind}")
    types = []
    alloc = np.array([[rng.randint(0, 1000) for _ in range(n_its)] for _ in range(n_res)], I64)
    for i in range(n_its):
        t = {IT_KEY: new_requirement(IT_KEY, "In", None, f"type-{i}")}
        if kind == "contention":
            t["label3"] = new_requirement("label3", "In", None, "y")       # label65 undefined on every type
            types.append(t)
            continue
        for key in ("label3", "label65", "label1"):
            vals = space.values[key]
            how = rng.choice(["undefined", "In", "In", "NotIn", "Exists", "In []"])
            if how == "In":
                t[key] = new_requirement(key, "In", None, *rng.sample(vals, min(len(vals), rng.randint(1, 3))))
            elif how == "NotIn":
                t[key] = new_requirement(key, "NotIn", None, *rng.sample(vals, min(len(vals), rng.randint(1, 3))))
            elif how == "Exists":
                t[key] = new_requirement(key, "Exists", None)
            elif how == "In []":
                t[key] = new_requirement(key, "In", None)
        if rng.random() < 0.2:
            alloc[rng.randrange(n_res), i] = -rng.randint(1, 5)
        types.append(t)
    if kind == "wrong-name":
        types[n_its // 2][IT_KEY] = new_requirement(IT_KEY, "In", None, f"type-{n_its // 2 + 1}")
    if kind == "bound":
        types[n_its // 2]["label3"] = new_requirement("label3", "Gt", None, "1")
    return space, types, alloc


def expected_it_index(space, types, alloc):
    """The tables of ksp.h (kv_has, key_undef, key_compl, key_neg, it_alloc_ok) and the error word, from the definition: bit `it`
    of kv_has[value] iff the type defines the value's key and its requirement Has() the value; key_undef / key_compl / key_neg iff
    the type does not define the key / its requirement is a complement / its operator is NotIn or DoesNotExist. Rows of the
    instance-type key and bits past n_its stay zero."""
    n_its = len(types)
    iw = (n_its + 63) // 64
    kv = [0] * (space.rw * 64)
    und, cmp_, neg = [0] * space.nk, [0] * space.nk, [0] * space.nk
    ok = error = 0
    for it, t in enumerate(types):
        own = t.get(IT_KEY)
        if own is None or own.struct() != new_requirement(IT_KEY, "In", None, f"type-{it}").struct():
            error |= 1
        if any(r.gte is not None or r.lte is not None for r in t.values()):
            error |= 2
        if all(alloc[x, it] >= 0 for x in range(alloc.shape[0])):
            ok |= 1 << it
        for k, key in enumerate(space.keys):
            if k == space.key_it:
                continue
            if key not in t:
                und[k] |= 1 << it
                continue
            r = t[key]
            if r.complement:
                cmp_[k] |= 1 << it
            if negative(r):
                neg[k] |= 1 << it
            for v, p in space.bitpos[key].items():
                if has(r, v):
                    kv[p] |= 1 << it
    words = lambda rows: np.array([np.frombuffer(b.to_bytes(iw * 8, "little"), U64) for b in rows], U64).reshape(len(rows), iw)
    return dict(kv_has=words(kv), key_undef=words(und), key_compl=words(cmp_), key_neg=words(neg), it_alloc_ok=words([ok])[0], error=error, it_words=iw)


def run_it_index(lib_path, space, types, alloc):
    n_its, n_res = len(types), alloc.shape[0]
    iw = (n_its + 63) // 64
    keep = []
    t = encode_sets(space, types)
    rs = _reqsets(t, n_its, keep)
    alloc = np.ascontiguousarray(alloc, I64)
    arg = _IndexIn(space.nk, space.off.ctypes.data, space.key_it, space.value_int.ctypes.data, space.value_is_int.ctypes.data, space.value_valid.ctypes.data,
                   n_its, n_res, ctypes.pointer(rs), alloc.ctypes.data)
    fill = 0xEEEEEEEEEEEEEEEE
    out = dict(kv_has=np.full((space.rw * 64, iw), fill, U64), key_undef=np.full((space.nk, iw), fill, U64), key_compl=np.full((space.nk, iw), fill, U64),
               key_neg=np.full((space.nk, iw), fill, U64), it_alloc_ok=np.full(iw, fill, U64))
    o = _IndexOut(*[out[f].ctypes.data for f in INDEX_FIELDS], 0xEEEEEEEE, 0xEEEEEEEE)
    st = _lib(lib_path).ksolve_test_it_index(ctypes.byref(arg), ctypes.byref(o))
    assert st == 0, f"ksolve_test_it_index: status {st}"
    out["error"], out["it_words"] = o.error, o.it_words
    return out


def check_it_index(got, want, what="", tables=True):
    assert (got["error"], got["it_words"]) == (want["error"], want["it_words"]), (what, "error word / it_words", got["error"], got["it_words"], want["error"], want["it_words"])
    if tables:
        bad = mismatches(got, want, INDEX_FIELDS)
        assert not bad, (what, bad[:6])


# ------------------------------------------------------------------------------------------------ the runs both tests share
def run_tables(lib, golden):
    """The reference's tables through ksolve_test_reqalg, one launch per table; returns what every launch answered."""
    tables, compat = golden
    defs, space = tables["definitions"], table_space()
    one = lambda name: {"key": from_selector(defs[name])}
    # Intersection rows through reqbuf_add, field for field; HasIntersection against "the table's result is not empty"
    rows = tables["intersection"]
    A, B = [one(a) for a, _, _ in rows], [one(b) for _, b, _ in rows]
    outs = []
    got = run_reqalg(lib, space, A, B)
    outs.append(got)
    check_reqalg(space, A, B, got, what="intersection table")
    for i, (a, b, exp) in enumerate(rows):
        struct = table_struct(defs, exp)
        buf = decode_sets(space, dict(mask=got["buf_mask"], defined=got["buf_flags"][0], complement=got["buf_flags"][1], has_gte=got["buf_flags"][2],
                                         has_lte=got["buf_flags"][3], gte=got["buf_gte"], lte=got["buf_lte"], minv=got["buf_minv"]), i)
        assert buf == {"key": struct}, (a, b, exp, buf)
        assert (int(got["has_intersection"][i]) & 1) == (1 if struct.complement or struct.values else 0), (a, b)
    # Has rows through req_has and req_values_word, Operator rows through req_op
    rows = tables["has"]
    A = [one(name) for name, _, _ in rows]
    got = run_reqalg(lib, space, A, A)
    outs.append(got)
    check_reqalg(space, A, A, got, what="has table")
    for i, (name, value, exp) in enumerate(rows):
        p = space.bitpos["key"][value]
        for f in ("has_word", "values_word"):
            assert ((int(got[f][i, p // 64]) >> (p % 64)) & 1) == int(exp), (name, value, f)
    rows = tables["operator"]
    A = [one(name) for name, _ in rows]
    got = run_reqalg(lib, space, A, A)
    outs.append(got)
    check_reqalg(space, A, A, got, what="operator table")
    assert [int(got["op"][i, 0]) for i in range(len(rows))] == [OP_NAMES[op] for _, op in rows]
    # Compatible rows, the zone key well-known: strict is allow_undefined = false, loose = true
    cdefs = compat["definitions"]
    sets = lambda name: {} if cdefs[name] is None else {cdefs[name]["key"]: from_selector(cdefs[name])}
    for j, mode in enumerate(("strict", "loose")):
        A, B = [sets(a) for a, _, _ in compat[mode]], [sets(b) for _, b, _ in compat[mode]]
        got = run_reqalg(lib, space, A, B)
        outs.append(got)
        check_reqalg(space, A, B, got, what=f"compatible table ({mode})")
        for i, (a, b, exp) in enumerate(compat[mode]):
            assert (int(got["compatible"][j, i]) == COMPAT_OK) == exp, (mode, a, b)
    # the Gt / Lt / Gte / Lte cases
    pairs = gte_lte_pairs()
    A, B = [{"key": a} for a, _ in pairs], [{"key": b} for _, b in pairs]
    outs.append(run_reqalg(lib, space, A, B))
    check_reqalg(space, A, B, outs[-1], what="gte / lte cases")
    return outs


def run_shape(lib, name):
    """The generated pairs of a shape: one launch."""
    space, A, B = gen_pairs(name)
    got = run_reqalg(lib, space, A, B, null_cols=SHAPES[name]["null"])
    assert np.array_equal(got["values_word"], got["has_word"]), (name, "req_values_word differs from req_has bit by bit")
    check_reqalg(space, A, B, got, what=f"shape {name}")
    return got


def run_index(lib, n_its, n_res, kind):
    space, types, alloc = index_case(n_its, n_res, kind)
    got = run_it_index(lib, space, types, alloc)
    want = expected_it_index(space, types, alloc)
    assert want["error"] == {"ordinary": 0, "contention": 0, "wrong-name": 1, "bound": 2}[kind]
    # (a type with a bound is refused by the error word: the index of such a problem is never read)
    check_it_index(got, want, what=(kind, n_its, n_res), tables=kind != "bound")
    return got, want


def same_outputs(one, other, fields):
    """The fields in which two runs of the same case (device and emulation) differ, bit for bit: none expected, also where the
    definition leaves a field open."""
    return [f for f in fields if not np.array_equal(np.asarray(one[f]), np.asarray(other[f]))]
