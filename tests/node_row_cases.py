"""The static (class, node) rows (ksolve_node_dead0: csrc/kernels.h node_dead0_body over csrc/nodecheck.h) against their definition,
stated here on Python sets and ints. Requirements, the dictionary, Requirements.Compatible and the encoder are those of
tests/reqalg_cases.py (Req, Space, compatible, encode_sets): nothing of them is restated.

THE DEFINITION (existingnode.go:81-102). Bit e of dead0[k] is set iff
  * the node has a taint the class does not tolerate (:83), or
  * hp_on, the class side has a host-port table, and node.hp & cls_hp[k][1] != 0 (:87-93), or
  * resources.Fits fails (:96): some remaining[r] < 0, or request[r] > remaining[r], or
  * node.requirements.Compatible(class.requirements) returns an error (:100) — no AllowUndefined option: a key the node does not
    define is allowed only under the class's NotIn or DoesNotExist, or
  * e >= n_nodes.

THE LAYOUT. A key takes whole mask words (reqalg_cases.Space), so the small dictionary's 3 keys take 3 words and the wide one's 6
keys take 7: one key of 70 values over two words, one integer-valued key under the classes' Gt and Lt (inbounds_word,
empty_bounds), and a second integer-valued key for the single differences.

run_node_rows() drives the test-only entry point ksolve_test_node_dead0 of a test build of the solver library: the class records
laid out by the product's own class gather, one launch of the kernel. Every comparison is exact, bits past the last node included."""
import copy
import ctypes
import functools
import os
import random

import numpy as np

from reqalg_cases import I64, U32, U64, Req, Space, _ReqSets, _reqsets, compatible, encode_sets, new_requirement

REASONS = ("taint", "host port", "resources", "requirements")


# ------------------------------------------------------------------------------------------------ the definition
def reasons(p, k, e):
    """the reasons of THE DEFINITION that hold for class k on node e (none: the node stays alive for the class)"""
    out = []
    if int(p["taints"][e]) & ~int(p["tolerates"][k]) & (2**64 - 1):
        out.append("taint")
    if p["hp_on"] and p["cls_hp"] is not None and p["node_hp"] is not None and int(p["node_hp"][e]) & int(p["cls_hp"][k][1]):
        out.append("host port")
    if any(int(p["remaining"][r][e]) < 0 or int(p["requests"][r][k]) > int(p["remaining"][r][e]) for r in range(p["n_res"])):
        out.append("resources")
    if compatible(p["nodes"][e], p["classes"][k]) != 0:
        out.append("requirements")
    return out


def expected_rows(p):
    """dead0 as [n_classes][node_words] from the definition, and the reasons of every pair"""
    nn, nc = len(p["nodes"]), len(p["classes"])
    nw = (nn + 63) // 64
    why = {(k, e): reasons(p, k, e) for k in range(nc) for e in range(nn)}
    past = sum(1 << e for e in range(nn, nw * 64))
    rows = [past | sum(1 << e for e in range(nn) if why[k, e]) for k in range(nc)]
    return np.array([np.frombuffer(b.to_bytes(nw * 8, "little"), U64) for b in rows], U64).reshape(nc, nw), why


def dead_pairs(table, nn):
    """the (class, node) pairs a table marks dead, and whether every bit past the last node is set"""
    bits = [int.from_bytes(np.ascontiguousarray(row).tobytes(), "little") for row in table]
    past = all(b >> nn == (1 << (table.shape[1] * 64 - nn)) - 1 for b in bits)
    return {(k, e) for k, b in enumerate(bits) for e in range(nn) if (b >> e) & 1}, past


# ------------------------------------------------------------------------------------------------ the dictionaries
WIDE = [f"w{i}" for i in range(70)]


def small_space():
    return Space([("zone", ["a", "b", "c"]), ("arch", ["amd64", "arm64"]), ("tier", ["1", "2", "3", "x"])])


def wide_space():
    return Space([("zone", ["a", "b", "c"]), ("wide", WIDE), ("gen", ["1", "2", "3", "5", "8", "13", "x"]), ("arch", ["amd64", "arm64"]), ("team", ["t1", "t2", "t3", "t4"]),
                  ("rack", ["1", "2", "3", "4", "5"])])


SPACES = {"small": small_space, "wide": wide_space}
INT_KEYS = ("tier", "gen", "rack")


# ------------------------------------------------------------------------------------------------ generated problems
# (n_nodes, n_classes, n_res, dictionary, host ports: on | off = the tables with hp_on 0 | none = no tables)
GRID = [(1, 1, 2, "small", "on"), (1, 1, 2, "wide", "on"), (63, 31, 2, "small", "none"), (63, 31, 2, "wide", "on"), (64, 32, 2, "small", "on"), (64, 32, 3, "wide", "off"),
        (65, 33, 2, "small", "on"), (65, 33, 2, "wide", "on"), (130, 70, 2, "small", "on"), (130, 70, 2, "wide", "on"), (65, 33, 1, "wide", "on"), (65, 33, 4, "wide", "on"),
        (65, 33, 8, "wide", "on")]
TAINT_BITS, PORT_BITS = (0, 5, 63), (0, 7, 63)


def grid_id(case):
    return "%dx%d-res%d-%s-hp_%s" % tuple(case)


def _class_req(rng, key, vals):
    ints = [v for v in vals if v.lstrip("-").isdigit()]
    kind = rng.choice(["In"] * 6 + ["NotIn"] * 3 + ["Exists"] * 2 + ["DoesNotExist"] + (["Gt", "Lt", "GtLt", "GtLt"] if key in INT_KEYS else []))
    if kind == "In":
        return new_requirement(key, "In", None, *rng.sample(vals, min(len(vals), rng.randint(1, 3))))
    if kind == "NotIn":
        return new_requirement(key, "NotIn", None, *rng.sample(vals, min(len(vals), rng.randint(1, 2))))
    if kind in ("Exists", "DoesNotExist"):
        return new_requirement(key, kind, None)
    if kind in ("Gt", "Lt"):
        return new_requirement(key, kind, None, rng.choice(ints))
    lo, hi = int(rng.choice(ints)), int(rng.choice(ints))        # Gt lo and Lt hi together: one in four is an empty range
    return Req(key, (), True, gte=lo + 1, lte=hi - 1)


def _node_req(rng, key, vals):
    kind = rng.choice(["In"] * 14 + ["In many"] * 2 + ["NotIn"] * 3 + ["Exists"])
    if kind == "In":
        return new_requirement(key, "In", None, rng.choice(vals[:3] + vals[-2:]))      # (the first and the last values: both words of the wide key)
    if kind == "In many":
        return new_requirement(key, "In", None, *rng.sample(vals, min(len(vals), 3)))
    if kind == "NotIn":
        return new_requirement(key, "NotIn", None, *rng.sample(vals, min(len(vals), rng.randint(1, 2))))
    return new_requirement(key, "Exists", None)


@functools.lru_cache(maxsize=None)
def generated(nn, nc, n_res, space_name, hp):
    """A seeded problem of the grid, with its expected table: built once, shared, not to be changed."""
    space = SPACES[space_name]()
    rng = random.Random(f"node rows {nn} {nc} {n_res} {space_name}")
    word = lambda bits, p: sum(1 << b for b in bits if rng.random() < p)
    classes, nodes = [], []
    for _ in range(nc):
        classes.append({k: _class_req(rng, k, space.values[k]) for k in space.keys if rng.random() < 1.2 / space.nk})
    for _ in range(nn):
        nodes.append({k: _node_req(rng, k, space.values[k]) for k in space.keys if rng.random() < 0.85})
    p = dict(space=space, classes=classes, nodes=nodes, n_res=n_res, hp_on=1 if hp == "on" else 0)
    p["tolerates"] = np.array([(rng.getrandbits(64) & ~sum(1 << b for b in TAINT_BITS)) | word(TAINT_BITS, 0.7) for _ in range(nc)], U64)
    p["taints"] = np.array([word(TAINT_BITS, 0.14) for _ in range(nn)], U64)
    # (cls_hp[k][0], the ports the class binds, holds every bit a node may hold: only word [1] may decide)
    p["cls_hp"] = None if hp == "none" else np.array([[sum(1 << b for b in PORT_BITS) | rng.getrandbits(64), word(PORT_BITS, 0.25)] for _ in range(nc)], U64)
    p["node_hp"] = None if hp == "none" else np.array([word(PORT_BITS, 0.17) for _ in range(nn)], U64)
    p["requests"] = np.array([[rng.randint(0, 4) for _ in range(nc)] for _ in range(n_res)], I64)
    rem = lambda: -rng.randint(1, 3) if rng.random() < 0.05 / n_res else rng.randint(0, 3) if rng.random() < 0.17 / n_res else rng.randint(4, 1 << 40)
    p["remaining"] = np.array([[rem() for _ in range(nn)] for _ in range(n_res)], I64)
    p["expected"], p["why"] = expected_rows(p)
    for a in p.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return p


def shares(p):
    """of all pairs: alive, dead, and each reason as the only one"""
    n = len(p["why"])
    out = {"alive": sum(1 for w in p["why"].values() if not w) / n}
    out["dead"] = 1 - out["alive"]
    for r in REASONS:
        out[r] = sum(1 for w in p["why"].values() if w == [r]) / n
    return out


# ------------------------------------------------------------------------------------------------ single differences
def base_problem(e0, k0, nn=65, nc=33, n_res=8):
    """A wide-dictionary problem in which every pair is alive, with node e0 and class k0 prepared for the single differences: node e0
    alone leaves `team` undefined, holds one value of `wide` and of `gen` where the others hold more or another, and carries a
    complement set on `rack`."""
    space = wide_space()
    variants = [{}, {"zone": new_requirement("zone", "In", None, "a", "b")}, {"gen": new_requirement("gen", "Gt", None, "2")}, {"wide": new_requirement("wide", "In", None, "w65", "w1")},
                {"arch": new_requirement("arch", "NotIn", None, "arm64"), "zone": new_requirement("zone", "Exists", None)}, {"rack": new_requirement("rack", "Lt", None, "4")},
                {"wide": new_requirement("wide", "NotIn", None, "w0", "w64")}, {"team": new_requirement("team", "NotIn", None, "t3"), "gen": new_requirement("gen", "Lt", None, "13")}]
    classes = [dict(variants[k % len(variants)]) for k in range(nc)]
    classes[k0] = {}
    nodes = []
    for e in range(nn):
        nodes.append({"zone": new_requirement("zone", "In", None, "ab"[e % 2]), "wide": new_requirement("wide", "In", None, "w65", "w66"), "gen": new_requirement("gen", "In", None, "8"),
                      "arch": new_requirement("arch", "In", None, "amd64"), "rack": new_requirement("rack", "In", None, "2")})
    nodes[e0] = {"zone": new_requirement("zone", "In", None, "a"), "wide": new_requirement("wide", "In", None, "w65"), "gen": new_requirement("gen", "In", None, "3"),
                 "arch": new_requirement("arch", "In", None, "amd64"), "rack": new_requirement("rack", "NotIn", None, "1")}
    for e in range(nn):     # (a class that names `team` under NotIn stays alive on e0, the only node without the key)
        if e != e0:
            nodes[e]["team"] = new_requirement("team", "In", None, "t1")
    p = dict(space=space, classes=classes, nodes=nodes, n_res=n_res, hp_on=1)
    p["tolerates"] = np.full(nc, 2**64 - 1, U64)
    p["taints"] = np.zeros(nn, U64)
    p["cls_hp"] = np.array([[1 << (k % 64), 1 << (k % 64)] for k in range(nc)], U64)      # class k conflicts with port bit k alone
    p["node_hp"] = np.zeros(nn, U64)
    p["requests"] = np.array([[1 + (k + r) % 5 for k in range(nc)] for r in range(n_res)], I64)
    p["remaining"] = np.full((n_res, nn), 100, I64)
    return p


def _changes(n_res):
    """name -> (the change on a copy of the base problem, what must flip: pair | none | column (every class on the node) | row (the class
    on every node))"""
    def taint(b):
        def f(p, e, k):
            p["taints"][e] = 1 << b
            p["tolerates"][k] = (2**64 - 1) & ~(1 << b)
        return f

    def port(on):
        def f(p, e, k):
            p["node_hp"][e] = int(p["cls_hp"][k][1])
            p["hp_on"] = on
        return f

    def short(r):
        def f(p, e, k):
            p["requests"][r][k] = 50
            p["remaining"][r][e] = 49        # request[r] - 1; the other classes ask for at most 5
        return f

    def negative(r, request):
        def f(p, e, k):
            p["requests"][r][k] = request
            p["remaining"][r][e] = -1
        return f

    def cls(req):
        def f(p, e, k):
            p["classes"][k] = {req.key: req}
        return f
    ch = {"taint bit 0": (taint(0), "pair"), "taint bit 63": (taint(63), "pair"), "host port": (port(1), "pair"), "host port, hp_on 0": (port(0), "none")}
    for r in range(n_res):
        ch[f"remaining[{r}] = request - 1"] = (short(r), "pair")
    for r in (0, n_res - 1):
        ch[f"remaining[{r}] = -1, request 0"] = (negative(r, 0), "column")
    for r in range(n_res):                                                   # (only the `remaining < 0` half of Fits refuses these)
        ch[f"remaining[{r}] = -1, request -2"] = (negative(r, -2), "column")
    ch["In on a key the node does not define"] = (cls(new_requirement("team", "In", None, "t1")), "pair")
    ch["NotIn on a key the node does not define"] = (cls(new_requirement("team", "NotIn", None, "t2")), "none")
    ch["disjoint In on the second word"] = (cls(new_requirement("wide", "In", None, "w66")), "pair")
    ch["Gt above the node's only value"] = (cls(new_requirement("gen", "Gt", None, "5")), "pair")
    ch["Gt and Lt with an empty range"] = (cls(Req("rack", (), True, gte=4, lte=2)), "row")
    return ch


CHANGES = _changes(8)
POSITIONS = [(64, 32), (0, 0)]


def changed_problem(e0, k0, name):
    p = copy.deepcopy(base_problem(e0, k0))
    CHANGES[name][0](p, e0, k0)
    return p


def flips_of(kind, e0, k0, nn=65, nc=33):
    return {"pair": {(k0, e0)}, "none": set(), "column": {(k, e0) for k in range(nc)}, "row": {(k0, e) for e in range(nn)}}[kind]


# ------------------------------------------------------------------------------------------------ position independence
CLASS_SPOTS, NODE_SPOTS = (0, 31, 32, 69), (0, 63, 64, 129)


@functools.lru_cache(maxsize=None)
def position_problem():
    """the (130, 70) wide problem with one class row at CLASS_SPOTS and one node at NODE_SPOTS"""
    p = copy.deepcopy(generated(130, 70, 2, "wide", "on"))
    for i, spots in ((0, CLASS_SPOTS), (1, NODE_SPOTS)):
        src = spots[1] + 6
        for s in spots:
            if i == 0:
                p["classes"][s] = p["classes"][src]
                p["tolerates"][s], p["cls_hp"][s], p["requests"][:, s] = p["tolerates"][src], p["cls_hp"][src], p["requests"][:, src]
            else:
                p["nodes"][s] = p["nodes"][src]
                p["taints"][s], p["node_hp"][s], p["remaining"][:, s] = p["taints"][src], p["node_hp"][src], p["remaining"][:, src]
    p["expected"], p["why"] = expected_rows(p)
    return p


# ------------------------------------------------------------------------------------------------ the entry point
class _NodeIn(ctypes.Structure):
    _fields_ = [("n_keys", ctypes.c_uint32), ("key_word_off", ctypes.c_void_p), ("value_int", ctypes.c_void_p), ("value_is_int", ctypes.c_void_p), ("value_valid", ctypes.c_void_p),
                ("n_classes", ctypes.c_uint32), ("n_res", ctypes.c_uint32), ("cls_reqs", ctypes.POINTER(_ReqSets)), ("requests", ctypes.c_void_p), ("tolerates", ctypes.c_void_p),
                ("host_ports", ctypes.c_void_p), ("n_nodes", ctypes.c_uint32), ("hp_on", ctypes.c_uint32), ("node_mask", ctypes.c_void_p), ("node_defined", ctypes.c_void_p),
                ("node_complement", ctypes.c_void_p), ("node_remaining", ctypes.c_void_p), ("node_taints", ctypes.c_void_p), ("node_hp", ctypes.c_void_p)]


class _NodeOut(ctypes.Structure):
    _fields_ = [("dead0", ctypes.c_void_p), ("node_words", ctypes.c_uint32)]


_libs = {}


def _lib(path):
    if path not in _libs:
        lib = ctypes.CDLL(os.path.abspath(path))
        lib.ksolve_test_node_dead0.restype = ctypes.c_int
        lib.ksolve_test_node_dead0.argtypes = [ctypes.POINTER(_NodeIn), ctypes.POINTER(_NodeOut)]
        _libs[path] = lib
    return _libs[path]


def run_node_rows(lib_path, p):
    """ksolve_test_node_dead0 on a problem: dead0 as [n_classes][node_words]. The class tables hold JUNK in bound slots without their
    flag bit; the output starts as a pattern no answer has."""
    space, nn, nc, nr = p["space"], len(p["nodes"]), len(p["classes"]), p["n_res"]
    nw = (nn + 63) // 64
    keep = []
    cls = _reqsets(encode_sets(space, p["classes"], junk=True), nc, keep)
    nt = encode_sets(space, p["nodes"], null_cols=True)       # (label sets: no bounds)
    tabs = dict(requests=np.ascontiguousarray(p["requests"], I64), tolerates=np.ascontiguousarray(p["tolerates"], U64), node_mask=np.ascontiguousarray(nt["mask"].T),
                node_defined=np.ascontiguousarray(nt["defined"], U32), node_complement=np.ascontiguousarray(nt["complement"], U32),
                node_remaining=np.ascontiguousarray(p["remaining"], I64), node_taints=np.ascontiguousarray(p["taints"], U64),
                host_ports=None if p["cls_hp"] is None else np.ascontiguousarray(p["cls_hp"], U64), node_hp=None if p["node_hp"] is None else np.ascontiguousarray(p["node_hp"], U64))
    assert tabs["requests"].shape == (nr, nc) and tabs["node_remaining"].shape == (nr, nn) and tabs["node_mask"].shape == (space.rw, nn)
    ptr = lambda f: None if tabs[f] is None else tabs[f].ctypes.data
    arg = _NodeIn(space.nk, space.off.ctypes.data, space.value_int.ctypes.data, space.value_is_int.ctypes.data, space.value_valid.ctypes.data, nc, nr, ctypes.pointer(cls),
                  ptr("requests"), ptr("tolerates"), ptr("host_ports"), nn, p["hp_on"], ptr("node_mask"), ptr("node_defined"), ptr("node_complement"), ptr("node_remaining"),
                  ptr("node_taints"), ptr("node_hp"))
    out = np.full((nc, nw), 0xEEEEEEEEEEEEEEEE, U64)
    o = _NodeOut(out.ctypes.data, 0xEEEEEEEE)
    st = _lib(lib_path).ksolve_test_node_dead0(ctypes.byref(arg), ctypes.byref(o))
    assert st == 0, f"ksolve_test_node_dead0: status {st}"
    assert o.node_words == nw
    return out


def check_rows(p, got, want=None, what=""):
    """every word of the table against the definition; a mismatch names the pairs and their reasons"""
    if want is None:
        want = p["expected"] if "expected" in p else expected_rows(p)[0]
    if np.array_equal(got, want):
        return
    nn = len(p["nodes"])
    g, gp = dead_pairs(got, nn)
    w, _ = dead_pairs(want, nn)
    wrong = sorted(g ^ w)
    k, e = wrong[0] if wrong else (0, 0)
    raise AssertionError(f"{what}: {len(wrong)} pairs differ from the definition (bits past the last node all dead: {gp}), e.g. {wrong[:6]}; class {k} {p['classes'][k]} on node {e} "
                         f"{p['nodes'][e]}: the definition says {reasons(p, k, e) or 'alive'}")


# ------------------------------------------------------------------------------------------------ the runs both tests share
def run_generated(lib, case):
    p = generated(*case)
    got = run_node_rows(lib, p)
    check_rows(p, got, what=str(case))
    return got


def run_single_differences(lib, e0, k0):
    """Test B: the base table and the table behind every change; only what the change's kind names may differ between the two."""
    base = base_problem(e0, k0)
    tables = [run_node_rows(lib, base)]
    check_rows(base, tables[0], what=f"base problem, node {e0} / class {k0}")
    assert not tables[0][:, 0].any() and (tables[0][:, 1] == np.uint64(2**64 - 2)).all()
    for name, (_, kind) in CHANGES.items():
        p = changed_problem(e0, k0, name)
        got = run_node_rows(lib, p)
        flipped, past = dead_pairs(got ^ tables[0], 65)
        assert flipped == flips_of(kind, e0, k0), (name, f"node {e0} / class {k0}", kind, sorted(flipped)[:6])
        check_rows(p, got, what=f"{name}, node {e0} / class {k0}")
        tables.append(got)
    return tables


def run_positions(lib):
    """Test C: one class row at four indices, one node at four indices: equal verdicts."""
    p = position_problem()
    got = run_node_rows(lib, p)
    for k in CLASS_SPOTS[1:]:
        assert np.array_equal(got[k], got[CLASS_SPOTS[0]]), ("class row", k)
    bit = lambda e: (got[:, e // 64] >> np.uint64(e % 64)) & np.uint64(1)
    for e in NODE_SPOTS[1:]:
        assert np.array_equal(bit(e), bit(NODE_SPOTS[0])), ("node", e)
    check_rows(p, got, what="position problem")
    return got
