"""The cold half of the cursor engine (csrc/fast_engine.h FastCold: setup(), compat_word, offering_cells, create_entry, fast_lookup /
fast_fits / fast_fields_ok, filter_diag, new_slot, new_claim with row_accepts, refresh_claim) against its definition, restated here on
Python sets of strings and Python ints.

THE DEFINITION works on requirement sets as tests/reqalg_cases.py has them (dict key -> Req; compatible / bad_keys / has / add are the
restatement of requirement.go and requirements.go there) and on plain lists. Nothing is shared with the oracle library or with the
product's bit-mask code:

  prefilter       scheduler.go:156-171 — t_its[t] = the types of tmpl_its[t] without a negative allocatable, whose requirements
                  Intersect the template's (requirements.go:254-274) and that have an available offering in a zone x capacity-type
                  cell the template admits; active_templates = the templates with a non-empty list
  packing         the variable keys = the keys some class defines, in key order; a field per key (one bit per dictionary value, one
                  phantom bit on top under pod operators), one guard bit behind each field; pack_set() gives the packed word of any
                  requirement set, the templates' (tvmask) and the classes' (cvmask / dmask / kdef) among them
  tmplok          taints tolerated and no custom key the template leaves undefined, with the pod-operator refinements of setup()
  declines        decline.h's reasons 1, 3 to 12, in the order setup() tests them
  F(set)          nodeclaim.go:541-638 — the types of the id's t_its row whose requirements Intersect the merged set and that have an
                  available offering in a cell the merged set admits; ent_its row = F
  Pareto front    the distinct effective-allocatable vectors of F that no other dominates, in descending lexicographic order: the first
                  in FastEnt::cap (0x3FFFFFFF in unused resources), the others in the pool from the entry's offset; at most 1 + 16 per
                  set (kFastMaxPareto) and 256 pool rows (kFastPool); the cache takes 820 entries (80 % of 1,024)
  fits            some type of F has an effective allocatable >= req + size in every resource — what fast_fits must say
  fields_ok       Requirements.Compatible of the claim's set with the class's, where tmplok has said yes
  CanAdd          nodeclaim.go:124-242 — taints, Compatible, and some type of F(merged set) holds the claim's requests plus the pod's:
                  bit s of row j of every claim's acceptance word, after every event (Model.check_words)
  new_claim       scheduler.go:695-790 — the first template in order that takes the pod, a hostname number per template attempted,
                  the first error in template order with InstanceTypeFilterError's flags (nodeclaim.go:585-592), the verdict kept
                  per class while the limits stand, DECLINE_UNSCHEDULABLE_POD as the retry's net, DECLINE_KERNEL_CAPACITY /
                  DECLINE_CLAIM_SLOTS
  limits          scheduler.go:706-727, 1049-1085 — `remaining` per NodePool; a pool with no node left or no viable type is skipped
                  (E_LIMITS, no hostname number); a type list narrower than the pool's current one opens a LIMIT STAGE: the next id
                  below 32 with that list, the template's packed word under the id, bit t of every class's tmplok copied to its
                  bit, `first_claim` at the first narrowing, DECLINE_LIMIT_STAGES when no id is left; a created claim takes the
                  largest capacity among the types of F that hold the pod off `remaining` (the `nodes` entry is consulted, never
                  counted down by the cold path) and voids every kept verdict; without limit stages the engine stops at the first
                  exclusion (DECLINE_LIMIT_NODES / DECLINE_LIMIT_EXCLUDES_TYPE)
  new_slot        the row with the most classes that could share a claim with this one, the emptiest among equals, its first free
                  lane; every slot taken: all dropped, slot 0, bit 16 in the answer

A reachable requirement set is (template t, the classes merged into it): run() hands the kernel pack_set() of the merged set, never
an AND of packed words, except where the operation under test IS the AND (FITS: the loop's `st.vmask & cvmask`).

run() drives ksolve_test_fast_cold of a test build of the solver library (tests/emu/libksolve_emu.so on the host,
tests/emu/libksolve_hooks.so on the GPU); expected() is the same answer from the definition; mismatches() lists every field that
differs. EXCLUDED from the comparison, because the definition leaves them open: FastVar and FastMisc's vkey / voff / vwidth / vword /
fmask past nv, FastMisc::its / rem / cand / acc (scratch), pool rows past n_pool, the vmask / cap / info bits 8.. of invalid cache
entries, ent_its rows of invalid slots, the records of free class slots, everything but setup's return value when setup() declines,
and nothing else: the acceptance bits of slots that new_slot dropped all at once and no class has taken again are whatever the claims held
at the drop, which the model keeps (Model.stale) and the comparison holds bit for bit."""
import ctypes
import os
import random

import numpy as np

from reqalg_cases import (COMPAT_OK, I32, I64, U32, U64, Space, _ReqSets, _reqsets, add, bad_keys, compatible, encode_sets, has, negative,
                          new_requirement, operator)

ZONE, CT, IT_KEY, HOSTNAME = "topology.kubernetes.io/zone", "karpenter.sh/capacity-type", "node.kubernetes.io/instance-type", "kubernetes.io/hostname"
K_ENT, K_POOL, K_EXTRA, K_MAX_VAR, K_VAR_BITS = 1024, 256, 16, 12, 56       # fast_engine.h kFastEnt, kFastPool, kFastMaxPareto, kFastMaxVar, kFastVarBits
K_GATE = 820                                                               # entries the cache takes: n_ent * 5 < 1,024 * 4
EXT_BIT, UNUSED_CAP = 1 << 63, 0x3FFFFFFF
K_EFF_NEVER = -((1 << 30) - 1)                                             # kernels.h kEffNever
OP_ENTRY, OP_FITS, OP_CELLS, OP_COMPAT, OP_DIAG, OP_SLOT, OP_NEWCLAIM, OP_ADD = 1, 2, 3, 4, 5, 6, 7, 8       # fast_cold_probe.h FCOP_*
FREE = 0xFFFFFFFF                                                          # kFastFree
E_TAINTS, E_INCOMPATIBLE, E_INSTANCE_TYPES, E_NO_TEMPLATES, E_LIMITS = 1, 2, 4, 6, 7     # engine.h E_*
DECLINE_KERNEL_CAPACITY, DECLINE_CACHE_FULL, DECLINE_CACHE_FULL_NEW_CLAIM, DECLINE_CLAIM_SLOTS, DECLINE_UNSCHEDULABLE_POD = -1, 20, 25, 26, 27
DECLINE_LIMIT_NODES, DECLINE_LIMIT_EXCLUDES_TYPE, DECLINE_LIMIT_STAGES = 23, 24, 29
NO_CLAIM = 0xFFFFFFFF
(DECLINE_NOT_PLAIN, DECLINE_TEMPLATE_NOT_POSITIVE, DECLINE_CLASS_NOT_POSITIVE, DECLINE_SELECTS_HOST_OR_TYPE, DECLINE_KEYS_DO_NOT_PACK, DECLINE_QUANTITY_RANGE,
 DECLINE_CLASS_EMPTY_IN, DECLINE_CLASS_KEY_DEFINEDNESS, DECLINE_CLASS_DNE_MIXED, DECLINE_CLASS_NOTIN_BOUNDS, DECLINE_CLASS_EXISTS_UNDEFINED) = 1, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12
KSOLVE_ERR_INVALID = 1
DEVICE_KERNELS = {(0, 1, 0), (0, 4, 0), (0, 1, 1), (0, 4, 1), (0, 1, 2), (0, 4, 2), (1, 1, 0), (2, 4, 1)}     # (plan, rows, flavour) ksolve_test_fast_cold.hip compiles


def In(key, *values):
    return new_requirement(key, "In", None, *values)


def req(key, op, *values):
    return new_requirement(key, op, None, *values)


class Problem:
    """A catalogue, NodePool templates and pod classes as the definition reads them.
    types[i]: requirement set (with IT_KEY In [its name]); alloc / cap[r][i]; offers[i]: set of (zone index, capacity-type index) with
    an available offering; templates[t]: dict(reqs, its, taints, limits [n_res + 1], limit_mask); groups[t]: [(types, overhead [n_res])]
    for the templates in tmpl_ov; classes[c]: dict(reqs, requests [n_res], tolerates)."""

    def __init__(self, space, types, alloc, offers, templates, classes, n_zones, n_cts, cap=None, tmpl_ov=0, groups=None, plain=1, plain_nodes=0, plain_ops=0,
                 ops=0, lim=0, rows=1, plan=0, flavour=0, max_claims=64, claim_cap=0):
        self.space, self.types, self.offers, self.templates, self.classes = space, types, offers, templates, classes
        self.alloc = np.array(alloc, I64).reshape(-1, len(types))
        self.cap = self.alloc.copy() if cap is None else np.array(cap, I64).reshape(-1, len(types))
        self.n_res, self.n_its, self.n_zones, self.n_cts = self.alloc.shape[0], len(types), n_zones, n_cts
        self.tmpl_ov, self.groups = tmpl_ov, groups or [[] for _ in templates]
        self.plain, self.plain_nodes, self.plain_ops, self.ops, self.lim = plain, plain_nodes, plain_ops, ops, lim
        self.rows, self.plan, self.flavour, self.max_claims, self.claim_cap = rows, plan, flavour, max_claims, claim_cap
        self.podops = flavour == 2
        self.zones = space.values[ZONE][:n_zones] if ZONE in space.kidx else None
        self.cts = space.values[CT][:n_cts] if CT in space.kidx else None


# ------------------------------------------------------------------------------------------------ the definition
def eff(P, t, r, it):
    """allocatable less the overhead of the type's daemon-overhead group in template t (scheduler.go:963-1043): the group itself where
    the template has one, the first group that holds the type otherwise, K_EFF_NEVER where none does"""
    if not (P.tmpl_ov >> t) & 1:
        return int(P.alloc[r][it])
    gs = P.groups[t]
    g = gs[0] if len(gs) == 1 else next((g for g in gs if it in g[0]), None)
    return K_EFF_NEVER if g is None else int(P.alloc[r][it]) - g[1][r]


def admits(P, reqs, cell):
    """the zone x capacity-type cell holds a value the requirement set Has() on both keys (types.go:553-570)"""
    z, c = cell
    return (P.zones is None or ZONE not in reqs or has(reqs[ZONE], P.zones[z])) and (P.cts is None or CT not in reqs or has(reqs[CT], P.cts[c]))


def prefilter(P, t):
    T = P.templates[t]
    return {it for it in T["its"] if all(P.alloc[r][it] >= 0 for r in range(P.n_res)) and not bad_keys(P.types[it], T["reqs"])
            and any(admits(P, T["reqs"], cell) for cell in P.offers[it])}


def decline_reason(P):
    """setup()'s answer: 0 or the first reason of decline.h in the order setup() tests them"""
    sp, wk = P.space, P.space.well_known
    if not (P.plain or (P.ops and P.plain_ops)) or P.n_res > 4 or len(P.templates) > 32:
        return DECLINE_NOT_PLAIN
    if not P.ops and any(operator(r) != "In" or r.gte is not None or r.lte is not None for T in P.templates for r in T["reqs"].values()):
        return DECLINE_TEMPLATE_NOT_POSITIVE
    if not P.podops and any(r.complement for c in P.classes for r in c["reqs"].values()):
        return DECLINE_CLASS_NOT_POSITIVE
    if P.podops:
        kop = {o: {k for c in P.classes for k, r in c["reqs"].items() if operator(r) == o} for o in ("In", "NotIn", "Exists", "DoesNotExist")}
        t_undef = {k for k in sp.keys for T in P.templates if k not in T["reqs"]}
        t_notin = {k for T in P.templates for k, r in T["reqs"].items() if operator(r) == "NotIn"}
        t_bounds = {k for T in P.templates for k, r in T["reqs"].items() if r.gte is not None or r.lte is not None}
        if (kop["NotIn"] | kop["DoesNotExist"]) & (kop["In"] | kop["Exists"]) & t_undef - wk:
            return DECLINE_CLASS_KEY_DEFINEDNESS
        if kop["DoesNotExist"] & (kop["NotIn"] | t_notin):
            return DECLINE_CLASS_DNE_MIXED
        if kop["NotIn"] & t_bounds:
            return DECLINE_CLASS_NOTIN_BOUNDS
        if kop["Exists"] & t_undef & wk:
            return DECLINE_CLASS_EXISTS_UNDEFINED
    var = [k for k in sp.keys if any(k in c["reqs"] for c in P.classes)]
    if HOSTNAME in var or IT_KEY in var:
        return DECLINE_SELECTS_HOST_OR_TYPE
    bits = 0
    for j, k in enumerate(var):
        width = len(sp.values[k]) + (1 if P.podops else 0)
        if len(sp.values[k]) > 64 or j >= K_MAX_VAR or bits + width + 1 > K_VAR_BITS:
            return DECLINE_KEYS_DO_NOT_PACK
        bits += width + 1
    lim = 1 << 30
    if any(a >= lim or a <= -lim for a in P.alloc.ravel().tolist()):
        return DECLINE_QUANTITY_RANGE
    for t in range(len(P.templates)):
        if (P.tmpl_ov >> t) & 1 and any(not -lim < eff(P, t, r, it) < lim for r in range(P.n_res) for it in range(P.n_its)):
            return DECLINE_QUANTITY_RANGE
    if any(q >= lim or q < 0 for c in P.classes for q in c["requests"]):
        return DECLINE_QUANTITY_RANGE
    if not P.podops and any(not r.values for c in P.classes for r in c["reqs"].values()):
        return DECLINE_CLASS_EMPTY_IN
    return 0


class Definition:
    """What setup() leaves, and the functions of a requirement set; `decline` != 0: nothing else is defined."""

    def __init__(self, P):
        self.P = P
        self.decline = decline_reason(P)
        if self.decline:
            return
        sp = P.space
        self.var = [k for k in sp.keys if any(k in c["reqs"] for c in P.classes)]
        self.nv = len(self.var)
        self.width = [len(sp.values[k]) + (1 if P.podops else 0) for k in self.var]
        self.off = [sum(w + 1 for w in self.width[:j]) for j in range(self.nv)]
        self.fmask = [((1 << w) - 1) << o for w, o in zip(self.width, self.off)]
        self.vword = [int(sp.off[sp.kidx[k]]) for k in self.var]
        self.dne_vars = sum(1 << j for j, k in enumerate(self.var) if any(k in c["reqs"] and operator(c["reqs"][k]) == "DoesNotExist" for c in P.classes)) if P.podops else 0
        self.t_its = [prefilter(P, t) for t in range(len(P.templates))]
        self.active = sum(1 << t for t, s in enumerate(self.t_its) if s)
        self.tvmask = [self.pack_set(T["reqs"], t) for t, T in enumerate(P.templates)]
        self.tdef = [self.keybits(T["reqs"]) for T in P.templates]
        self.cls = [self.class_record(c) for c in P.classes]
        self.remaining = [list(T["limits"]) for T in P.templates]
        self.real = list(range(len(P.templates)))        # id -> template: a limit stage (Model.limit_stage) appends its own

    def keybits(self, reqs):
        return sum(1 << self.P.space.kidx[k] for k in reqs)

    def pack_set(self, reqs, top):
        """the packed word of a requirement set: per variable key the values it Has() (and the phantom bit for a complement set under
        pod operators), the guard bit where the set leaves the key undefined or — a template's own complement requirement, any
        complement or DoesNotExist under pod operators — holds no concrete In set; `top` in the top byte"""
        sp, vm = self.P.space, top << 56
        for j, k in enumerate(self.var):
            guard, ph = 1 << (self.off[j] + self.width[j]), 1 << (self.off[j] + self.width[j] - 1)
            if k not in reqs:
                vm |= self.fmask[j] | guard
                continue
            r = reqs[k]
            f = sum(1 << (self.off[j] + i) for i, v in enumerate(sp.values[k]) if has(r, v))
            if self.P.podops:
                if r.complement:
                    vm |= f | ph | guard
                else:
                    vm |= f if f else ph | guard          # In [] == DoesNotExist: the phantom bit alone
            else:
                vm |= f | (guard if r.complement else 0)
        return vm

    def class_record(self, c):
        P, sp = self.P, self.P.space
        size = [c["requests"][r] if r < P.n_res else 0 for r in range(4)]
        dmask = sum(self.fmask[j] for j, k in enumerate(self.var) if k in c["reqs"])
        ok = 0
        for t, T in enumerate(P.templates):
            if T["taints"] & ~c["tolerates"]:
                continue
            good = True
            for k, r in c["reqs"].items():
                o = operator(r) if P.podops else "In"
                if o in ("In", "Exists") and k not in T["reqs"] and k not in sp.well_known:       # requirements.go:185-193
                    good = False
                if k in T["reqs"] and o == "Exists" and operator(T["reqs"][k]) == "DoesNotExist":
                    good = False
                if k in T["reqs"] and o == "DoesNotExist" and not negative(T["reqs"][k]):
                    good = False
            ok |= good << t
        return dict(cvmask=self.pack_set(c["reqs"], 0xFF), dmask=dmask, size=size, tmplok=ok, kdef=self.keybits(c["reqs"]))

    # ---- functions of a requirement set: (template t, classes merged into it) ----
    def merged(self, t, classes=()):
        reqs = dict(self.P.templates[self.real[t]]["reqs"])
        for k in classes:
            add(reqs, *self.P.classes[k]["reqs"].values())       # Requirements.Add, requirements.go:133-140
        return reqs

    def compat_types(self, t, reqs):
        """the types of t's prefiltered list whose requirements Intersect the set (nodeclaim.go:620-622)"""
        return {it for it in self.t_its[t] if not bad_keys(self.P.types[it], reqs)}

    def cells(self, reqs):
        return {(z, c) for z in range(self.P.n_zones) for c in range(self.P.n_cts) if admits(self.P, reqs, (z, c))}

    def F(self, t, reqs):
        return {it for it in self.compat_types(t, reqs) if any(admits(self.P, reqs, cell) for cell in self.P.offers[it])}

    def front(self, t, F):
        """the distinct Pareto-maximal effective-allocatable vectors of F, descending"""
        vecs = {tuple(eff(self.P, self.real[t], r, it) for r in range(self.P.n_res)) for it in F}
        keep = [v for v in vecs if not any(u != v and all(a <= b for a, b in zip(v, u)) for u in vecs)]
        return sorted(keep, reverse=True)

    def fits(self, t, F, need):
        return any(all(eff(self.P, self.real[t], r, it) >= need[r] for r in range(self.P.n_res)) for it in F)

    def can_join(self, t, classes, k):
        """CanAdd's requirement half (nodeclaim.go:126-136) for a pod of class k on a claim of template t that holds `classes`"""
        c = self.P.classes[k]
        return not (self.P.templates[self.real[t]]["taints"] & ~c["tolerates"]) and compatible(self.merged(t, classes), c["reqs"], self.P.space.well_known) == COMPAT_OK


def fast_hash(vm):
    """the cache's first probe (fast_engine.h fast_hash: the halves folded with a rotation, one multiply, the top ten bits)"""
    lo, hi = vm & 0xFFFFFFFF, vm >> 32
    return (((lo ^ (((hi << 15) | (hi >> 17)) & 0xFFFFFFFF)) * 0x9E3779B1) & 0xFFFFFFFF) >> 22


class Cache:
    """the requirement-set cache as the definition keeps it: slot -> (vm, types, front, pool offset)"""

    def __init__(self):
        self.slots, self.n_pool, self.pool = {}, 0, []

    def find(self, vm):
        """(slot or -1, probes)"""
        h, probes = fast_hash(vm), 1
        while h in self.slots:
            if self.slots[h]["vm"] == vm:
                return h, probes
            h, probes = (h + 1) & (K_ENT - 1), probes + 1
        return -1, probes

    def create(self, vm, F, front):
        """create_entry's slot, or -1 with the state it leaves (vectors written before the refusal stay in the pool)"""
        if len(self.slots) >= K_GATE:
            return -1
        h = fast_hash(vm)
        while h in self.slots:
            h = (h + 1) & (K_ENT - 1)
        off = self.n_pool
        for i, v in enumerate(front[1:], 1):
            if i > K_EXTRA or self.n_pool >= K_POOL:
                return -1
            self.pool.append(v)
            self.n_pool += 1
        self.slots[h] = dict(vm=vm, F=F, front=front, off=off)
        return h


class Model:
    """The loop's cold state as the definition keeps it: the cache, the claims as (template, classes joined, requests) with their
    acceptance words, the class slots, the hostname numbers, the kept verdicts. No NodePool limits (tmpl_limit_mask 0)."""

    def __init__(self, D, cap):
        self.D, self.P, self.cap = D, D.P, cap
        self.cache, self.claims, self.acc, self.hostseq = Cache(), [], [], []
        self.scls = [[FREE] * 64 for _ in range(4)]
        self.host_seq, self.bail, self.epoch, self.us_cls, self.evicted, self.us = 0, 0, 1, {}, False, (0, 0)
        self.stale = set()                                 # slots dropped all at once that no class has taken again: their bits stay in the claims' words
        self.remaining = [list(r) for r in D.remaining]    # per NodePool: remaining[q] per resource, then the nodes (consulted, never counted down by the engine)
        self.cur, self.first_claim, self.limit_facts = list(range(32)), NO_CLAIM, []

    def viable(self, t, lm):
        """filterByRemainingResources (scheduler.go:1069-1085) over the template's prefiltered types"""
        return {it for it in self.D.t_its[t] if all(int(self.P.cap[q][it]) <= self.remaining[t][q] for q in range(self.P.n_res) if (lm >> q) & 1)}

    def limit_stage(self, t, lm):
        """the id a new claim of template t carries under its limits (scheduler.go:706-727): t or its current stage while the limits
        exclude nothing new; a new stage — the next free id below 32, its type list, the template's packed word under its own id, bit t
        of every class's tmplok copied to its bit — when they do; -1 skip the template (no node left, no type left), -2 no id left"""
        D, nr = self.D, self.P.n_res
        if (lm >> nr) & 1 and self.remaining[t][nr] <= 0:
            return -1
        L = self.viable(t, lm)
        differs = L != D.t_its[self.cur[t]]
        if differs and self.first_claim == NO_CLAIM:
            self.first_claim = len(self.claims)
        if not L:
            return -1
        if not differs:
            return self.cur[t]
        s = len(D.real)
        if s >= 32:
            return -2
        D.real.append(t), D.t_its.append(L), D.tvmask.append((D.tvmask[t] & ~(0xFF << 56)) | (s << 56)), D.tdef.append(D.tdef[t])
        self.cur[t] = s
        for c in D.cls:
            c["tmplok"] |= ((c["tmplok"] >> t) & 1) << s
        self.limit_facts.append(("stage", t, len(self.claims)))
        return s

    def subtract_max(self, t, lm, F, size):
        """subtractMax (scheduler.go:1049-1066) over the new claim's instance types: F cut to the types that hold the pod"""
        P = self.P
        fit = [it for it in F if all(eff(P, t, r, it) >= size[r] for r in range(P.n_res))]
        for q in range(P.n_res):
            if (lm >> q) & 1:
                self.remaining[t][q] -= max(int(P.cap[q][it]) for it in fit)

    def entry(self, t, chain):
        """the cache entry of the set, created when it is met for the first time; None: no room"""
        reqs = self.D.merged(t, chain)
        vm = self.D.pack_set(reqs, t)
        slot, _ = self.cache.find(vm)
        if slot < 0:
            F = self.D.F(t, reqs)
            slot = self.cache.create(vm, F, self.D.front(t, F))
        return self.cache.slots[slot] if slot >= 0 else None

    def can_add(self, claim, k, cached=True):
        """CanAdd (nodeclaim.go:124-242) of a pod of class k on the claim; None: the cache has no room for the set"""
        t, chain, have = claim
        if not self.D.can_join(t, chain, k):
            return False
        need = [have[r] + self.P.classes[k]["requests"][r] for r in range(self.P.n_res)]
        if not cached:
            return self.D.fits(t, self.D.F(t, self.D.merged(t, chain + (k,))), need)
        e = self.entry(t, chain + (k,))
        return None if e is None else self.D.fits(t, e["F"], need)

    def row(self, claim, j):
        word = 0
        for l in range(64):
            if self.scls[j][l] != FREE:
                a = self.can_add(claim, self.scls[j][l])
                if a is None:
                    self.bail = DECLINE_CACHE_FULL
                    return None
                word |= a << l
        return word

    def rows(self, x):
        """every acceptance word of claim x, row by row; False: the cache had no room (the rows before that one are written)"""
        for j in range(self.P.rows):
            w = self.row(self.claims[x], j)
            if w is None:
                return False
            self.acc[x][j] = w
        return True

    def diag(self, t, chain, size):
        """InstanceTypeFilterError's flags (nodeclaim.go:585-592) over the id's type list"""
        reqs, P = self.D.merged(t, chain), self.P
        flags = 0
        for it in self.D.t_its[t]:
            cm = not bad_keys(P.types[it], reqs)
            off = any(admits(P, reqs, cell) for cell in P.offers[it])
            fit = off and all(eff(P, self.D.real[t], r, it) >= size[r] for r in range(P.n_res))       # (fits() reports itFits only with a compatible offering)
            flags |= (1 if cm else 0) | (2 if fit else 0) | (4 if off else 0) | (16 if cm and off and not fit else 0) | (32 if fit and not cm else 0)
        return flags

    def new_claim(self, k, retry):
        """addToNewNodeClaim (scheduler.go:695-790): 1 created, 2 no template takes the pod (keep flavours: self.us = error, flags), 0 stop (self.bail)"""
        P, D, keep = self.P, self.D, self.P.flavour >= 1
        c = P.classes[k]
        size = D.cls[k]["size"]
        if keep and not D.active:
            self.us = (E_NO_TEMPLATES, 0)
            return 2
        if keep and k in self.us_cls and self.us_cls[k][3] != self.epoch:
            self.limit_facts.append(("verdict invalidated", k, len(self.claims)))
        if keep and k in self.us_cls and self.us_cls[k][3] == self.epoch:
            self.limit_facts.append(("verdict reused", k, len(self.claims)))
            err, flags, tried, _ = self.us_cls[k]
            self.host_seq += tried
            self.us = (err, flags)
            return 2
        seq0, first, first_flags = self.host_seq, 0, 0
        for t, T in enumerate(P.templates):
            if not (D.active >> t) & 1:
                continue
            lm, ts = T["limit_mask"], t
            if lm and P.lim:
                ts = self.limit_stage(t, lm)
                if ts == -1:
                    first = first or E_LIMITS         # the reference returns before NewNodeClaim: no hostname number
                    self.limit_facts.append(("skipped", t, len(self.claims)))
                    continue
                if ts == -2:
                    self.bail = DECLINE_LIMIT_STAGES
                    return 0
            elif lm:                                  # without limit stages the engine goes on only while the limits exclude nothing
                if (lm >> P.n_res) & 1 and self.remaining[t][P.n_res] <= 0:
                    self.bail = DECLINE_LIMIT_NODES
                    return 0
                if self.viable(t, lm) != D.t_its[t]:
                    self.bail = DECLINE_LIMIT_EXCLUDES_TYPE
                    return 0
            self.host_seq += 1
            if T["taints"] & ~c["tolerates"]:
                first = first or (E_TAINTS if keep else 0)
                continue
            if not D.can_join(t, (), k):
                first = first or (E_INCOMPATIBLE if keep or (D.cls[k]["tmplok"] >> t) & 1 else 0)
                continue
            t_, t = t, ts                             # from here on the claim's requirement set carries the id
            e = self.entry(t, (k,))
            if e is None:
                self.bail = DECLINE_CACHE_FULL_NEW_CLAIM
                return 0
            if not D.fits(t, e["F"], size):
                if keep and not first:
                    first, first_flags = E_INSTANCE_TYPES, self.diag(t, (k,), size)
                continue
            if retry:
                self.bail = DECLINE_UNSCHEDULABLE_POD
                return 0
            if len(self.claims) >= P.max_claims or len(self.claims) >= self.cap:
                self.bail = DECLINE_KERNEL_CAPACITY if len(self.claims) >= P.max_claims else DECLINE_CLAIM_SLOTS
                return 0
            claim = (t, (k,), list(size))
            self.claims.append(claim), self.hostseq.append(self.host_seq), self.acc.append([0] * P.rows)
            if not self.rows(len(self.claims) - 1):
                return 0
            if lm:
                self.subtract_max(t_, lm, e["F"], size)
                self.epoch += 1 if keep else 0        # the limits moved: no kept verdict stands
            return 1
        if not keep:
            self.bail = DECLINE_UNSCHEDULABLE_POD
            return 0
        self.us = (first or E_NO_TEMPLATES, first_flags)
        self.us_cls[k] = (self.us[0], self.us[1], self.host_seq - seq0, self.epoch)
        return 2

    def add(self, x, k):
        t, chain, have = self.claims[x]
        self.claims[x] = (t, chain + (k,), [a + b for a, b in zip(have, self.D.cls[k]["size"])])
        return 0 if self.rows(x) else -1

    def friends(self, a, b):
        """two classes that could share a NodeClaim: a template both take, a common value on every key both select on"""
        ra, rb = self.P.classes[a]["reqs"], self.P.classes[b]["reqs"]
        return bool(self.D.cls[a]["tmplok"] & self.D.cls[b]["tmplok"]) and all(not bad_keys({key: ra[key]}, {key: rb[key]}) for key in ra if key in rb)

    def new_slot(self, k):
        R = self.P.rows
        pref, best = 0, -1
        if R > 1:
            for j in range(R):
                used = [c for c in self.scls[j] if c != FREE]
                if len(used) == 64:
                    continue
                score = 128 * sum(self.friends(c, k) for c in used) + 64 - len(used)
                if score > best:
                    best, pref = score, j
        slot = next((64 * j + self.scls[j].index(FREE) for j in [(jj + pref) % R for jj in range(R)] if FREE in self.scls[j]), -1)
        evicted = 0
        if slot < 0:
            self.stale |= {(j, l) for j in range(R) for l in range(64)}
            self.scls = [[FREE] * 64 for _ in range(4)]
            slot, evicted, self.evicted = 0, 1 << 16, True
        row, sl = slot >> 6, slot & 63
        self.scls[row][sl] = k
        self.stale.discard((row, sl))
        for x0 in range(0, len(self.claims), 64):          # (64 claims at a time: their words are written when all 64 verdicts stand)
            verdicts = []
            for claim in self.claims[x0:x0 + 64]:
                a = self.can_add(claim, k)
                if a is None:
                    self.bail = DECLINE_CACHE_FULL
                    return -1
                verdicts.append(a)
            for x, a in enumerate(verdicts, x0):
                self.acc[x][row] = (self.acc[x][row] & ~(1 << sl)) | (a << sl)
        return slot | evicted

    def check_words(self):
        """bit s of row j of every claim's word == CanAdd(claim, class in slot 64 j + s), straight from the definition; free slots read 0,
        but for the slots that were dropped all at once and that no class has taken again (self.stale): a claim that was there at the
        drop keeps the bit it had — which mismatches() compares with the device's, bit for bit — and a claim created since reads 0"""
        for x, claim in enumerate(self.claims):
            for j in range(self.P.rows):
                for l in range(64):
                    k, bit = self.scls[j][l], (self.acc[x][j] >> l) & 1
                    if k != FREE:
                        assert bit == self.can_add(claim, k, cached=False), (x, j, l)
                    elif (j, l) not in self.stale:
                        assert bit == 0, (x, j, l)


def expected(P, script):
    """The definition's answer to run(P, script): dict of the fields mismatches() compares. script: list of
    ("ENTRY", t, classes) | ("FITS", t, classes, k, req[4]) | ("CELLS", t, classes) | ("COMPAT", t, classes) — the requirement set of
    template t with the classes merged; FITS: a pod of class k against the claim (t, classes) with requests req."""
    D = Definition(P)
    out = dict(setup_ret=D.decline, D=D)
    if D.decline:
        return out
    M = Model(D, P.claim_cap or 1 << 30)
    cache, res, facts = M.cache, [], []
    iw = (P.n_its + 63) // 64
    for op in script:
        kind = op[0]
        if kind in ("SLOT", "NEWCLAIM", "ADD"):
            if kind == "SLOT":
                r = dict(ret=M.new_slot(op[1]))
            elif kind == "NEWCLAIM":
                r = dict(ret=M.new_claim(op[1], bool(op[2])))
                r["aux"] = M.us[0] | (M.us[1] << 8) if r["ret"] == 2 else 0
                facts.append(("new_claim", r["ret"], M.us if r["ret"] == 2 else M.bail))
            else:
                r = dict(ret=M.add(op[1], op[2]))
            r["bail"] = M.bail
            res.append(r)
            if M.bail or r["ret"] < 0:
                break                    # (the engine stops: the words of the claim it was at are whatever it had written)
            M.check_words()
            continue
        t, classes = op[1], tuple(op[2])
        reqs = D.merged(t, classes)
        vm = D.pack_set(reqs, t)
        if kind == "ENTRY":
            F = D.F(t, reqs)
            front = D.front(t, F)
            slot = cache.create(vm, F, front)
            res.append(dict(ret=slot))
            facts.append(("front", min(len(front), 18), "refused" if slot < 0 else "ok"))
            if slot < 0:
                break
        elif kind == "FITS":
            k, have = op[3], op[4]
            c = P.classes[k]
            joined = D.merged(t, classes + (k,))
            m = vm & D.cls[k]["cvmask"]                       # what the loop looks up: the claim's word ANDed with the class's
            slot, probes = cache.find(m)
            need = [have[r] + c["requests"][r] for r in range(P.n_res)]
            ok = D.can_join(t, classes, k)
            fit = slot >= 0 and D.fits(t, cache.slots[slot]["F"], need)
            if ok:
                assert m == D.pack_set(joined, t), "the AND of two packed words is not the packed word of the merged set"
            res.append(dict(ret=slot, fits=int(fit), joins=int(ok), m=m, dmask=D.cls[k]["dmask"], tmplok=(D.cls[k]["tmplok"] >> t) & 1))
            facts.append(("lookup", "miss" if slot < 0 else "first" if probes == 1 else "later", int(fit)))
        elif kind == "CELLS":
            res.append(dict(cells=sum(1 << (z * 4 + c) for z, c in D.cells(reqs))))
        elif kind == "COMPAT":
            res.append(dict(compat=set_words(D.compat_types(t, reqs), iw)))
        elif kind == "DIAG":
            flags = M.diag(t, classes, op[3])
            res.append(dict(ret=flags))
            facts.append(("diag", flags))
        else:
            raise ValueError(kind)
    out.update(res=res, facts=facts, cache=cache, n_ent=len(cache.slots), n_pool=cache.n_pool, M=M)
    return out


def set_words(s, iw):
    return np.frombuffer(sum(1 << i for i in s).to_bytes(iw * 8, "little"), U64).copy()


# ------------------------------------------------------------------------------------------------ the entry point
class _Op(ctypes.Structure):
    _fields_ = [("op", ctypes.c_uint32), ("k", ctypes.c_int32), ("x", ctypes.c_int32), ("retry", ctypes.c_int32), ("vm", ctypes.c_uint64), ("dmask", ctypes.c_uint64),
                ("req", ctypes.c_int32 * 4), ("size", ctypes.c_int32 * 4)]


class _Res(ctypes.Structure):
    _fields_ = [("ran", ctypes.c_int32), ("ret", ctypes.c_int32), ("bail", ctypes.c_int32), ("pad", ctypes.c_int32), ("aux", ctypes.c_uint64)]


class _Scal(ctypes.Structure):
    _fields_ = [(f, ctypes.c_int32) for f in ("setup_ret", "nv", "n_ent", "n_pool", "n_claims", "bail_code")] + \
               [(f, ctypes.c_uint32) for f in ("active_templates", "host_seq", "po_on", "dne_vars", "us_epoch")] + [("ops_run", ctypes.c_int32)]


class _Var(ctypes.Structure):
    _fields_ = [("nv", ctypes.c_int32), ("vkey", ctypes.c_uint8 * 12), ("voff", ctypes.c_uint8 * 12), ("vwidth", ctypes.c_uint8 * 12), ("vword", ctypes.c_uint16 * 12)]


class _Misc(ctypes.Structure):
    _fields_ = [("tvmask", ctypes.c_uint64 * 32), ("tdef", ctypes.c_uint32 * 32), ("fmask", ctypes.c_uint64 * 12), ("vkey", ctypes.c_uint8 * 12), ("voff", ctypes.c_uint8 * 12),
                ("vwidth", ctypes.c_uint8 * 12), ("vword", ctypes.c_uint16 * 12), ("its", ctypes.c_uint64 * 32), ("rem", ctypes.c_uint64 * 32), ("cand", ctypes.c_uint64 * 32),
                ("acc", ctypes.c_uint64 * 4)]


class _PodOps(ctypes.Structure):
    _fields_ = [("on", ctypes.c_uint32), ("dne", ctypes.c_uint32)]


class _Limits(ctypes.Structure):
    _fields_ = [("real", ctypes.c_uint8 * 32), ("cur", ctypes.c_uint8 * 32), ("n_ids", ctypes.c_uint32), ("first_claim", ctypes.c_uint32)]


_P, _U, _I = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int32


class _In(ctypes.Structure):
    _fields_ = [("n_keys", _U), ("key_word_off", _P), ("value_int", _P), ("value_is_int", _P), ("value_valid", _P), ("key_zone", _I), ("key_ct", _I), ("key_it", _I),
                ("key_hostname", _I), ("well_known_mask", _U), ("n_its", _U), ("n_res", _U), ("n_zones", _U), ("n_cts", _U), ("plain", _U), ("plain_nodes", _U), ("plain_ops", _U),
                ("it_reqs", ctypes.POINTER(_ReqSets)), ("it_alloc", _P), ("it_cap", _P), ("it_off_avail", _P), ("n_templates", _U), ("tmpl_reqs", ctypes.POINTER(_ReqSets)),
                ("tmpl_its", _P), ("tmpl_taints", _P), ("tmpl_limits", _P), ("tmpl_limit_mask", _P), ("tmpl_ov", _U), ("dg_first", _P), ("dg_ov", _P), ("dg_its", _P),
                ("n_classes", _U), ("cls_reqs", ctypes.POINTER(_ReqSets)), ("cls_requests", _P), ("cls_tolerates", _P), ("ops", _U), ("lim", _U), ("rows", _U), ("plan", _U),
                ("flavour", _U), ("max_claims", _U), ("cap", _U), ("n_ops", _U), ("script", _P)]


_OUT_TABLES = ("scal", "misc", "var", "podops", "lim", "cls", "t_its", "t_remaining", "it_eff", "ent", "pool", "ent_its", "rec", "c_hostseq", "aslot", "scls", "cur", "us_cls",
               "res", "compat")


class _Out(ctypes.Structure):
    _fields_ = [("kernel", _U), ("it_words", _U), ("misc_words", _U), ("cap", _U), ("t_rows", _U)] + [(f, _P) for f in _OUT_TABLES]


assert ctypes.sizeof(_Op) == 64 and ctypes.sizeof(_Res) == 24 and ctypes.sizeof(_Scal) == 48 and ctypes.sizeof(_Var) == 64 and ctypes.sizeof(_Misc) == 1344

_libs = {}


def _lib(path):
    if path not in _libs:
        lib = ctypes.CDLL(os.path.abspath(path))
        lib.ksolve_test_fast_cold.restype = ctypes.c_int
        lib.ksolve_test_fast_cold.argtypes = [ctypes.POINTER(_In), ctypes.POINTER(_Out)]
        _libs[path] = lib
    return _libs[path]


def run(lib_path, P, script, want=None, edit=None):
    """ksolve_test_fast_cold on P and the script: dict with status and, when it is 0, everything downloaded. The packed words the
    operations take come from the definition (`want`, expected(P, script)): the kernel's own setup() must agree on them, and
    mismatches() says so before anything else."""
    want = want or expected(P, script)
    sp, n_its, nr, T, nc = P.space, P.n_its, P.n_res, len(P.templates), len(P.classes)
    iw = (n_its + 63) // 64
    keep = []
    arr = lambda a, dt: keep.append(np.ascontiguousarray(a, dt)) or keep[-1].ctypes.data
    sets = [_reqsets(encode_sets(sp, rows), len(rows), keep) for rows in (P.types, [t["reqs"] for t in P.templates], [c["reqs"] for c in P.classes])]
    avail = [sum(1 << (z * 4 + c) for z, c in o) for o in P.offers]
    ops = (_Op * max(1, len(script)))()
    if not want["setup_ret"]:
        for o, op, w in zip(ops, script, want["res"] + [None] * len(script)):
            D = want["D"]
            o.op = {"ENTRY": OP_ENTRY, "FITS": OP_FITS, "CELLS": OP_CELLS, "COMPAT": OP_COMPAT, "DIAG": OP_DIAG, "SLOT": OP_SLOT, "NEWCLAIM": OP_NEWCLAIM, "ADD": OP_ADD}[op[0]]
            if op[0] == "SLOT":
                o.k = op[1]
                continue
            if op[0] == "NEWCLAIM":
                o.k, o.retry = op[1], op[2]
                continue
            if op[0] == "ADD":
                o.x, o.k = op[1], op[2]
                continue
            o.vm = D.pack_set(D.merged(op[1], tuple(op[2])), op[1])
            if op[0] == "DIAG":
                o.size[:] = list(op[3]) + [0] * (4 - len(op[3]))
            if op[0] == "FITS":
                o.vm &= D.cls[op[3]]["cvmask"]
                o.dmask = D.cls[op[3]]["dmask"]
                o.req[:] = list(op[4]) + [0] * (4 - len(op[4]))
                o.size[:] = D.cls[op[3]]["size"]
    else:
        for o, op in zip(ops, script):        # (setup() declines: the operations never run, whatever they hold)
            o.op, o.vm = OP_CELLS, 0
    n_dg, first, ov, gits = 0, [0], [], []
    for t in range(T):
        for members, over in (P.groups[t] if (P.tmpl_ov >> t) & 1 else [(set(range(n_its)), [0] * nr)]):
            ov.append(over), gits.append(set_words(members, iw))
        first.append(len(ov))
    fill = lambda shape, dt: np.frombuffer(b"\xA5" * (int(np.prod(shape)) * np.dtype(dt).itemsize), dt).reshape(shape).copy()
    rows = P.rows
    t_rows = max(32, T) if P.lim else T
    buf = dict(scal=(_Scal * 2)(), misc=fill((2, 168), U64), var=_Var(), podops=_PodOps(), lim=_Limits(), cls=fill((nc, 5), U64), t_its=fill((t_rows, iw), U64),
               t_remaining=fill((T, nr + 1), I64), it_eff=fill((T, nr, n_its), I64), ent=fill((K_ENT, 4), U64), pool=fill((K_POOL, 4), I32), ent_its=fill((K_ENT, iw), U64),
               rec=fill((P.max_claims, 3 + rows), U64), c_hostseq=fill(P.max_claims, U32), aslot=fill((64 * rows, 5), U64), scls=fill((4, 64), U32), cur=fill((4, 64), U32),
               us_cls=fill(nc, U64), res=(_Res * max(1, len(script)))(), compat=fill((max(1, len(script)), iw), U64))
    for f in ("scal", "var", "podops", "lim", "res"):
        ctypes.memset(ctypes.addressof(buf[f]), 0xA5, ctypes.sizeof(buf[f]))
    ptr = lambda v: v.ctypes.data if isinstance(v, np.ndarray) else ctypes.addressof(v)
    out = _Out(0, 0, 0, 0, 0, *[ptr(buf[f]) for f in _OUT_TABLES])
    key = lambda name: sp.kidx.get(name, -1)
    arg = _In(sp.nk, sp.off.ctypes.data, sp.value_int.ctypes.data, sp.value_is_int.ctypes.data, sp.value_valid.ctypes.data, key(ZONE), key(CT), key(IT_KEY), key(HOSTNAME),
              sp.well_known_mask, n_its, nr, P.n_zones, P.n_cts, P.plain, P.plain_nodes, P.plain_ops, ctypes.pointer(sets[0]), arr(P.alloc, I64), arr(P.cap, I64), arr(avail, U64),
              T, ctypes.pointer(sets[1]), arr([set_words(t["its"], iw) for t in P.templates], U64), arr([t["taints"] for t in P.templates], U64),
              arr([t["limits"] for t in P.templates], I64), arr([t["limit_mask"] for t in P.templates], U32), P.tmpl_ov, arr(first, I32), arr(ov, I64), arr(gits, U64),
              nc, ctypes.pointer(sets[2]), arr([c["requests"] for c in P.classes], I64), arr([c["tolerates"] for c in P.classes], U64), P.ops, P.lim, rows, P.plan, P.flavour,
              P.max_claims, P.claim_cap, len(script), ctypes.addressof(ops))
    if edit:
        edit(arg, ops)            # (tests of the hook's own checks: an index out of range)
    st = _lib(lib_path).ksolve_test_fast_cold(ctypes.byref(arg), ctypes.byref(out))
    buf.update(status=st, kernel=out.kernel, it_words=out.it_words, cap=out.cap, misc=[_Misc.from_buffer_copy(buf["misc"][i].tobytes()) for i in range(2)])
    return buf


def kernel_id(P, emulation):
    return (1000 if emulation else 0) + P.flavour * 100 + P.plan * 10 + P.rows


# ------------------------------------------------------------------------------------------------ the comparison
def mismatches(got, want, P, script, limit=12):
    """every field of the download that differs from the definition's answer, as (field, index, got, want)"""
    bad = []

    def eq(name, g, w, idx=None):
        if (np.asarray(g) != np.asarray(w)).any() if isinstance(g, np.ndarray) or isinstance(w, np.ndarray) else g != w:
            bad.append((name, idx, g, w))

    if got["status"] != 0:
        return [("status", None, got["status"], 0)]
    s0, s1 = got["scal"][0], got["scal"][1]
    eq("setup_ret", s0.setup_ret, want["setup_ret"])
    eq("setup_ret behind the script", s1.setup_ret, want["setup_ret"])
    if want["setup_ret"]:
        eq("ops_run", s1.ops_run, 0)
        return bad[:limit]
    D = want["D"]
    T, nc, nr, iw = len(P.templates), len(P.classes), P.n_res, (P.n_its + 63) // 64
    Mo = want["M"]
    for s, (n_claims, host_seq, bail) in ((s0, (0, 0, 0)), (s1, (len(Mo.claims), Mo.host_seq, Mo.bail))):
        eq("nv", s.nv, D.nv), eq("active_templates", s.active_templates, D.active), eq("bail_code", s.bail_code, bail), eq("n_claims", s.n_claims, n_claims), eq("host_seq", s.host_seq, host_seq)
        if P.flavour >= 1:
            eq("us_epoch", s.us_epoch, 1 if s is s0 else Mo.epoch)
        if P.flavour == 2:
            eq("po_on", s.po_on, 1), eq("dne_vars", s.dne_vars, D.dne_vars)
    eq("n_ent behind setup", s0.n_ent, 0), eq("n_pool behind setup", s0.n_pool, 0)
    for i, M in enumerate(got["misc"]):
        for t in range(T if i == 0 else len(D.real)):
            eq(f"misc[{i}].tvmask", M.tvmask[t], D.tvmask[t], t), eq(f"misc[{i}].tdef", M.tdef[t], D.tdef[t], t)
        for j in range(D.nv):
            eq(f"misc[{i}].fmask", M.fmask[j], D.fmask[j], j), eq(f"misc[{i}].vkey", M.vkey[j], P.space.kidx[D.var[j]], j), eq(f"misc[{i}].voff", M.voff[j], D.off[j], j)
            eq(f"misc[{i}].vwidth", M.vwidth[j], D.width[j], j), eq(f"misc[{i}].vword", M.vword[j], D.vword[j], j)
    V = got["var"]
    eq("var.nv", V.nv, D.nv)
    for j in range(D.nv):
        eq("var", (V.vkey[j], V.voff[j], V.vwidth[j], V.vword[j]), (P.space.kidx[D.var[j]], D.off[j], D.width[j], D.vword[j]), j)
    if P.flavour == 2:
        eq("podops", (got["podops"].on, got["podops"].dne), (1, D.dne_vars))
    if P.lim:
        L = got["lim"]
        eq("lim.real", list(L.real), D.real + list(range(len(D.real), 32))), eq("lim.cur", list(L.cur), Mo.cur), eq("lim", (L.n_ids, L.first_claim), (len(D.real), Mo.first_claim))
    for c in range(nc):
        w, g = D.cls[c], got["cls"][c]
        eq("cls.cvmask", int(g[0]), w["cvmask"], c), eq("cls.dmask", int(g[1]), w["dmask"], c)
        eq("cls.size", [int(x) for x in g[2:4].view(I32)], w["size"], c)
        eq("cls.tmplok", int(g[4]) & 0xFFFFFFFF, w["tmplok"], c), eq("cls.kdef", int(g[4]) >> 32, w["kdef"], c)
    for t in range(T):
        eq("t_its", got["t_its"][t], set_words(D.t_its[t], iw), t)
        eq("t_remaining", got["t_remaining"][t].tolist(), Mo.remaining[t], t)
        if (P.tmpl_ov >> t) & 1:
            eq("it_eff", got["it_eff"][t].tolist(), [[eff(P, t, r, it) for it in range(P.n_its)] for r in range(nr)], t)
    if P.lim:
        for t in range(T, len(D.real)):
            eq("t_its of a limit stage", got["t_its"][t], set_words(D.t_its[t], iw), t)
        eq("t_its rows of the free ids", int(got["t_its"][len(D.real):].any()), 0)
    if P.flavour >= 1:
        eq("us_cls", got["us_cls"].tolist(), [(lambda v: v[0] | v[1] << 8 | v[2] << 16 | v[3] << 32)(Mo.us_cls[k]) if k in Mo.us_cls else 0 for k in range(nc)])
    eq("c_hostseq", got["c_hostseq"][:len(Mo.claims)].tolist(), Mo.hostseq)
    for x, (t, chain, have) in enumerate(Mo.claims):
        g = got["rec"][x]
        eq("claim.vmask", int(g[0]), D.pack_set(D.merged(t, chain), t), x), eq("claim.req", [int(v) for v in g[1:3].view(I32)], have, x)
        eq("claim.acc", [int(v) for v in g[3:]], Mo.acc[x], x)
    eq("scls", got["scls"].tolist(), Mo.scls), eq("cur", int(got["cur"].any()), 0)
    for j in range(P.rows):
        for l in range(64):
            if Mo.scls[j][l] != FREE:
                w, g = D.cls[Mo.scls[j][l]], got["aslot"][64 * j + l]
                eq("aslot", (int(g[0]), int(g[1]), [int(v) for v in g[2:4].view(I32)], int(g[4]) & 0xFFFFFFFF, int(g[4]) >> 32), (w["cvmask"], w["dmask"], w["size"], w["tmplok"], w["kdef"]), (j, l))
    # the script
    res, cache = want["res"], want["cache"]
    eq("ops_run", s1.ops_run, len(res))
    for i, (op, w) in enumerate(zip(script, res)):
        g = got["res"][i]
        eq("res.ran", g.ran, 1, i), eq("res.bail", g.bail, w.get("bail", 0), i)
        if op[0] in ("SLOT", "NEWCLAIM", "ADD", "DIAG"):
            eq(op[0], g.ret, w["ret"], i)
            if op[0] == "NEWCLAIM" and P.flavour >= 1:
                eq("us_err_ | us_diag_ << 8", g.aux, w["aux"], i)
        elif op[0] == "ENTRY":
            eq("create_entry", g.ret, w["ret"], i)
        elif op[0] == "FITS":
            eq("fast_lookup", g.ret, w["ret"], i), eq("fast_fits", g.aux & 1, w["fits"], i)
            eq("tmplok and fast_fields_ok", w["tmplok"] & (g.aux >> 1) & 1, w["joins"], i)
        elif op[0] == "CELLS":
            eq("offering_cells", g.aux, w["cells"], i)
        elif op[0] == "COMPAT":
            eq("compat_word", got["compat"][i], w["compat"], i)
    for i in range(len(res), len(script)):
        eq("res.ran of an operation behind the script's end", got["res"][i].ran & 0xFFFFFFFF, 0xA5A5A5A5, i)
    eq("n_ent", s1.n_ent, want["n_ent"]), eq("n_pool", s1.n_pool, want["n_pool"])
    for h in range(K_ENT):
        e, info = got["ent"][h], int(got["ent"][h][3]) & 0xFFFFFFFF
        if h not in cache.slots:
            eq("ent.info bit 0 of a free slot", info & 1, 0, h)
            continue
        s = cache.slots[h]
        first = list(s["front"][0]) + [UNUSED_CAP] * (4 - nr) if s["front"] else [-1] * 4        # (an empty F: no vector, capacities -1)
        extra = max(0, len(s["front"]) - 1)
        eq("ent.vmask", int(e[0]), s["vm"] | (EXT_BIT if extra else 0), h), eq("ent.cap", [int(x) for x in e[1:3].view(I32)], first, h)
        eq("ent.info", info, 1 | (extra << 8) | (s["off"] << 16), h), eq("ent.pad", int(e[3]) >> 32, 0, h)
        eq("ent_its", got["ent_its"][h], set_words(s["F"], iw), h)
        for x, v in enumerate(s["front"][1:]):
            eq("pool", got["pool"][s["off"] + x].tolist(), list(v) + [UNUSED_CAP] * (4 - nr), (h, x))
    return bad[:limit]


FIELDS_BIT_FOR_BIT = ("scal", "var", "podops", "lim", "cls", "t_its", "t_remaining", "ent_its", "res", "compat", "c_hostseq", "us_cls", "scls", "cur", "rec")


def device_differs(dev, emu, P):
    """the fields in which two downloads differ, over everything the definition specifies (the emulation's kernel id aside)"""
    bad = []
    raw = lambda v: v.tobytes() if isinstance(v, np.ndarray) else bytes(v)
    for f in FIELDS_BIT_FOR_BIT:
        if f in ("var", "scal") or (f == "podops" and P.flavour != 2) or (f == "lim" and not P.lim):
            continue
        if raw(dev[f]) != raw(emu[f]):
            bad.append(f)
    # (the emulation's FastCold carries the set-aside list's and the pod operators' state whatever the flavour: compared where the flavour has it)
    names = [f for f, _ in _Scal._fields_ if not (f == "us_epoch" and P.flavour < 1) and not (f in ("po_on", "dne_vars") and P.flavour < 2)]
    for i in range(2):
        if [getattr(dev["scal"][i], f) for f in names] != [getattr(emu["scal"][i], f) for f in names]:
            bad.append(("scal", i))
    if dev["var"].nv != emu["var"].nv or any(bytes(dev["var"])[4 + 12 * a + j] != bytes(emu["var"])[4 + 12 * a + j] for a in range(3) for j in range(dev["var"].nv)):
        bad.append("var")
    if dev["scal"][0].setup_ret:
        return bad
    n_pool = dev["scal"][1].n_pool
    if raw(dev["pool"][:n_pool]) != raw(emu["pool"][:n_pool]):
        bad.append("pool")
    for h in range(K_ENT):
        valid = int(dev["ent"][h][3]) & 1
        if valid != int(emu["ent"][h][3]) & 1 or (valid and raw(dev["ent"][h]) != raw(emu["ent"][h])):
            bad.append(("ent", h))
    for i in range(2):
        a, b = dev["misc"][i], emu["misc"][i]
        if list(a.tvmask)[:len(P.templates)] != list(b.tvmask)[:len(P.templates)] or list(a.tdef)[:len(P.templates)] != list(b.tdef)[:len(P.templates)]:
            bad.append(("misc", i))
    return bad


# ------------------------------------------------------------------------------------------------ the cases
ARCH, TEAM, TIER = "kubernetes.io/arch", "example.com/team", "example.com/tier"
TEAMS, TIERS = ["a", "b", "c", "d", "e"], ["gold", "silver", "bronze", "tin"]


def make_space(n_its, n_zones=3, n_cts=2, teams=TEAMS, extra=()):
    """well-known keys around the instance-type key (its dictionary is the type list), two custom keys, the hostname"""
    keys = [(ARCH, ["amd64", "arm64"]), (TEAM, list(teams)), (ZONE, [f"zone-{i}" for i in range(n_zones)]), (IT_KEY, [f"type-{i}" for i in range(n_its)]),
            (CT, ["on-demand", "spot", "reserved", "burst"][:n_cts]), (TIER, TIERS), (HOSTNAME, ["host-0"])] + list(extra)
    return Space(keys, well_known=[ARCH, ZONE, IT_KEY, CT, HOSTNAME], key_it=IT_KEY)


def some(rng, vals, lo=1, hi=None):
    return rng.sample(vals, rng.randint(lo, min(hi or len(vals), len(vals))))


def gen_type(rng, sp, i, n_zones, n_cts, operators=True):
    offers = {(z, c) for z in range(n_zones) for c in range(n_cts) if rng.random() < 0.5} or {(rng.randrange(n_zones), rng.randrange(n_cts))}
    t = {IT_KEY: In(IT_KEY, f"type-{i}"), ARCH: In(ARCH, rng.choice(sp.values[ARCH])),
         ZONE: In(ZONE, *{sp.values[ZONE][z] for z, _ in offers}), CT: In(CT, *{sp.values[CT][c] for _, c in offers})}
    for key in (TEAM, TIER):
        how = rng.choice(["undefined", "In", "In", "In", "NotIn", "Exists", "DoesNotExist"] if operators else ["undefined", "In", "In"])
        if how in ("In", "NotIn"):
            t[key] = req(key, how, *some(rng, sp.values[key], 1, 3))
        elif how != "undefined":
            t[key] = req(key, how)
    return t, offers


def gen_problem(seed, n_its=20, n_res=2, n_templates=3, n_classes=6, n_zones=3, n_cts=2, ops=0, flavour=0, rows=1, plan=0, overhead=False, lim=0, special=(), big=1000):
    """a random catalogue, templates and classes of the engine's shape. special: type indices that alone carry TIER In [tin] — a class
    that selects it gets exactly those types."""
    rng = random.Random(f"fast cold {seed} {n_its} {n_res} {n_templates} {n_classes} {n_zones} {n_cts} {ops} {flavour}")
    sp = make_space(n_its, n_zones, n_cts)
    types, offers = [], []
    for i in range(n_its):
        t, o = gen_type(rng, sp, i, n_zones, n_cts)
        if special:
            t[TIER] = In(TIER, "tin") if i in special else In(TIER, *some(rng, TIERS[:3], 1, 2))
        types.append(t), offers.append(o)
    if n_its > 2:
        offers[n_its // 2] = {(n_zones - 1, n_cts - 1)}           # a type whose only available offering sits in the last cell
        types[n_its // 2][ZONE], types[n_its // 2][CT] = In(ZONE, sp.values[ZONE][-1]), In(CT, sp.values[CT][-1])
    alloc = [[rng.randint(1, big) for _ in range(n_its)] for _ in range(n_res)]
    for i in rng.sample(range(n_its), max(1, n_its // 10)) if n_its > 4 else []:
        alloc[rng.randrange(n_res)][i] = -rng.randint(1, 5)       # it_alloc_ok
    templates = []
    for t in range(n_templates):
        reqs = {}
        for key in (ARCH, ZONE, CT, TEAM, TIER):
            if rng.random() < (0.45 if key in (TEAM, TIER) else 0.35):
                how = rng.choice(["In", "In", "NotIn", "Exists", "DoesNotExist", "Gt"] if ops else ["In"])
                if how == "Gt":
                    reqs[key] = req(key, rng.choice(["Gt", "Lt"]), "3")       # no value of these dictionaries is an integer: nothing is inside the bounds
                elif how in ("In", "NotIn"):
                    reqs[key] = req(key, how, *some(rng, sp.values[key], 1, 3))
                else:
                    reqs[key] = req(key, how)
        if special:
            reqs.pop(TIER, None)
        if ops and rng.random() < 0.3:
            reqs[IT_KEY] = req(IT_KEY, rng.choice(["In", "NotIn"]), *some(rng, sp.values[IT_KEY], 1, max(1, n_its // 2)))
        templates.append(dict(reqs=reqs, its=set(range(n_its)) if rng.random() < 0.6 else set(some(rng, range(n_its), max(1, n_its // 2))), taints=rng.choice([0, 0, 1, 2, 3]),
                              limits=[rng.randint(0, 10 ** 6) for _ in range(n_res + 1)], limit_mask=0))
    classes = []
    for c in range(n_classes):
        reqs = {}
        for key in (ARCH, ZONE, CT, TEAM, TIER):
            if rng.random() < 0.4:
                how = rng.choice(["In", "In", "NotIn", "Exists"]) if flavour == 2 and key in (ARCH, ZONE, CT) else "In"
                reqs[key] = req(key, how, *some(rng, sp.values[key], 1, 3)) if how != "Exists" else req(key, "Exists")
        if special and c == 0:
            reqs = {TIER: In(TIER, "tin")}
        classes.append(dict(reqs=reqs, requests=[rng.randint(0, big // 4) for _ in range(n_res)], tolerates=rng.choice([0, 1, 3, 3])))
    tmpl_ov, groups = 0, [[] for _ in templates]
    if overhead:
        for t in range(n_templates):
            if t % 2 == 0:
                half = set(some(rng, range(n_its), 1, max(1, n_its - 1)))
                groups[t] = [(half, [rng.randint(0, big // 2) for _ in range(n_res)]), ((set(range(n_its)) - half - {0}) | {min(half)}, [rng.randint(0, 2 * big) for _ in range(n_res)])]       # (one type in both groups: the first counts)
                tmpl_ov |= 1 << t
    return Problem(sp, types, alloc, offers, templates, classes, n_zones, n_cts, tmpl_ov=tmpl_ov, groups=groups, plain=0 if ops else 1, plain_ops=1 if ops else 0, ops=ops, lim=lim,
                   flavour=flavour, rows=rows, plan=plan)


def gen_script(P, seed, n_sets=24, fits_per_set=3):
    """requirement sets that pods can reach — a template and a chain of classes each of which may join — entered once each, then
    looked up (before and after they are cached), with their cells and compatible types"""
    D = Definition(P)
    if D.decline:
        return [("CELLS", 0, ())]
    rng = random.Random(f"script {seed}")
    T, nc = len(P.templates), len(P.classes)
    sets, seen = [], set()
    for _ in range(n_sets * 4):
        t, chain = rng.randrange(T), ()
        for _ in range(rng.randint(0, 3)):
            k = rng.randrange(nc)
            if D.can_join(t, chain, k):
                chain += (k,)
        vm = D.pack_set(D.merged(t, chain), t)
        if vm not in seen and len(sets) < n_sets:
            seen.add(vm), sets.append((t, chain))
    script = []
    big = int(P.alloc.max())
    for i, (t, chain) in enumerate(sets):
        have = lambda: [rng.choice([0, rng.randint(0, big), rng.randint(0, big // 4)]) for _ in range(P.n_res)]
        if i % 3 == 0:
            script.append(("FITS", t, chain[:-1], chain[-1], have()) if chain else ("CELLS", t, chain))      # a lookup before the set is cached
        script.append(("ENTRY", t, chain))
        script += [("CELLS", t, chain), ("COMPAT", t, chain)]
    for t, chain in sets:
        for _ in range(fits_per_set):
            k = rng.randrange(nc)
            script.append(("FITS", t, chain, k, have()))
        if chain:
            script.append(("FITS", t, chain[:-1], chain[-1], have()))       # the set itself, as the loop reaches it
    return script


def front_problem(m, n_res=2, flavour=0, rows=1, plan=0, ties=False):
    """one template, one class, m + 2 types: an antichain of m allocatable vectors, one type dominated by one of them, one duplicate.
    ties: four resources, every vector the same in the first three — the last decides."""
    n = m + 2
    sp = make_space(n, 1, 1)
    types = [{IT_KEY: In(IT_KEY, f"type-{i}")} for i in range(n)]
    if ties:
        n_res, vec = 4, [(500, 7, 7 + i, 100 - i) for i in range(m)]
    else:
        vec = [tuple([100 + 10 * i, 900 - 10 * i] + [50] * (n_res - 2))[:n_res] for i in range(m)] if n_res > 1 else [(100,)] * m
    vec = vec + [tuple(max(0, x - 1) for x in vec[0]), vec[-1]]
    order = list(range(n))
    random.Random(f"front {m} {n_res}").shuffle(order)
    alloc = [[vec[order[i]][r] for i in range(n)] for r in range(n_res)]
    tm = [dict(reqs={}, its=set(range(n)), taints=0, limits=[0] * (n_res + 1), limit_mask=0)]
    cl = [dict(reqs={TEAM: In(TEAM, "a")}, requests=[1] * n_res, tolerates=0)]
    P = Problem(sp, types, alloc, [{(0, 0)}] * n, tm, cl, 1, 1, flavour=flavour, rows=rows, plan=plan)
    P.front_size = len({v for v in vec}) - 1 if not (n_res == 1) else 1
    return P


def front_script(P):
    vecs = sorted({tuple(int(P.alloc[r][i]) for r in range(P.n_res)) for i in range(P.n_its)})
    s = [("ENTRY", 0, ()), ("CELLS", 0, ()), ("COMPAT", 0, ())]
    for v in vecs:                                                   # every vector exactly, one more in each resource, one less
        s.append(("FITS", 0, (), 0, [x - 1 for x in v]))
        for r in range(P.n_res):
            s.append(("FITS", 0, (), 0, [x - 1 + (q == r) for q, x in enumerate(v)]))
    s.append(("FITS", 0, (), 0, [0] * P.n_res))
    return s


def hash_problem(flavour=0):
    """32 identical templates over one type, 46 classes (every non-empty subset of the teams, of the tiers): 14,880 reachable sets
    over a tiny catalogue, enough to pick runs that hash to one slot, sets at slot 1,023, and to fill the cache to its gate"""
    sp = make_space(1, 1, 1)
    types = [{IT_KEY: In(IT_KEY, "type-0")}]
    tm = [dict(reqs={TEAM: In(TEAM, *TEAMS), TIER: In(TIER, *TIERS)}, its={0}, taints=0, limits=[0, 0], limit_mask=0) for _ in range(32)]
    subsets = lambda vals: [[v for i, v in enumerate(vals) if (m >> i) & 1] for m in range(1, 1 << len(vals))]
    cl = [dict(reqs={TEAM: In(TEAM, *s)}, requests=[1], tolerates=0) for s in subsets(TEAMS)] + [dict(reqs={TIER: In(TIER, *s)}, requests=[1], tolerates=0) for s in subsets(TIERS)]
    return Problem(sp, types, [[100]], [{(0, 0)}], tm, cl, 1, 1, flavour=flavour)


def hash_sets(P):
    D = Definition(P)
    sets = [(t, (a, 31 + b)) for t in range(32) for a in range(31) for b in range(15)]
    by_hash = {}
    for s in sets:
        by_hash.setdefault(fast_hash(D.pack_set(D.merged(*s), s[0])), []).append(s)
    return D, sets, by_hash


def hash_script(P, fill):
    """three sets at slot 1,023 (slots 1,023, 0, 1), a run of five sets with one hash, lookups of every one of them and of a set
    that is not cached but probes through the run; fill: entries up to the gate (820) and one beyond, which is refused"""
    D, sets, by_hash = hash_sets(P)
    wrap, (h, run) = by_hash[1023][:3], max(((h, v) for h, v in by_hash.items() if h not in (1023, 0, 1, 2)), key=lambda kv: len(kv[1]))
    assert len(wrap) == 3 and len(run) >= 6
    picked = wrap + run[:5]
    script = [("ENTRY", t, c) for t, c in picked]
    look = lambda t, c: ("FITS", t, c[:1], c[1], [0])
    script += [look(t, c) for t, c in picked] + [look(*run[5])] + [look(*by_hash[1023][3])] if len(by_hash[1023]) > 3 else []
    if fill:
        rest = [s for s in sets if s not in picked and s != run[5]]
        script += [("ENTRY", t, c) for t, c in rest[:K_GATE - len(picked)]]
        script += [look(*rest[0]), look(*rest[K_GATE - len(picked) - 1]), look(*run[5]), ("ENTRY",) + rest[K_GATE]]       # the 821st
        script += [look(*rest[0])]                                       # behind the refusal: not run
    return script


def pool_problem():
    """17 identical templates over an antichain of 17 vectors: 16 entries fill the pool's 256 rows"""
    P = front_problem(17)
    P.templates = [dict(P.templates[0]) for _ in range(18)]
    P.groups = [[] for _ in P.templates]
    return P


def pool_script(P):
    return [("ENTRY", t, ()) for t in range(16)] + [("FITS", 15, (), 0, [259, 739]), ("FITS", 15, (), 0, [260, 739]), ("ENTRY", 16, ()), ("ENTRY", 17, ())]


CASES = {}


def case(name):
    def deco(f):
        CASES[name] = f
        return f
    return deco


def _gen(name, **kw):
    CASES[name] = lambda: (lambda P: (P, gen_script(P, name)))(gen_problem(name, **kw))


# sizes: types 1 / 63 / 64 / 65 / 130 / 2,048; templates 1 / 2 / 31 / 32; classes 1 / 64 / 65 / 130; resources 1..4; zones 1 / 16; capacity types 1 / 4
_gen("1-type", n_its=1, n_res=1, n_templates=1, n_classes=1, n_zones=1, n_cts=1)
_gen("63-types", n_its=63, n_res=2, n_templates=2, n_classes=64, special=(0, 62))
_gen("64-types", n_its=64, n_res=3, n_templates=2, n_classes=65, special=(0, 63), rows=4)
_gen("65-types", n_its=65, n_res=4, n_templates=31, n_classes=6, special=(63, 64), n_zones=16, n_cts=4)
_gen("130-types", n_its=130, n_res=2, n_templates=32, n_classes=130, special=(0, 64, 128, 129), rows=4)
_gen("2048-types", n_its=2048, n_res=2, n_templates=2, n_classes=4, special=(0, 1984, 2047))
_gen("operators", n_its=70, n_res=2, n_templates=8, n_classes=8, ops=1)
_gen("operators-130", n_its=130, n_res=3, n_templates=6, n_classes=8, ops=1, special=(64, 129), flavour=1)
_gen("overhead", n_its=40, n_res=3, n_templates=4, n_classes=6, overhead=True)
_gen("overhead-operators", n_its=66, n_res=2, n_templates=5, n_classes=6, overhead=True, ops=1, flavour=1, rows=4)
_gen("keep", n_its=30, n_res=2, n_templates=3, n_classes=6, flavour=1)
_gen("pod-operators", n_its=40, n_res=2, n_templates=1, n_classes=8, flavour=2)
_gen("pod-operators-4-rows", n_its=70, n_res=2, n_templates=2, n_classes=7, flavour=2, rows=4, ops=1)
_gen("plan-1", n_its=30, n_res=2, n_templates=3, n_classes=6, plan=1)
_gen("plan-2", n_its=30, n_res=2, n_templates=3, n_classes=6, plan=2, rows=4, flavour=1)
_gen("limits-switch", n_its=30, n_res=2, n_templates=3, n_classes=6, lim=1)
for _s in range(6):
    _gen(f"family-{_s}", n_its=24 + 9 * _s, n_res=1 + _s % 4, n_templates=2 + _s, n_classes=5 + _s, ops=_s % 2, overhead=_s % 3 == 0, flavour=(_s % 3 == 2) * 1)
for _m in (1, 2, 16, 17, 18):
    CASES[f"front-{_m}"] = lambda m=_m: (lambda P: (P, front_script(P)))(front_problem(m))
CASES["front-1-resource"] = lambda: (lambda P: (P, front_script(P)))(front_problem(3, n_res=1))
CASES["front-3-resources"] = lambda: (lambda P: (P, front_script(P)))(front_problem(5, n_res=3, rows=4))
CASES["front-ties"] = lambda: (lambda P: (P, front_script(P)))(front_problem(6, ties=True))
CASES["hash-runs"] = lambda: (lambda P: (P, hash_script(P, False)))(hash_problem())
CASES["cache-gate"] = lambda: (lambda P: (P, hash_script(P, True)))(hash_problem(flavour=1))
CASES["pool-full"] = lambda: (lambda P: (P, pool_script(P)))(pool_problem())


def load(name):
    return CASES[name]()


# ------------------------------------------------------------------------------------------------ declines, on both sides of each bound
def small(classes=None, templates=None, n_res=1, alloc=None, extra=(), n_its=4, **kw):
    sp = make_space(n_its, 2, 2, extra=extra)
    types = [{IT_KEY: In(IT_KEY, f"type-{i}"), ARCH: In(ARCH, "amd64")} for i in range(n_its)]
    templates = templates or [{}]
    tm = [dict(reqs=r, its=set(range(n_its)), taints=0, limits=[0] * (n_res + 1), limit_mask=0) for r in templates]
    cl = [dict(reqs=c.get("reqs", {}), requests=c.get("requests", [1] * n_res), tolerates=0) for c in (classes or [dict(reqs={ARCH: In(ARCH, "amd64")})])]
    return Problem(sp, types, alloc or [[100] * n_its] * n_res, [{(0, 0)}] * n_its, tm, cl, 2, 2, **kw)


def _keys(widths):
    return [(f"example.com/k{i}", [f"v{j}" for j in range(w)]) for i, w in enumerate(widths)]


def _selecting(widths):
    return [dict(reqs={f"example.com/k{i}": In(f"example.com/k{i}", "v0") for i in range(len(widths))})]


B30 = 1 << 30
_ov = lambda over: dict(tmpl_ov=1, groups=[[({0, 1, 2, 3}, [over])]])
DECLINES = {
    "plain": lambda: (small(), 0),
    "not plain": lambda: (small(plain=0), 1),
    "plain but for NodePool bounds, without the switch": lambda: (small(plain=0, plain_ops=1), 1),
    "plain but for NodePool bounds, with the switch": lambda: (small(plain=0, plain_ops=1, ops=1), 0),
    "4 resources": lambda: (small(n_res=4), 0),
    "5 resources": lambda: (small(n_res=5), 1),
    "32 templates": lambda: (small(templates=[{}] * 32), 0),
    "33 templates": lambda: (small(templates=[{}] * 33), 1),
    "NodePool NotIn": lambda: (small(templates=[{TEAM: req(TEAM, "NotIn", "a")}]), 3),
    "NodePool NotIn, with the switch": lambda: (small(templates=[{TEAM: req(TEAM, "NotIn", "a")}], ops=1), 0),
    "NodePool In []": lambda: (small(templates=[{TEAM: In(TEAM)}]), 3),
    "NodePool Exists": lambda: (small(templates=[{}, {TEAM: req(TEAM, "Exists")}]), 3),
    "NodePool Gt": lambda: (small(templates=[{TEAM: req(TEAM, "Gt", "1")}]), 3),
    "NodePool In": lambda: (small(templates=[{TEAM: In(TEAM, "a")}]), 0),
    "class NotIn": lambda: (small(classes=[dict(reqs={ARCH: req(ARCH, "NotIn", "arm64")})]), 4),
    "class Exists": lambda: (small(classes=[dict(), dict(reqs={ARCH: req(ARCH, "Exists")})], flavour=1), 4),
    "class NotIn under pod operators": lambda: (small(classes=[dict(reqs={ARCH: req(ARCH, "NotIn", "arm64")})], flavour=2), 0),
    "class selects on the hostname": lambda: (small(classes=[dict(reqs={HOSTNAME: In(HOSTNAME, "host-0")})]), 5),
    "class selects on the instance type": lambda: (small(classes=[dict(), dict(reqs={IT_KEY: In(IT_KEY, "type-1")})]), 5),
    "12 variable keys": lambda: (small(classes=_selecting([1] * 12), extra=_keys([1] * 12)), 0),
    "13 variable keys": lambda: (small(classes=_selecting([1] * 13), extra=_keys([1] * 13)), 6),
    "56 packed bits": lambda: (small(classes=_selecting([27, 27]), extra=_keys([27, 27])), 0),
    "57 packed bits": lambda: (small(classes=_selecting([27, 28]), extra=_keys([27, 28])), 6),
    "56 packed bits under pod operators": lambda: (small(classes=_selecting([26, 26]), extra=_keys([26, 26]), flavour=2), 0),
    "57 packed bits under pod operators": lambda: (small(classes=_selecting([27, 26]), extra=_keys([27, 26]), flavour=2), 6),
    "a key of two dictionary words": lambda: (small(classes=_selecting([65]), extra=_keys([65])), 6),
    "a wide key nobody selects on": lambda: (small(extra=_keys([65])), 0),
    "allocatable 2^30 - 1": lambda: (small(alloc=[[100, B30 - 1, 100, 100]]), 0),
    "allocatable 2^30": lambda: (small(alloc=[[100, 100, 100, B30]]), 7),
    "allocatable -2^30 + 1": lambda: (small(alloc=[[1 - B30, 100, 100, 100]]), 0),
    "allocatable -2^30": lambda: (small(n_res=2, alloc=[[100] * 4, [100, 100, -B30, 100]]), 7),
    "effective allocatable 2^30 - 1": lambda: (small(alloc=[[100, B30 - 2, 100, 100]], **_ov(-1)), 0),
    "effective allocatable 2^30": lambda: (small(alloc=[[100, B30 - 1, 100, 100]], **_ov(-1)), 7),
    "effective allocatable -2^30 + 1": lambda: (small(alloc=[[100, 0, 100, B30 - 1]], **_ov(B30 - 1)), 0),
    "effective allocatable -2^30": lambda: (small(alloc=[[100, 0, 100, B30 - 1]], **_ov(B30)), 7),
    "request 2^30 - 1": lambda: (small(classes=[dict(), dict(requests=[B30 - 1])]), 0),
    "request 2^30": lambda: (small(classes=[dict(), dict(requests=[B30])]), 7),
    "request 0": lambda: (small(classes=[dict(requests=[0])]), 0),
    "request -1": lambda: (small(classes=[dict(requests=[-1])]), 7),
    "class In []": lambda: (small(classes=[dict(), dict(reqs={TEAM: In(TEAM)})], templates=[{TEAM: In(TEAM, "a")}]), 8),
    "class In [] under pod operators": lambda: (small(classes=[dict(), dict(reqs={TEAM: In(TEAM)})], templates=[{TEAM: In(TEAM, "a")}], flavour=2), 0),
    "NotIn and In on a custom key a NodePool leaves undefined": lambda: (small(classes=[dict(reqs={TEAM: req(TEAM, "NotIn", "a")}), dict(reqs={TEAM: In(TEAM, "b")})], flavour=2), 9),
    "NotIn and In on a custom key every NodePool defines": lambda: (small(classes=[dict(reqs={TEAM: req(TEAM, "NotIn", "a")}), dict(reqs={TEAM: In(TEAM, "b")})],
                                                                          templates=[{TEAM: In(TEAM, "a", "b")}], flavour=2), 0),
    "NotIn and In on a well-known key a NodePool leaves undefined": lambda: (small(classes=[dict(reqs={ZONE: req(ZONE, "NotIn", "zone-0")}), dict(reqs={ZONE: In(ZONE, "zone-1")})], flavour=2), 0),
    "DoesNotExist and NotIn classes on one key": lambda: (small(classes=[dict(reqs={TEAM: req(TEAM, "DoesNotExist")}), dict(reqs={TEAM: req(TEAM, "NotIn", "a")})], flavour=2), 10),
    "DoesNotExist class, NotIn NodePool": lambda: (small(classes=[dict(reqs={TEAM: req(TEAM, "DoesNotExist")})], templates=[{TEAM: req(TEAM, "NotIn", "a")}], ops=1, flavour=2), 10),
    "DoesNotExist classes alone": lambda: (small(classes=[dict(reqs={TEAM: req(TEAM, "DoesNotExist")}), dict(reqs={TEAM: In(TEAM)})], flavour=2), 0),
    "class NotIn on a key with NodePool bounds": lambda: (small(classes=[dict(reqs={ARCH: req(ARCH, "NotIn", "arm64")})], templates=[{ARCH: req(ARCH, "Gt", "3")}], plain=0, plain_ops=1, ops=1, flavour=2), 11),
    "class NotIn, NodePool bounds on another key": lambda: (small(classes=[dict(reqs={ARCH: req(ARCH, "NotIn", "arm64")})], templates=[{TEAM: req(TEAM, "Lt", "3")}], plain=0, plain_ops=1, ops=1, flavour=2), 0),
    "class Exists on a well-known key a NodePool leaves undefined": lambda: (small(classes=[dict(reqs={ZONE: req(ZONE, "Exists")})], templates=[{ZONE: In(ZONE, "zone-0")}, {}], flavour=2), 12),
    "class Exists on a well-known key every NodePool defines": lambda: (small(classes=[dict(reqs={ZONE: req(ZONE, "Exists")})], templates=[{ZONE: In(ZONE, "zone-0")}], flavour=2), 0),
}


def _refused(P=None, script=None, **fields):
    def edit(arg, ops):
        for f, v in fields.items():
            if f.startswith("op_"):
                setattr(ops[0], f[3:], v)
            else:
                setattr(arg, f, v)
    return (P or small(), script or [("ENTRY", 0, ())], edit)


REFUSED = {
    "2,049 types": lambda: _refused(small(n_its=2049)),
    "17 zones": lambda: _refused(n_zones=17), "5 capacity types": lambda: _refused(n_cts=5), "no zone": lambda: _refused(n_zones=0),
    "2 rows": lambda: _refused(rows=2), "plan 3": lambda: _refused(plan=3), "flavour 3": lambda: _refused(flavour=3), "no claim": lambda: _refused(max_claims=0),
    "no class": lambda: _refused(n_classes=0), "no template": lambda: _refused(n_templates=0), "9 resources": lambda: _refused(n_res=9),
    "a requirement set of template 1 of 1": lambda: _refused(op_vm=1 << 56), "of template 255": lambda: _refused(op_vm=0xFF << 56),
    "of template 32 with limit stages": lambda: _refused(small(lim=1), op_vm=32 << 56),
    "an unknown operation": lambda: _refused(op_op=9), "operation 0": lambda: _refused(op_op=0),
    "filter_diag without the set-aside list": lambda: _refused(op_op=5),
    "a class outside the classes": lambda: _refused(op_op=6, op_k=1), "class -1": lambda: _refused(op_op=7, op_k=-1),
    "a claim outside the claims": lambda: _refused(op_op=8, op_x=64), "claim -1": lambda: _refused(op_op=8, op_x=-1),
    "tmpl_ov names a template that is not there": lambda: _refused(tmpl_ov=2),
}


# ------------------------------------------------------------------------------------------------ the loop's cold events: class slots, new claims, pods joining
def loop_problem(seed, flavour, rows, plan, n_classes=12, n_templates=3, n_its=40, n_res=2, ops=0, **kw):
    """the first gen_problem setup() takes, with classes that fail in every way: taints they do not tolerate, requirements no template meets, requests no type holds"""
    for attempt in range(200):        # (the first generated problem that setup() takes: the pod operators decline many mixes)
        P = gen_problem(f"loop {seed} {attempt}", n_its=n_its, n_res=n_res, n_templates=n_templates, n_classes=n_classes, flavour=flavour, rows=rows, plan=plan, ops=ops, **kw)
        if not decline_reason(P):
            break
    rng = random.Random(f"loop classes {seed}")
    big = int(P.alloc.max())
    for c, cl in enumerate(P.classes):
        how = c % 6
        if how == 3:
            cl["requests"] = [big + 1 + rng.randint(0, 5)] + [0] * (P.n_res - 1)          # no type holds it
        elif how == 4:
            cl["requests"] = [rng.randint(big // 2, big) for _ in range(P.n_res)]          # few types hold it
        elif how == 5 and c % 12 == 5:
            cl["tolerates"] = 0
        else:
            cl["tolerates"] = 3
    for T in P.templates[::2]:
        T["taints"] = T["taints"] or 1
    if P.lim:                                              # NodePool limits that bind after a few claims; one pool with its nodes used up
        for t, T in enumerate(P.templates):
            T["limit_mask"] = rng.choice([1, 1 << (P.n_res - 1), (1 << P.n_res) - 1]) | ((1 << P.n_res) if t == 1 else 0)
            T["limits"] = [rng.randint(1, 4) * big for _ in range(P.n_res)] + [0 if t == 1 else 5]
    return P


def loop_script(P, seed, n_events=60):
    """the events of the loop as it raises them: a class takes a slot when its first pod comes, a pod that no claim accepts opens a
    claim, a pod an acceptance bit admits joins the claim (the model's own CanAdd decides which), with lookups and filter_diag between"""
    D = Definition(P)
    assert not D.decline, D.decline
    rng = random.Random(f"loop script {seed}")
    M, script, nc = Model(D, P.claim_cap or 1 << 30), [], len(P.classes)
    slotted = set()
    lost = [] if P.flavour >= 1 else [k for k in range(nc) if Model(D, 1 << 30).new_claim(k, False) != 1]      # without the set-aside list such a pod ends the engine: the last event
    for _ in range(n_events):
        k = rng.choice([k for k in range(nc) if k not in lost])
        if k not in slotted:
            script.append(("SLOT", k)), M.new_slot(k), slotted.add(k)
            if M.evicted:
                slotted = {k}
        takers = [x for x, cl in enumerate(M.claims) if M.can_add(cl, k, cached=False)]
        if takers and rng.random() < 0.7:
            x = takers[0]
            script.append(("ADD", x, k)), M.add(x, k)
        else:
            script.append(("NEWCLAIM", k, 0))
            if M.new_claim(k, False) == 0:
                break
        if P.flavour >= 1 and rng.random() < 0.3:
            t = rng.randrange(len(P.templates))
            script.append(("DIAG", t, (k,) if D.can_join(t, (), k) else (), [rng.choice([0, 1, int(P.alloc.max()) // 2, int(P.alloc.max()) + 1]) for _ in range(P.n_res)]))
        if M.claims and rng.random() < 0.3:
            x = rng.randrange(len(M.claims))
            t, chain, have = M.claims[x]
            script.append(("FITS", t, chain, k, have[:P.n_res]))
    if lost and not M.bail:
        script += [("NEWCLAIM", lost[0], 0), ("NEWCLAIM", 0, 0)]
    return script


def _loop(name, flavour, rows, plan, **kw):
    CASES[name] = lambda: (lambda P: (P, loop_script(P, name)))(loop_problem(name, flavour, rows, plan, **kw))


_loop("loop-plain", 0, 1, 0, n_classes=6)
_loop("loop-plain-4-rows", 0, 4, 0, n_classes=70, n_templates=4)
_loop("loop-keep", 1, 1, 0)
_loop("loop-keep-4-rows", 1, 4, 0, n_classes=80, n_templates=5, ops=1)
_loop("loop-pod-operators", 2, 1, 0, n_templates=1)
_loop("loop-pod-operators-4-rows", 2, 4, 0, n_templates=1, n_classes=10)
_loop("loop-plan-1", 0, 1, 1, n_classes=6)
_loop("loop-plan-2", 1, 4, 2, n_classes=30, overhead=True)
_loop("loop-keep-overhead", 1, 1, 0, overhead=True, ops=1, n_res=4)
_loop("loop-keep-130-types", 1, 1, 0, n_its=130, n_classes=20, special=(0, 64, 129))


def _with(P, **kw):
    for f, v in kw.items():
        setattr(P, f, v)
    return P


def _placeable(P):
    D = Definition(P)
    M = Model(D, 1 << 30)
    return [k for k in range(len(P.classes)) if Model(D, 1 << 30).new_claim(k, False) == 1]


def _edge(name, make):
    CASES[name] = make


# a verdict kept and used again; the retry's net on both sides; the capacity and the plan's claim slots; a pod nobody takes without the set-aside list
_edge("verdict-reused", lambda: (lambda P: (P, [("NEWCLAIM", 3, 0), ("NEWCLAIM", 3, 0), ("NEWCLAIM", 3, 1), ("NEWCLAIM", 0, 0), ("NEWCLAIM", 3, 0)]))(loop_problem("verdict", 1, 1, 0)))
_edge("retry-net", lambda: (lambda P: (P, [("NEWCLAIM", 3, 1), ("NEWCLAIM", _placeable(P)[0], 1), ("NEWCLAIM", 3, 1)]))(loop_problem("verdict", 1, 1, 0)))
_edge("unschedulable-without-the-list", lambda: (lambda P: (P, [("NEWCLAIM", _placeable(P)[0], 0), ("NEWCLAIM", 3, 0), ("NEWCLAIM", _placeable(P)[0], 0)]))(loop_problem("verdict", 0, 1, 0)))
_edge("max-claims", lambda: (lambda P: (P, [("NEWCLAIM", _placeable(P)[0], 0)] * 5))(_with(loop_problem("verdict", 1, 1, 0), max_claims=3)))
_edge("claim-slots", lambda: (lambda P: (P, [("NEWCLAIM", _placeable(P)[0], 0)] * 4))(_with(loop_problem("verdict", 0, 4, 0), max_claims=5, claim_cap=2)))
_edge("no-active-template", lambda: (lambda P: (P, [("NEWCLAIM", 0, 0), ("NEWCLAIM", 1, 0)]))(_with(small(flavour=1, classes=[dict(), dict()]), offers=[set()] * 4)))
# every slot taken: the 65th class of one row, the 257th of four, drops them all
_edge("evict-1-row", lambda: (lambda P: (P, [("NEWCLAIM", _placeable(P)[0], 0)] + [("SLOT", k) for k in range(66)] + [("NEWCLAIM", _placeable(P)[1], 0), ("ADD", 0, _placeable(P)[0])]))(
    loop_problem("evict", 0, 1, 0, n_classes=66)))
_edge("evict-4-rows", lambda: (lambda P: (P, [("NEWCLAIM", _placeable(P)[0], 0)] + [("SLOT", k) for k in range(258)] + [("NEWCLAIM", _placeable(P)[1], 0)]))(
    loop_problem("evict", 1, 4, 0, n_classes=258)))


# single conditions the generated problems reach too rarely to count on
def _pod_operator_types():
    """a claim whose NotIn set pods have grown meets types of every operator on the key: In the last dictionary value, NotIn, Exists, DoesNotExist, undefined, In a value the set excludes"""
    sp = make_space(6, 1, 1)
    types = [{IT_KEY: In(IT_KEY, f"type-{i}")} for i in range(6)]
    for i, r in enumerate([In(TEAM, "e"), req(TEAM, "NotIn", "a"), req(TEAM, "Exists"), req(TEAM, "DoesNotExist"), None, In(TEAM, "a")]):
        if r:
            types[i][TEAM] = r
    tm = [dict(reqs={}, its=set(range(6)), taints=0, limits=[0, 0], limit_mask=0)]
    cl = [dict(reqs={TEAM: req(TEAM, "NotIn", "a")}, requests=[1], tolerates=0), dict(reqs={TEAM: req(TEAM, "NotIn", "b", "c")}, requests=[1], tolerates=0),
          dict(reqs={TEAM: req(TEAM, "NotIn", *TEAMS)}, requests=[1], tolerates=0)]       # no dictionary value left: an Exists type still intersects (two complements)
    P = Problem(sp, types, [[100] * 6], [{(0, 0)}] * 6, tm, cl, 1, 1, flavour=2)
    script = [op for chain in ((), (0,), (1,), (0, 1), (2,), (0, 2)) for op in (("ENTRY", 0, chain), ("COMPAT", 0, chain), ("CELLS", 0, chain), ("FITS", 0, chain, 0, [0]), ("FITS", 0, chain, 1, [98]))]
    return P, script + [("SLOT", 0), ("SLOT", 1), ("NEWCLAIM", 0, 0), ("ADD", 0, 1), ("NEWCLAIM", 1, 0)]


def _exists_against_does_not_exist():
    P = small(templates=[{TEAM: req(TEAM, "DoesNotExist")}, {TEAM: In(TEAM, "a")}], classes=[dict(reqs={TEAM: req(TEAM, "Exists")}), dict(reqs={TEAM: req(TEAM, "DoesNotExist")})], ops=1, flavour=2)
    return P, [("CELLS", 1, ()), ("SLOT", 0), ("SLOT", 1), ("NEWCLAIM", 0, 0), ("NEWCLAIM", 1, 0), ("FITS", 0, (), 0, [0]), ("FITS", 1, (), 1, [0])]


def _fits_without_an_offering():
    """the only type that holds the pod has no offering in the zone the pod selects: it does not fit (nodeclaim.go:624-638)"""
    sp = make_space(2, 2, 1)
    types = [{IT_KEY: In(IT_KEY, f"type-{i}"), ZONE: In(ZONE, f"zone-{i}")} for i in range(2)]
    tm = [dict(reqs={}, its={0, 1}, taints=0, limits=[0, 0], limit_mask=0)]
    cl = [dict(reqs={ZONE: In(ZONE, "zone-1")}, requests=[500], tolerates=0)]
    return Problem(sp, types, [[1000, 10]], [{(0, 0)}, {(1, 0)}], tm, cl, 2, 1, flavour=1), [("DIAG", 0, (0,), [500]), ("NEWCLAIM", 0, 0), ("DIAG", 0, (), [500]), ("DIAG", 0, (0,), [5])]


CASES["pod-operators-types"] = _pod_operator_types
CASES["exists-against-does-not-exist"] = _exists_against_does_not_exist
CASES["fits-without-an-offering"] = _fits_without_an_offering


# ------------------------------------------------------------------------------------------------ NodePool limits
def chain_problem(r0, n_templates=1, lim=1, flavour=1, rows=1, nodes=None):
    """36 types whose capacities in the limited resource all differ, one of them (capacity 1) the only type that holds a pod of class 0:
    every claim of class 0 takes 1 off `remaining`, and from 58 down every claim's list is one type narrower than the one before — a
    new limit stage per claim. Class 1 fits every type (its claims take the largest capacity left), class 2 none. With two templates the
    pools are told apart by taints: class 0 tolerates the first alone, class 3 is class 0 for the second."""
    n = 36
    sp = make_space(n, 1, 1)
    types = [{IT_KEY: In(IT_KEY, f"type-{i}")} for i in range(n)]
    caps = [1] + [60 - i for i in range(1, n)]
    alloc = [[100] * n, [1000] + [10] * (n - 1)]
    tm = [dict(reqs={}, its=set(range(n)), taints=(1 << t) if n_templates > 1 else 0, limits=[r0, 0, 0 if nodes is None else nodes], limit_mask=1 | (4 if nodes is not None else 0))
          for t in range(n_templates)]
    cl = [dict(reqs={}, requests=[1, 500], tolerates=1), dict(reqs={}, requests=[1, 1], tolerates=3), dict(reqs={}, requests=[1, 5000], tolerates=3),
          dict(reqs={}, requests=[1, 500], tolerates=2)]
    return Problem(sp, types, alloc, [{(0, 0)}] * n, tm, cl, 1, 1, cap=[caps, alloc[1]], lim=lim, flavour=flavour, rows=rows, max_claims=128)


def _chain(r0, script, **kw):
    return lambda: (chain_problem(r0, **kw), script)


_A, _B, _C, _A2 = ("NEWCLAIM", 0, 0), ("NEWCLAIM", 1, 0), ("NEWCLAIM", 2, 0), ("NEWCLAIM", 3, 0)
# a stage at the first claim and at every claim after it, until no id is left: the 33rd id
CASES["limit-stages-33"] = _chain(58, [("SLOT", 0), ("SLOT", 1)] + [_A] * 16 + [("ADD", 3, 0), ("FITS", 5, (0,), 1, [1, 500]), ("FITS", 9, (0,), 0, [99, 500]), ("COMPAT", 16, ()), ("CELLS", 16, (0,))] + [_A] * 20)
# the limits exclude nothing until a middle claim; a verdict kept, used again, voided when the limits move, and E_LIMITS once no type is left
CASES["limit-middle-claim"] = _chain(62, [("SLOT", 2), _C, _C] + [_A] * 3 + [_C, _C, _A, _A, _C, ("DIAG", 1, (0,), [1, 500])] + [_B] * 3 + [_C, _A], rows=4)
# ... and only at the script's last claim
CASES["limit-last-claim"] = _chain(61, [_A] * 4, flavour=0)
# two NodePools exhausting alternately: their stages' ids interleave
CASES["limit-two-pools"] = _chain(58, [("SLOT", 0), ("SLOT", 3)] + [_A, _A2] * 6 + [_B] * 4 + [_A, _A2], n_templates=2)
# a pool whose nodes are used up is skipped (E_LIMITS); without limit stages the engine stops instead, as it does when a limit excludes a type
CASES["limit-nodes-used-up"] = _chain(62, [_A, _B, _C], nodes=0)
CASES["limit-nodes-left"] = _chain(62, [_A, _B, _C, _A], nodes=1)
CASES["limit-nodes-used-up-without-stages"] = _chain(62, [_A], nodes=0, lim=0)
CASES["limit-excludes-without-stages"] = _chain(61, [_A] * 5, lim=0, flavour=0)
_loop("loop-limits", 1, 1, 0, lim=1, n_classes=10)
_loop("loop-limits-4-rows", 1, 4, 0, lim=1, n_classes=70, n_templates=4, ops=1)
_loop("loop-limits-plain", 0, 1, 0, lim=1, n_classes=8)
# the cache at its gate when a new claim needs an entry
def _cache_full_new_claim():
    P = hash_problem(flavour=1)
    D = Definition(P)
    D_, sets, _ = hash_sets(P)
    entries = [("ENTRY", t, c) for t, c in sets if t][:K_GATE]          # (no set of template 0, where every new claim starts)
    cached = {D.pack_set(D.merged(t, c), t) for _, t, c in entries}
    k = next(k for k in range(len(P.classes)) if D.pack_set(D.merged(0, (k,)), 0) not in cached)       # a class whose first claim needs an entry of its own
    return P, entries + [("NEWCLAIM", k, 0), ("NEWCLAIM", k, 0)]


CASES["cache-full-new-claim"] = _cache_full_new_claim
