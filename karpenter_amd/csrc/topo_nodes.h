// topo_nodes.h — the spread engine's existing-node path: addToExistingNode (scheduler.go:614-656) for one pod, INSIDE the engine's
// per-pod step (topo_engine.h, TopoEngine<W, true>), in front of its claim selection.
//
// Why this is not node_stage.h once more. The cursor engine's stage rests on two facts: the (class, node) verdict is static up to
// resources, and `remaining` only shrinks, so a rejection is permanent and the whole queue can be run against the nodes before
// the loop starts. With topology the second fact fails for groups on dictionary keys: a node in zone 1 that refuses a pod for skew
// accepts a later pod of the same class once pods have landed in zones 2 and 3 — on nodes or on NodeClaims. Node or NodeClaim
// depends on counters the claims move, so the test stands inside the step. ExistingNode.CanAdd (existingnode.go:81-139) splits into
//   * checks that only ever move towards rejection — the static row (taints, strict Compatible: ksolve_node_dead0), resources.Fits
//     against `remaining`, and for every hostname group of the pod count(node) + self <= limit (the hostname key's minimum is 0:
//     topologygroup.go:236-249, :407-415; per-node counts only grow). These keep the stage's scheme: per class an alive word per
//     64-node block and a cursor, the first block whose word is not zero. A node's hostname counters are ONE 64-bit word of 4-bit
//     fields, the layout of a claim record (TopoRec::hcnt), so the class's hlim / hinc compare and add work on it unchanged.
//   * checks that go both ways — for every dictionary-key group of the pod the node's single domain must be one the pod may take
//     NOW (topologygroup.go:229-298, :324-388, :404-439 with nodeDomains a one-value set): bit z(node) of the candidate-domain mask
//     the engine evaluates once per pod anyway (TopoEngine::choose_domains). A node that fails only this keeps its alive bit, and
//     the cursor does not move past its block.
// The lowest node index that passes everything wins (scheduler.go:639). The commit (existingnode.go:172-185, topology.go:197-220):
// remaining -= requests, slot = the node's pod count, every dictionary-key group that counts the pod counts the node's domain
// (a one-domain set: Record always counts; anti-affinity blocks the same one domain), every hostname group adds its increment.
//
// Where the tables live. The engine's LDS plan is nearly full, so `remaining`, the pod counts, the hostname words, the nodes'
// domain indices, the alive words and the cursors are in the HBM workspace (L2-resident at these sizes: 2,000 nodes x 500 classes
// = 190 KB). A pod whose class still has a live block costs three dependent round trips — the class's cursor (with its requests),
// the alive words of up to 64 blocks from the cursor on (one lane each: blocks without a live node are skipped by a ballot, not
// visited), the block's nodes (one lane each: remaining, pod count, hostname word, domain bytes, all issued together) — and the
// fence behind the commit's stores. The walk past a block whose nodes are alive but inadmissible by domain costs the third trip
// again per block. A class whose cursor has reached the end costs nothing: the loop reads the cursors once per 64 pods.
// One wavefront; plain vector stores; written on W:: only, so that the emulation runs this source.
#pragma once
#include "fast_engine.h"
#include "topo_types.h"

namespace ks {

struct TopoNodePick { int node; uint32_t slot; };   // node < 0: no node takes the pod

// ---- Topology node filters (engines 24 / 25; topo_engine.h, "Topology node filters") ----
// TopologyNodeFilter.Matches (topologynodefilter.go:68-96) of slot s for a bin whose packed requirement word is m. `undef`: the guard
// bits of the keys the bin does not define — the strict Compatible of :71 fails an In term on such a key, well known or not, while a
// guard bit that stands for a NodePool's own NotIn / Exists / Gt / Lt is a defined key whose field holds the values it admits.
KS_FN bool topo_filter_matches(const TopoFiltSlot& s, const KS_LDS FastMisc* Mp, int nv, uint64_t m, uint64_t undef, bool taints_ok) {
  if (!taints_ok) return false;
  if (!s.n_terms) return true;
  for (int i = 0; i < (int)s.n_terms; ++i) {   // any term (topologynodefilter.go:89-95)
    bool ok = true;
    for (int j = 0; j < nv; ++j) {
      const uint64_t fm = Mp->fmask[j];
      if (!(s.fdm[i] & fm)) continue;
      if (!(m & s.fvm[i] & fm) || ((undef >> (Mp->voff[j] + Mp->vwidth[j])) & 1)) ok = false;
    }
    if (ok) return true;
  }
  return false;
}
// the slots `fs` of a class against one bin: the bits of its hinc / zsel that Record (topology.go:197-220) does not count there
template <class TOK>
KS_FN TopoFiltCut topo_filter_cut(const TopoFilt* ft, const KS_LDS FastMisc* Mp, int nv, uint32_t fs, uint64_t m, uint64_t undef, TOK taints_ok) {
  TopoFiltCut c; c.h = 0; c.z = 0;
  for (uint32_t b = fs & ((1u << kTopoFiltSlots) - 1u); b; b &= b - 1) {
    const TopoFiltSlot s = ft->slot[ctz64(b)];
    if (!topo_filter_matches(s, Mp, nv, m, undef, taints_ok(s))) { c.h |= s.hbit; c.z |= s.zbit; }
  }
  return c;
}
// ... under the pod operators of engines 29 / 30 (topo_engine.h, "The spread engine's pod operators"): a term may be NotIn / Exists /
// DoesNotExist, packed like a class over fields whose top bit is the phantom value; the guard bit's position in fvm marks a NotIn /
// DoesNotExist term on that key, which passes a bin that does not define the key. On a defined key strict Compatible is "the two
// fields share a bit" (requirements.go:254-274 with the escape of :260-265 — what setup_filters declines is what this cannot read).
KS_FN bool topo_filter_matches_po(const TopoFiltSlot& s, const KS_LDS FastMisc* Mp, int nv, uint64_t m, uint64_t undef, bool taints_ok) {
  if (!taints_ok) return false;
  if (!s.n_terms) return true;
  for (int i = 0; i < (int)s.n_terms; ++i) {
    bool ok = true;
    for (int j = 0; j < nv; ++j) {
      const uint64_t fm = Mp->fmask[j];
      if (!(s.fdm[i] & fm)) continue;
      const int gb = Mp->voff[j] + Mp->vwidth[j];
      if ((undef >> gb) & 1) { if (!((s.fvm[i] >> gb) & 1)) ok = false; }
      else if (!(m & s.fvm[i] & fm)) ok = false;
    }
    if (ok) return true;
  }
  return false;
}
template <class TOK>
KS_FN TopoFiltCut topo_filter_cut_po(const TopoFilt* ft, const KS_LDS FastMisc* Mp, int nv, uint32_t fs, uint64_t m, uint64_t undef, TOK taints_ok) {
  TopoFiltCut c; c.h = 0; c.z = 0;
  for (uint32_t b = fs; b; b &= b - 1) {   // (kTopoFiltSlotsPodOps slots: every bit of the class's word)
    const TopoFiltSlot s = (&ft->slot[0])[ctz64(b)];
    if (!topo_filter_matches_po(s, Mp, nv, m, undef, taints_ok(s))) { c.h |= s.hbit; c.z |= s.zbit; }
  }
  return c;
}
struct TopoNoFilt { static constexpr bool on = false; };   // every other setting: the node commit counts what the class says
struct TopoNodeFilt { static constexpr bool on = true; uint32_t fs; int nv; const TopoFilt* ft; };   // fs: the class's slots (0: none)
// ... against an existing node: its packed word from its label row (a node defines a key with ONE value, ksolve_impl.h
// node_stage_declines) and its own taints against the owner's tolerations
template <class W>
KS_COLD TopoFiltCut topo_node_filter_cut(const ProblemView* Pk, const Workspace* Sk, const KS_LDS FastMisc* Mp, TopoNodeFilt ctx, int node) {
  const int nn = Pk->n_nodes;
  const uint32_t ndef = Sk->n_defined0[node];
  uint64_t m = 0, undef = 0;
  for (int j = 0; j < ctx.nv; ++j) {
    const uint64_t guard = 1ull << (Mp->voff[j] + Mp->vwidth[j]);
    if ((ndef >> Mp->vkey[j]) & 1u) m |= (Sk->n_mask0[(size_t)Mp->vword[j] * nn + node] << Mp->voff[j]) & Mp->fmask[j];
    else { m |= Mp->fmask[j] | guard; undef |= guard; }
  }
  const uint64_t taints = Pk->node_taints[node];
  const uint64_t* tol = Pk->topo.f_tolerates;
  return topo_filter_cut(ctx.ft, Mp, ctx.nv, ctx.fs, m, undef, [&](const TopoFiltSlot& s) { return !(s.taint && (taints & ~tol[s.group])); });
}


// ---- Pod operators beside existing nodes on the spread engine (engines 35 / 36; TopoEngine's NP) ----
// A node's label sets are single-valued In sets (reason 32) and existing nodes pass no AllowUndefined (existingnode.go:100), so what
// node_stage.h says of the cursor engine's stage holds here word for word: the (class, node) verdict up to resources is the row
// ksolve_node_dead0 computes (nodecheck.h kneg) — TopoNodes::dead0 IS that row, so the half of topo_nodes_place that only moves towards
// rejection needs nothing new — and the candidate-domain half needs nothing new either: every group key is defined on every node
// (reason 35), choose_domains evaluates a NotIn S class's field as "the values outside S", and a node's one domain is a dictionary
// value, never the phantom bit (a value that would be index kTopoMaxDom - 1 under the phantom layout: reason 36, below).
// Two things are new.
//  1. The node filter. Under the phantom layout a group's TopologyNodeFilter may hold NotIn / Exists / DoesNotExist terms in up to
//     kTopoFiltSlotsPodOps slots, read by topo_filter_matches_po. The node's packed word is already in that layout: a key the node
//     defines is its ONE value bit (no phantom bit, guard clear: a concrete set), a key it lacks is all ones with the guard bit, and
//     `undef` says so — a NotIn / DoesNotExist term passes it, an In / Exists term fails it (requirements.go:185-193).
//  2. Definedness. A NotIn S pod that lands on a node lacking key K writes NotIn S onto the node (existingnode.go:172-176); from
//     then on an In / Exists POD passes where it failed (node_stage.h, reason 37) and so does an In / Exists TERM of a node filter,
//     which here reads the node's pristine label row. topo_nodes_definedness declines both before any pod is placed. A DoesNotExist
//     pod needs no decline — behind it, on that node:
//         later pod / term    In S   Exists   NotIn S   DoesNotExist
//         before (K lacking)  fails  fails    passes    passes
//         after (K: In [])    fails  fails    passes    passes        (empty intersection, positive incoming operator; both negative: requirements.go:260-264)
struct TopoNodeFiltPo { static constexpr bool on = true; uint32_t fs; int nv; const TopoFilt* ft; bool po; };   // po: this batch has the phantom layout
template <class W>
KS_COLD TopoFiltCut topo_node_filter_cut(const ProblemView* Pk, const Workspace* Sk, const KS_LDS FastMisc* Mp, TopoNodeFiltPo ctx, int node) {
  if (!ctx.po) { TopoNodeFilt c; c.fs = ctx.fs; c.nv = ctx.nv; c.ft = ctx.ft; return topo_node_filter_cut<W>(Pk, Sk, Mp, c, node); }
  const int nn = Pk->n_nodes;
  const uint32_t ndef = Sk->n_defined0[node];
  uint64_t m = 0, undef = 0;
  for (int j = 0; j < ctx.nv; ++j) {
    const uint64_t guard = 1ull << (Mp->voff[j] + Mp->vwidth[j]);
    if ((ndef >> Mp->vkey[j]) & 1u) m |= (Sk->n_mask0[(size_t)Mp->vword[j] * nn + node] << Mp->voff[j]) & Mp->fmask[j];   // one dictionary value: the phantom bit stays clear
    else { m |= Mp->fmask[j] | guard; undef |= guard; }
  }
  const uint64_t taints = Pk->node_taints[node];
  const uint64_t* tol = Pk->topo.f_tolerates;
  return topo_filter_cut_po(ctx.ft, Mp, ctx.nv, ctx.fs, m, undef, [&](const TopoFiltSlot& s) { return !(s.taint && (taints & ~tol[s.group])); });
}
// The shape check of a batch with nodes under the phantom layout, before any pod is placed: DECLINE_NODE_KEY_DEFINEDNESS for a key K
// that some node lacks, some class uses with NotIn, and some class OR some node-filter term uses with In (non-empty) or Exists — per
// key over all nodes, classes and terms: conservative, never optimistic —, DECLINE_NODE_DOMAIN_RANGE for a node whose value of a
// group's key is the index the phantom bit takes. 0: neither.
template <class W>
KS_COLD int topo_nodes_definedness(const ProblemView* Pk, const Workspace* Sk, const TopoWork* Tk) {
  const ProblemView& Pv = *Pk; const Dict& d = Pv.dict;
  const int nn = Pv.n_nodes, nc = Pv.n_classes;
  const uint32_t* const ndef = Sk->n_defined0;
  const uint32_t all_keys = d.n_keys >= 32 ? 0xFFFFFFFFu : (1u << d.n_keys) - 1;
  auto keys_of = [&](const ReqRef& r, bool notin) {
    uint64_t m = 0;
    for (uint32_t ks_ = r.defined; ks_; ks_ &= ks_ - 1) {
      const int k = __builtin_ctz(ks_);
      const int op = req_op(d, r, k);
      if (notin ? op == OP_NOTIN : (op == OP_IN || op == OP_EXISTS)) m |= 1ull << k;
    }
    return m;
  };
  const uint32_t k_notin = (uint32_t)W::reduce_or(nc, [&](int c) { return keys_of(Pv.cls_reqs.at(d, c), true); });      // keys some class uses with NotIn
  uint32_t k_positive = (uint32_t)W::reduce_or(nc, [&](int c) { return keys_of(Pv.cls_reqs.at(d, c), false); });        // ... with In (non-empty) or Exists
  k_positive |= (uint32_t)W::reduce_or((int)Pv.topo.f_first[Pv.topo.n_groups], [&](int i) { return keys_of(Pv.topo.f_reqs.at(d, i), false); });   // ... or some term of a node filter does
  const uint32_t k_undef = (uint32_t)W::reduce_or(nn, [&](int e) { return (uint64_t)(~ndef[e] & all_keys); });          // keys some node leaves undefined
  if (k_notin & k_positive & k_undef) return DECLINE_NODE_KEY_DEFINEDNESS;
  const uint8_t* const dom = Tk->nd.dom;
  const uint32_t gkeys = (uint32_t)W::reduce_or(Pv.topo.n_groups, [&](int g) { return Pv.topo.key[g] >= 0 ? (uint64_t)1 << Pv.topo.key[g] : (uint64_t)0; });
  for (uint32_t ks_ = gkeys & all_keys; ks_; ks_ &= ks_ - 1) {
    const uint8_t* const row = dom + (size_t)__builtin_ctz(ks_) * nn;
    if (W::reduce_or(nn, [&](int e) { return (uint64_t)(row[e] >= (uint8_t)(kTopoMaxDom - 1) ? 1 : 0); })) return DECLINE_NODE_DOMAIN_RANGE;
  }
  return DECLINE_NONE;
}

// the per-solve state, from the pristine tables (the kernel's own set-up has accepted the problem: at most sixteen hostname groups)
template <class W>
KS_COLD void topo_nodes_init(const ProblemView* Pk, const Workspace* Sk, const TopoWork* Tk) {
  const ProblemView& P = *Pk; const Workspace& S = *Sk; const TopoNodes N = Tk->nd;
  const int nn = P.n_nodes, nw = P.node_words, nr = P.n_res, nc = P.n_classes;
  const int nh = P.topo.n_host_groups < kTopoMaxHost ? P.topo.n_host_groups : kTopoMaxHost;
  const int64_t* rem0 = S.n_remaining0; int64_t* rem = S.n_remaining; uint32_t* cnt = S.n_npods;
  const int32_t* nc0 = P.topo.node_counts0;
  W::for_n(nr * nn, [&](int i) { rem[i] = rem0[i]; });
  W::for_n(nn, [&](int e) {
    uint64_t w = 0;
    for (int f = 0; f < nh; ++f) { const int32_t c = nc0[(size_t)f * nn + e]; w |= (uint64_t)(c < 0 ? 0 : c > 7 ? 7 : c) << (4 * f); }
    N.hword[e] = w; cnt[e] = 0;
  });
  W::for_n(nc * nw, [&](int i) { N.alive[i] = ~N.dead0[i]; });   // (ksolve_node_dead0 marks the bits past the last node dead)
  W::for_n(nc, [&](int c) { N.cursor[c] = 0; });
}

// One pod of class k: the node that takes it, committed. hlim / hinc / zsel: the class's TopoClass; (zg0, vm0), (zg1, vm1): the
// dictionary-key groups it is tested against (-1: none) with their candidate-domain masks of this step.
// FILT: engines 24 / 25 — the filters of the groups that count the class are asked about the node that takes the pod.
template <class W, class FILT = TopoNoFilt>
KS_COLD TopoNodePick topo_nodes_place(const ProblemView* Pk, const Workspace* Sk, const TopoWork* Tk, KS_LDS TopoState* st, const KS_LDS FastMisc* Mp,
                                      uint32_t k, uint64_t hlim, uint64_t hinc, uint64_t zsel, int zg0, uint32_t vm0, int zg1, uint32_t vm1, FILT filt = FILT()) {
  TopoNodePick pick; pick.node = -1; pick.slot = 0;
  const TopoNodes N = Tk->nd;
  const int nn = fast_uniform(Pk->n_nodes), nw = fast_uniform(Pk->node_words), nr = fast_uniform(Pk->n_res);
  const uint32_t cb = (uint32_t)fast_uniform((int)N.cursor[k]);
  if (cb >= (uint32_t)nw) return pick;
  const int64_t* rq = Pk->cls_requests + (size_t)k * nr;
  const int64_t r0 = (int64_t)W::uniform((uint64_t)rq[0]), r1 = nr > 1 ? (int64_t)W::uniform((uint64_t)rq[1]) : 0,
                r2 = nr > 2 ? (int64_t)W::uniform((uint64_t)rq[2]) : 0, r3 = nr > 3 ? (int64_t)W::uniform((uint64_t)rq[3]) : 0;
  int64_t* const rem = Sk->n_remaining; uint32_t* const cnt = Sk->n_npods;
  const int key0 = zg0 >= 0 ? (int)Mp->vkey[fast_uniform((int)st->zg[zg0].var)] : -1, key1 = zg1 >= 0 ? (int)Mp->vkey[fast_uniform((int)st->zg[zg1].var)] : -1;
  const uint8_t* const d0 = key0 >= 0 ? N.dom + (size_t)key0 * nn : nullptr;
  const uint8_t* const d1 = key1 >= 0 ? N.dom + (size_t)key1 * nn : nullptr;
  uint64_t* const arow = N.alive + (size_t)k * nw;
  uint32_t newcur = (uint32_t)nw;   // the first block that still has a live node once this pod is through
  LaneVar<int64_t> v0, v1, v2, v3;
  LaneVar<uint64_t> hwv;
  LaneVar<uint32_t> cv, z0v, z1v;
  for (int b0 = (int)cb; b0 < nw && pick.node < 0; b0 += 64) {
    // the alive words of 64 blocks, one per lane: only the blocks with a live node are visited
    LaneVar<uint64_t> awv;
    const uint64_t live = W::ballot([&](int l) { const uint64_t w = b0 + l < nw ? arow[b0 + l] : 0ull; awv.at(l) = w; return w != 0; });
    for (uint64_t m = live; m && pick.node < 0; m &= m - 1) {
      const int j = ctz64(m), b = b0 + j, nb = b * 64;
      const uint64_t aw = awv.bcast(j);
      uint64_t mono = 0, cand = 0;
      W::ballot2([&](int l) {
        const int e = nb + l < nn ? nb + l : nn - 1;   // (the lanes past the last node read it again; their alive bits are zero)
        int64_t v = rem[e]; v0.at(l) = v;
        bool ok = ((aw >> l) & 1) && v >= 0 && r0 <= v;                              // resources.Fits (existingnode.go:96)
        if (nr > 1) { v = rem[(size_t)nn + e]; v1.at(l) = v; ok = ok && v >= 0 && r1 <= v; }
        if (nr > 2) { v = rem[(size_t)2 * nn + e]; v2.at(l) = v; ok = ok && v >= 0 && r2 <= v; }
        if (nr > 3) { v = rem[(size_t)3 * nn + e]; v3.at(l) = v; ok = ok && v >= 0 && r3 <= v; }
        const uint64_t hw = N.hword[e]; hwv.at(l) = hw; cv.at(l) = cnt[e];
        ok = ok && (((hlim - hw) & kTopoGuard) == kTopoGuard);                       // every hostname group: count + self <= limit
        const uint32_t z0 = d0 ? d0[e] : 0u, z1 = d1 ? d1[e] : 0u;
        z0v.at(l) = z0; z1v.at(l) = z1;
        const bool dm = (!d0 || (z0 < (uint32_t)kTopoMaxDom && ((vm0 >> z0) & 1u))) && (!d1 || (z1 < (uint32_t)kTopoMaxDom && ((vm1 >> z1) & 1u)));
        return (ok ? 1 : 0) | (ok && dm ? 2 : 0);
      }, mono, cand);
      if (mono != aw) W::store(&arow[b], mono);   // these tests only move towards rejection: failed for good
      if (mono && newcur == (uint32_t)nw) newcur = (uint32_t)b;
      if (cand) {
        const int wl = ctz64(cand), node = nb + wl;
        pick.node = node; pick.slot = cv.bcast(wl);
        uint64_t hinc_n = hinc, zsel_n = zsel;   // what Record counts on THIS node
        if constexpr (FILT::on) if (filt.fs) { const TopoFiltCut cut = topo_node_filter_cut<W>(Pk, Sk, Mp, filt, node); hinc_n &= ~cut.h; zsel_n &= ~cut.z; }
        // ExistingNode.Add (existingnode.go:172-185), by the node's own lane from the values it has just read
        W::each([&](int l) {
          if (l == wl) {
            rem[node] = v0.at(l) - r0;
            if (nr > 1) rem[(size_t)nn + node] = v1.at(l) - r1;
            if (nr > 2) rem[(size_t)2 * nn + node] = v2.at(l) - r2;
            if (nr > 3) rem[(size_t)3 * nn + node] = v3.at(l) - r3;
            cnt[node] = cv.at(l) + 1;
            N.hword[node] = topo_host_add(hwv.at(l), hinc_n);
          }
        });
        // Record (topology.go:197-220) on every dictionary-key group that counts the pod: the node's one domain
        const uint32_t zw0 = z0v.bcast(wl), zw1 = z1v.bcast(wl);
        for (uint64_t zs = zsel_n; zs; zs &= zs - 1) {
          KS_LDS TopoZg* const Z = &st->zg[ctz64(zs)];
          const int key = (int)Mp->vkey[fast_uniform((int)Z->var)];
          const uint32_t z = key == key0 ? zw0 : key == key1 ? zw1 : (uint32_t)fast_uniform((int)N.dom[(size_t)key * nn + node]);
          if (z < (uint32_t)kTopoMaxDom && W::leader()) { const int32_t c = Z->cnt[z]; Z->cnt[z] = c + 1; if (c == 0) Z->nonzero = Z->nonzero + 1; Z->dom = Z->dom | (1u << z); }
        }
      }
    }
  }
  if (newcur != cb) W::store(&N.cursor[k], newcur);
  W::sync();
  return pick;
}

}  // namespace ks
