// node_stage.h — the cursor engine's existing-node stage: addToExistingNode (scheduler.go:614-656) for every pod of the queue, as
// a pass of its own IN FRONT of the cursor loop (fast_engine.h), which then solves the pods no node took.
//
// Why the stage separates from the loop. For the cursor engine's shape (operators In only, no topology, host ports, volumes or
// bounds; node labels single-valued In sets) whether a pod lands on an existing node depends on node state alone, and node
// state changes only when earlier pods land on nodes: the in-flight NodeClaims never enter. More than that:
//   * ExistingNode.Add (existingnode.go:172-185) intersects the node's single-valued sets with a positive pod set and so leaves
//     them as they were; a key the node lacks rejects the pod (requirements.go:185-193). The (class, node) verdict up to
//     resources is therefore STATIC: exactly the rows ksolve_node_dead0 (kernels.h, nodecheck.h) computes for resident clusters.
//     They are computed with every solve's classes (FastWork::nd_dead0): class ids are not stable from solve to solve.
//   * the one dynamic check is resources.Fits against `remaining` (existingnode.go:96), which only shrinks: a node that has
//     rejected a class has rejected it for good.
// So each class keeps a cursor — the first 64-node block that can still hold it — and the block's alive bits (the static row's
// word less the nodes that have failed the class since): a pod costs one ballot over the block, one lane per node, lowest set bit
// wins (scheduler.go:639). A pod the reference would place on a node never reaches sort.Slice (scheduler.go:598), so taking
// these pods out of the queue leaves the claims' order, and with it every later decision of the loop, as it was.
//
// One wavefront. Per-solve state: cursors and current alive words by class in LDS; `remaining` and the nodes' pod counts in LDS
// while n_nodes x n_res x 8 bytes fit kNodeStageLdsRem (and the classes fit beside them), in the HBM workspace (Workspace::n_remaining / n_npods) otherwise —
// the kernel is compiled for both. Everything is reset at the start of every solve. Results leave in queue order, 64 entries per
// store, with plain vector stores: the node and slot of each entry, and the compacted queue of the entries left (their pod
// indices, in queue order); ksolve_fast_requeue (one thread per entry) scatters the former to the pods and rebuilds q_class /
// cls_first / cls_last for the latter.
#pragma once
#include "fast_engine.h"

namespace ks {

constexpr int kNodeStageLdsRem = 96 * 1024;   // bytes of `remaining` ([n_res][n_nodes] int64) the LDS variant holds; beyond: the HBM variant
constexpr int kNodeStageLdsClasses = 4096;    // cursor + alive word per class in LDS (12 B each) beside `remaining`; with more classes `remaining` goes to HBM ...
constexpr int kNodeStageMaxClasses = 12288;   // ... and the classes have the LDS to themselves; beyond: DECLINE_NODE_CLASSES (33)

// LDS layout (bytes): alive words [nc] u64 | cursors [nc] u32 | (LDS variant) pod counts [nn] u32 | remaining [nr][nn] i64
struct NodeStagePlan { int off_word, off_cur, off_npods, off_rem, total_bytes; };
KS_FN NodeStagePlan node_stage_plan(int nc, int nn, int nr, bool hbm) {
  NodeStagePlan p;
  p.off_word = 0;
  p.off_cur = nc * 8;
  p.off_npods = (p.off_cur + nc * 4 + 15) & ~15;
  p.off_rem = hbm ? p.off_npods : (p.off_npods + nn * 4 + 15) & ~15;
  p.total_bytes = hbm ? p.off_rem : p.off_rem + nr * nn * 8;
  return p;
}
KS_FN bool node_stage_hbm(int nc, int nn, int nr) { return (long long)nn * nr * 8 > (long long)kNodeStageLdsRem || nc > kNodeStageLdsClasses; }
static_assert(kNodeStageLdsClasses * 12 + kNodeStageLdsRem + kNodeStageLdsRem / 8 + 64 <= 160 * 1024 - 512 && kNodeStageMaxClasses * 12 + 64 <= 160 * 1024 - 512, "the node stage's LDS plans fit one CU");

template <bool HBM> struct NodeStageMem {
#if KS_DEVICE
  typedef typename std::conditional<HBM, int64_t*, KS_LDS int64_t*>::type rem_p;
  typedef typename std::conditional<HBM, uint32_t*, KS_LDS uint32_t*>::type cnt_p;
#else
  typedef int64_t* rem_p;
  typedef uint32_t* cnt_p;
#endif
};

// Pod operators beside existing nodes (engines 32 / 33; PO). A pod class with NotIn, Exists or DoesNotExist (In [] is DoesNotExist)
// meets a node whose label sets are single-valued In sets (reason 32 guarantees it):
//   * a key the node defines as In {a}: whatever is compatible intersects to In {a} again (requirements.go:133-140), so the node is
//     unchanged — In S passes iff a is in S, NotIn S iff a is not in S, Exists passes, DoesNotExist fails (requirements.go:254-274);
//   * a key the node lacks: In / Exists fail (requirements.go:189; existing nodes pass no AllowUndefined, existingnode.go:100),
//     NotIn / DoesNotExist pass, and ExistingNode.Add (existingnode.go:172-176) then writes the pod's requirement onto the node. Behind
//     a DoesNotExist pod a later In / Exists pod still fails (empty intersection, positive incoming operator) and a later NotIn /
//     DoesNotExist pod still passes (both sides negative, requirements.go:260-264): the verdicts are what they were. Behind a NotIn
//     [b] pod a later NotIn / DoesNotExist pod still passes — but an In [c] pod, c != b, or an Exists pod now PASSES where it failed.
// So the (class, node) verdict up to resources stays static — the rows of ksolve_node_dead0 (nodecheck.h, kneg) carry exactly these
// verdicts — but for one shape: a key some node lacks that carries both a NotIn class and an In (non-empty) or Exists class. The
// stage looks for it before any pod is placed, per key over all nodes and all classes (conservative, never optimistic), and hands the
// batch back with DECLINE_NODE_KEY_DEFINEDNESS. Otherwise the loop below is the one of the positive stage: `remaining` only shrinks.
template <class W, bool HBM, bool PO = false>
KS_DEV void pack_nodes_body(const FastArgs* a, char* lds) {
  const ProblemView& P = a->pv; const Workspace& S = a->ws; const FastWork& F = a->fw;
  const Dict& d = P.dict;
  const int np = fast_uniform(P.n_pods), nr = fast_uniform(P.n_res), nn = fast_uniform(P.n_nodes), nw = fast_uniform(P.node_words), nc = fast_uniform(P.n_classes);
  const NodeStagePlan pl = node_stage_plan(nc, nn, nr, HBM);
  KS_LDS uint64_t* const aword = (KS_LDS uint64_t*)(lds + pl.off_word);
  KS_LDS uint32_t* const acur = (KS_LDS uint32_t*)(lds + pl.off_cur);
  typename NodeStageMem<HBM>::rem_p rem;
  typename NodeStageMem<HBM>::cnt_p cnt;
  if constexpr (HBM) { rem = S.n_remaining; cnt = S.n_npods; }
  else { rem = (typename NodeStageMem<HBM>::rem_p)(lds + pl.off_rem); cnt = (typename NodeStageMem<HBM>::cnt_p)(lds + pl.off_npods); }
  const uint64_t* const dead0 = fast_uniform(F.nd_dead0);
  FastNodes out{};
  out.variant = HBM ? 2u : 1u;
  if constexpr (PO) {
    // ---- the shape with pod operators (above): three reductions, one verdict per key ----
    const ProblemView& Pv = P;
    const uint32_t* const ndef = S.n_defined0;
    const uint32_t all_keys = d.n_keys >= 32 ? 0xFFFFFFFFu : (1u << d.n_keys) - 1;
    auto keys_with = [&](bool notin) {
      return (uint32_t)W::reduce_or(nc, [&](int c) {
        const ReqRef cr = Pv.cls_reqs.at(d, c);
        uint64_t m = 0;
        for (uint32_t ks_ = cr.defined; ks_; ks_ &= ks_ - 1) {
          const int k = __builtin_ctz(ks_);
          const int op = req_op(d, cr, k);
          if (notin ? op == OP_NOTIN : (op == OP_IN || op == OP_EXISTS)) m |= 1ull << k;
        }
        return m; });
    };
    const uint32_t k_notin = keys_with(true);       // keys some class uses with NotIn
    const uint32_t k_positive = keys_with(false);   // ... with In (non-empty) or Exists
    const uint32_t k_undef = (uint32_t)W::reduce_or(nn, [&](int e) { return (uint64_t)(~ndef[e] & all_keys); });   // keys some node leaves undefined
    if (k_notin & k_positive & k_undef) out.bail = DECLINE_NODE_KEY_DEFINEDNESS;
  } else
  // ---- the shape: the stage rests on positive pod sets (a NotIn / DoesNotExist pod may ADD a key to a node: not static; engines
  // 32 / 33 take such pods, above). The reasons are those of fast_engine.h setup(), which would find the same classes behind the stage ----
  {
    const ProblemView& Pv = P;
    if (W::reduce_or(nc, [&](int c) { return (uint64_t)Pv.cls_reqs.complement[c]; })) out.bail = DECLINE_CLASS_NOT_POSITIVE;
    else if (W::reduce_or(nc, [&](int c) {
      const uint64_t* cm = Pv.cls_reqs.mask + (size_t)c * d.req_words;
      uint64_t bad = 0;
      for (uint32_t ks_ = Pv.cls_reqs.defined[c]; ks_; ks_ &= ks_ - 1) {
        const int key = __builtin_ctz(ks_);
        uint64_t any = 0;
        for (uint32_t w = d.key_word_off[key]; w < d.key_word_off[key + 1]; ++w) any |= cm[w];
        if (!any) bad = 1;   // In [] == DoesNotExist
      }
      return bad;
    })) out.bail = DECLINE_CLASS_EMPTY_IN;
  }
  if (out.bail) {
    if (W::leader()) *F.nodes = out;
    W::sync();
    return;
  }
  // ---- per-solve state ----
  {
    const int64_t* rem0 = S.n_remaining0;
    W::for_n(nc, [&](int c) { aword[c] = ~dead0[(size_t)c * nw]; acur[c] = 0; });
    W::for_n(nr * nn, [&](int i) { rem[i] = rem0[i]; });
    W::for_n(nn, [&](int i) { cnt[i] = 0; });
  }
  W::sync();
  const long long ms = S.max_steps;
  const int K = (ms < 0 || ms >= (long long)np) ? np : (int)ms;   // a step is a queue pop: the first K entries are this solve's
  out.limit_hit = (ms >= 0 && ms < (long long)np) ? 1u : 0u;
  const uint32_t* const qcls = fast_uniform((const uint32_t*)F.q_class);
  const uint32_t* const sorted = fast_uniform(P.sorted_pods);
  const int64_t* const creq = fast_uniform(P.cls_requests);
  uint32_t* const qnode = fast_uniform(F.q_claim); uint32_t* const qslot = fast_uniform(F.q_cnt); uint32_t* const left_pod = fast_uniform(F.nd_pod);
  uint32_t curk = 0xFFFFFFFFu, cb = 0;   // the class whose cursor and alive word are in registers
  uint64_t caw = 0;
  unsigned long long n_ref = 0, n_tests = 0;
  uint32_t n_left = 0, n_placed = 0;
  for (int base = 0; base < K; base += 64) {
    const int bn = K - base < 64 ? K - base : 64;
    // the block's entries, a lane each: class, pod, the class's requests (one gather for the 64 of them)
    LaneVar<uint32_t> kv, podv, resv, slotv;
    LaneVar<int64_t> q0, q1, q2, q3;
    W::each([&](int l) {
      const int i = base + (l < bn ? l : bn - 1);
      const uint32_t k = qcls[i] & ~kFastLastBit;
      kv.at(l) = k; podv.at(l) = sorted[i]; resv.at(l) = 0xFFFFFFFFu; slotv.at(l) = 0;
      const int64_t* rq = creq + (size_t)k * nr;
      q0.at(l) = rq[0]; q1.at(l) = nr > 1 ? rq[1] : 0; q2.at(l) = nr > 2 ? rq[2] : 0; q3.at(l) = nr > 3 ? rq[3] : 0;
    });
    for (int j = 0; j < bn; ++j) {
      const uint32_t k = kv.bcast(j);
      const int64_t r0 = q0.bcast(j), r1 = q1.bcast(j), r2 = q2.bcast(j), r3 = q3.bcast(j);
      if (k != curk) {
        if (curk != 0xFFFFFFFFu && W::leader()) { aword[curk] = caw; acur[curk] = cb; }
        W::order();
        curk = k;
        caw = W::uniform(aword[k]); cb = (uint32_t)fast_uniform((int)acur[k]);
      }
      int node = -1;
      while (cb < (uint32_t)nw) {
        if (caw == 0) {
          // the block is exhausted for this class: the next one with a node that may still hold it
          const uint64_t* row = dead0 + (size_t)k * nw;
          cb = (uint32_t)W::find_first((int)cb + 1, nw, [&](int w) { return ~row[w] != 0; });
          if (cb < (uint32_t)nw) caw = W::uniform(~row[cb]);
          continue;
        }
        // resources.Fits (existingnode.go:96): one lane per node of the block
        const int nb = (int)cb * 64;
        const uint64_t aw = caw;
        const uint64_t ok = W::ballot([&](int l) {
          if (!((aw >> l) & 1)) return false;
          const int e = nb + l;
          int64_t v = rem[e];
          bool fit = v >= 0 && r0 <= v;
          if (nr > 1) { v = rem[(size_t)nn + e]; fit = fit && v >= 0 && r1 <= v; }
          if (nr > 2) { v = rem[(size_t)2 * nn + e]; fit = fit && v >= 0 && r2 <= v; }
          if (nr > 3) { v = rem[(size_t)3 * nn + e]; fit = fit && v >= 0 && r3 <= v; }
          return fit;
        });
        n_tests += (unsigned long long)popc64(aw);
        caw = ok;   // `remaining` only shrinks: the nodes that failed the class have failed it for good
        if (ok) { node = nb + ctz64(ok); break; }
      }
      if (node >= 0) {
        // ExistingNode.Add (existingnode.go:172-185): remaining -= requests; the pod's slot is the node's count before it
        const uint32_t slot = (uint32_t)fast_uniform((int)cnt[node]);
        const int wl = node & 63;
        W::each([&](int l) {
          if (l == wl) {
            rem[node] -= r0;
            if (nr > 1) rem[(size_t)nn + node] -= r1;
            if (nr > 2) rem[(size_t)2 * nn + node] -= r2;
            if (nr > 3) rem[(size_t)3 * nn + node] -= r3;
            cnt[node] = slot + 1;
          }
          if (l == j) { resv.at(l) = (uint32_t)node; slotv.at(l) = slot; }
        });
        if constexpr (HBM) W::sync(); else W::order();
        n_ref += (unsigned long long)(node + 1);   // the reference evaluated the nodes up to and including the winner ...
        n_placed++;
      } else n_ref += (unsigned long long)nn;       // ... or every node
    }
    // the block's results in queue order; the entries no node took go to the compacted queue, in queue order
    const uint64_t leftm = W::ballot([&](int l) { return l < bn && resv.at(l) == 0xFFFFFFFFu; });
    const uint32_t lbase = n_left;
    W::each([&](int l) {
      if (l < bn) {
        qnode[base + l] = resv.at(l); qslot[base + l] = slotv.at(l);
        if ((leftm >> l) & 1) left_pod[lbase + (uint32_t)popc64(leftm & ((1ull << l) - 1))] = podv.at(l);
      }
    });
    n_left += (uint32_t)popc64(leftm);
  }
  if constexpr (!HBM) {   // Results.node_npods is read from the workspace
    uint32_t* gc = S.n_npods;
    W::for_n(nn, [&](int i) { gc[i] = cnt[i]; });
  }
  out.n_left = n_left; out.n_placed = n_placed; out.n_ref = n_ref; out.n_tests = n_tests;
  if (W::leader()) *F.nodes = out;
  W::sync();
}

// ksolve_fast_requeue — one thread per entry of the FULL queue, behind ksolve_pack_nodes: the entry's node under its pod index
// (Results.pod_assignment = -2 - node, pod_slot), then entry i of the COMPACTED queue as ksolve_fast_queue builds it (class, "not
// placed", the class's first / last entry; a.q.sorted = FastWork::nd_pod). Entries past the compacted queue read "not placed".
// ksolve_fast_remark — kFastLastBit over the compacted queue.
// pod_qpos (engines 20 / 21, FastWork::pod_qpos; null otherwise): every pod's position in the full queue, which the loop needs for
// the reference's queue lengths when it sets a pod aside.
struct FastRequeueArgs { FastQueueArgs q; const uint32_t* full_sorted; const FastNodes* nodes; uint32_t* pod_qpos; };
KS_DEV void fast_requeue_body(int i, const FastRequeueArgs& a) {
  if (a.pod_qpos) a.pod_qpos[a.full_sorted[i]] = (uint32_t)i;
  const uint32_t e = a.q.q_claim[i];
  if (e != 0xFFFFFFFFu) { const uint32_t p = a.full_sorted[i]; a.q.assign[p] = -2 - (int32_t)e; a.q.slot[p] = a.q.q_cnt[i]; }
  if ((uint32_t)i < a.nodes->n_left) fast_queue_body(i, a.q);
  else a.q.q_claim[i] = 0xFFFFFFFFu;
}
KS_FN void fast_remark_body(int i, const FastRequeueArgs& a) {
  if ((uint32_t)i < a.nodes->n_left) fast_mark_body(i, a.q);
}

}  // namespace ks
