// fast_cold_probe.h — TEST BUILDS ONLY (-DKSOLVE_TEST_HOOKS: tests/emu/libksolve_hooks.so, tests/emu/libksolve_emu.so; nothing of it is
// in the product): the cold half of the cursor engine (fast_engine.h FastCold) alone, one wavefront. The body constructs the FastCold the
// product's kernels construct, over an LDS segment laid out by the product's plan, calls setup() and then runs a SCRIPT of operations,
// one record each, every answer and every table the operations leave written to HBM for the host to download. The device kernels
// that instantiate it are in ksolve_test_fast_cold.hip, the emulation's twin is the same body on the loop-over-lanes Wave.
// tests/fast_cold_cases.py holds the definition the answers are compared with.
#pragma once
#ifdef KSOLVE_TEST_HOOKS
#include "fast_engine.h"

namespace ks {

enum {
  FCOP_ENTRY = 1,      // create_entry(vm)
  FCOP_FITS = 2,       // fast_lookup(vm), fast_fits(entry, req, size) when it is cached, fast_fields_ok(vm, dmask)
  FCOP_CELLS = 3,      // offering_cells(vm)
  FCOP_COMPAT = 4,     // compat_word(vm, t_its row of vm's id, w) for every word w
  FCOP_DIAG = 5,       // filter_diag(vm, size) — the keep flavours only
  FCOP_SLOT = 6,       // new_slot(k)
  FCOP_NEWCLAIM = 7,   // new_claim(F.cls[k], k, n_claims, retry)
  FCOP_ADD = 8         // a pod of class k joins claim x (state as the loop's commit writes it), refresh_claim(x)
};
struct FastColdOp { uint32_t op; int32_t k; int32_t x; int32_t retry; uint64_t vm, dmask; int32_t req[4], size[4]; };   // 64 B
// ran: 1 the operation ran (0xA5A5A5A5 stays where the script had ended before). ret: the call's return value (FITS: fast_lookup's).
// aux: FITS bit 0 fast_fits, bit 1 fast_fields_ok; CELLS the cells; NEWCLAIM us_err_ | us_diag_ << 8 (keep flavours). bail: bail_code behind it.
struct FastColdRes { int32_t ran, ret, bail, pad; uint64_t aux; };
struct FastColdScal {
  int32_t setup_ret, nv, n_ent, n_pool, n_claims, bail_code;
  uint32_t active_templates, host_seq, po_on, dne_vars, us_epoch;
  int32_t ops_run;
};
struct FastColdArgs {
  FastArgs fa;
  const FastColdOp* ops; int n_ops;
  FastColdRes* res;       // [n_ops]
  uint64_t* compat;       // [n_ops][it_words], written by FCOP_COMPAT
  FastColdScal* scal;     // [2]: behind setup(), behind the script
  uint64_t* misc;         // [2][sizeof(FastMisc) / 8]: FastMisc behind setup(), behind the script
  uint64_t* ent;          // [kFastEnt][4] the requirement-set cache behind the script
  int32_t* pool;          // [kFastPool][4]
  uint64_t* rec;          // [cap][3 + R] the claims' records (state, acceptance words) of the claims created
  uint64_t* aslot;        // [64 R][5] the class slots' records
  uint32_t* scls;         // [kFastRows][64] FastHot::scls
  uint32_t* cur;          // [kFastRows][64] FastHot::cur
};

template <class W, int GS, int R, bool US, bool PO>
KS_DEV void fast_cold_probe_body(const FastColdArgs* a, char* lds) {
  FastCold<W, GS, R, US, PO> cold;
  const ProblemView& P = a->fa.pv; const Workspace& S = a->fa.ws; const FastWork& F = a->fa.fw;
  cold.init(&P, &S, &F, lds);
  KS_LDS FastHot* const h = fast_uniform(cold.hs);
  W::each([&](int l) { for (int j = 0; j < kFastRows; ++j) { h->cur[j][l] = 0; h->scls[j][l] = kFastFree; } });   // as FastEngine::solve() starts
  W::sync();
  const int why = (int)W::uniform((uint64_t)(uint32_t)cold.setup());
  auto scalars = [&](int i, int ops_run) {
    FastColdScal s{};
    s.setup_ret = why; s.nv = cold.nv; s.n_ent = cold.n_ent; s.n_pool = cold.n_pool; s.n_claims = cold.n_claims; s.bail_code = cold.bail_code;
    s.active_templates = cold.active_templates; s.host_seq = cold.host_seq; s.ops_run = ops_run;
    if constexpr (PO) { s.po_on = (uint32_t)cold.po_on; s.dne_vars = cold.dne_vars; }
    if constexpr (US) s.us_epoch = cold.us_epoch;
    if (W::leader()) a->scal[i] = s;
  };
  auto misc = [&](int i) {
    const KS_LDS u64_alias* src = (const KS_LDS u64_alias*)cold.Mp;
    uint64_t* dst = a->misc + (size_t)i * (sizeof(FastMisc) / 8);
    W::for_n((int)(sizeof(FastMisc) / 8), [&](int w) { dst[w] = src[w]; });
  };
  scalars(0, 0); misc(0);
  W::sync();
  if (why) { scalars(1, 0); misc(1); W::sync(); return; }
  const int iw = P.it_words, n_ops = a->n_ops;
  int run = 0;
  for (int i = 0; i < n_ops; ++i) {
    const FastColdOp op = a->ops[i];
    const uint32_t what = (uint32_t)W::uniform((uint64_t)op.op);
    const uint64_t vm = W::uniform(op.vm);
    const int t = (int)(vm >> 56);
    const int tr = F.lim ? (int)F.lim->real[t] : t;
    FastColdRes r{};
    r.ran = 1;
    bool stop = false;
    // (a requirement set may name a limit stage only once the kernel has handed its id out: the template behind an id is FastLimits::real)
    if (what <= FCOP_DIAG && t >= (F.lim ? (int)F.lim->n_ids : P.n_templates)) { r.ret = -3; stop = true; }
    else if (what == FCOP_ENTRY) {
      r.ret = (int)W::uniform((uint64_t)(uint32_t)cold.create_entry(vm));
      stop = r.ret < 0;
    } else if (what == FCOP_FITS) {
      FastEnt e;
      r.ret = fast_lookup(cold.ent, vm, e);
      r.aux = (uint64_t)((r.ret >= 0 && fast_fits(cold.pool, e, op.req, op.size)) ? 1 : 0) | (uint64_t)(fast_fields_ok(vm, op.dmask) ? 2 : 0);
    } else if (what == FCOP_CELLS) {
      r.aux = cold.offering_cells(vm, t, tr);
    } else if (what == FCOP_COMPAT) {
      const uint64_t* tits = S.t_its + (size_t)t * iw;
      uint64_t* out = a->compat + (size_t)i * iw;
      W::for_n(iw, [&](int w) { out[w] = cold.compat_word(vm, tits, w); });
    } else if (what == FCOP_DIAG) {
      if constexpr (US) r.ret = (int)W::uniform((uint64_t)(uint32_t)cold.filter_diag(vm, op.size)); else { r.ret = -3; stop = true; }
    } else if (what == FCOP_SLOT) {
      r.ret = (int)W::uniform((uint64_t)(uint32_t)cold.new_slot(op.k));
      stop = r.ret < 0;
    } else if (what == FCOP_NEWCLAIM) {
      const FastSlot cs = F.cls[op.k];
      r.ret = (int)W::uniform((uint64_t)(uint32_t)cold.new_claim(cs, op.k, cold.n_claims, op.retry != 0));
      if constexpr (US) if (r.ret == 2) r.aux = (uint64_t)(uint32_t)cold.us_err_ | ((uint64_t)(uint32_t)cold.us_diag_ << 8);
      stop = r.ret == 0;
    } else if (what == FCOP_ADD) {
      if (op.x < 0 || op.x >= cold.n_claims) { r.ret = -3; stop = true; }   // (the script names a claim that was not created)
      else {
        // NodeClaim.Add as the loop's commit writes it: the class's values ANDed into the set, its requests added
        const FastSlot cs = F.cls[op.k];
        FastClaim st = cold.cst.state((uint32_t)op.x);
        st.vmask &= cs.cvmask;
        for (int q = 0; q < 4; ++q) st.req[q] += cs.size[q];
        if (W::leader()) cold.cst.put_state((uint32_t)op.x, st);
        W::sync();
        r.ret = (int)W::uniform((uint64_t)(uint32_t)cold.refresh_claim(op.x));
        stop = r.ret < 0;
      }
    } else { r.ret = -3; stop = true; }
    r.bail = cold.bail_code;
    if (W::leader()) a->res[i] = r;
    ++run;
    if (stop || cold.bail_code) break;
  }
  W::sync();
  scalars(1, run); misc(1);
  {
    const KS_LDS u64_alias* src = (const KS_LDS u64_alias*)cold.ent;
    uint64_t* dst = a->ent;
    W::for_n(kFastEnt * 4, [&](int w) { dst[w] = src[w]; });
    const KS_LDS int32_t* ps = cold.pool; int32_t* pd = a->pool;
    W::for_n(kFastPool * 4, [&](int w) { pd[w] = ps[w]; });
    const KS_LDS u64_alias* ss = (const KS_LDS u64_alias*)cold.aslot; uint64_t* sd = a->aslot;
    W::for_n(64 * R * 5, [&](int w) { sd[w] = ss[w]; });
    uint32_t* sc = a->scls; uint32_t* cu = a->cur;
    W::each([&](int l) { for (int j = 0; j < kFastRows; ++j) { sc[j * 64 + l] = h->scls[j][l]; cu[j * 64 + l] = h->cur[j][l]; } });
    const int nc = cold.n_claims;
    uint64_t* rd = a->rec;
    const typename FastMem<GS, R>::States cs_ = cold.cst;
    W::for_n(nc, [&](int c) {
      const FastClaim st = cs_.state((uint32_t)c);
      const u64_alias* s3 = (const u64_alias*)&st;
      for (int q = 0; q < 3; ++q) rd[(size_t)c * (3 + R) + q] = s3[q];
      for (int j = 0; j < R; ++j) rd[(size_t)c * (3 + R) + 3 + j] = cs_.acc((uint32_t)c, j);
    });
  }
  W::sync();
}

}  // namespace ks
#endif
