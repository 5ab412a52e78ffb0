// emu_launches.h — TEST ONLY: the host emulation's launches of the node kernels, of the spread engine with existing nodes and of its
// many-problem form, the effective-allocatable launch and the emulation's export of ksolve_solve_many. Included by ksolve_impl.h at
// its end, and only under KSOLVE_HOST_EMULATION (tests/emu/ksolve_emu.cpp, which holds the rest of the emulation's backend): these
// pieces reach into ksi:: internals (fast_requeue_args, topo_many_order, solve_many) and an emulation backend that does not define
// them itself still links. Never part of the product library.
#pragma once
#ifndef KSOLVE_HOST_EMULATION
#error "emu_launches.h belongs to the host emulation"
#endif
#include "topo_engine.h"

// (the emulation's launch is the loop over the grid)
static void be_launch_eff_alloc(ksolve_handle*, const ks::EffAllocArgs& a) { for (int t = 0; t < a.n_templates; ++t) for (int it = 0; it < a.n_its; ++it) ks::eff_alloc_body(t, it, a); }
// The node kernels: a kernel launch is a loop over its grid.
static void be_launch_pack_nodes(ksolve_handle* h, bool hbm, bool pod_ops) {
  const int lds_bytes = ks::node_stage_plan((int)h->n_classes, (int)h->n_nodes, (int)h->n_res, hbm).total_bytes;
  std::vector<char> lds((size_t)lds_bytes + 64, (char)0xA5);   // garbage, like the device's LDS at kernel start
  ks::FastArgs a{h->pv, h->ws, h->fw};
  be_h2d(h, h->d_fast_args, &a, sizeof(a));
  note_pack_kernel(h, ks::pack_nodes_kernel(hbm, pod_ops));   // the kernel the device backend launches, from the same lookup
  if (pod_ops) {
    if (hbm) ks::pack_nodes_body<ks::Wave, true, true>(h->d_fast_args, lds.data());
    else ks::pack_nodes_body<ks::Wave, false, true>(h->d_fast_args, lds.data());
  } else
  if (hbm) ks::pack_nodes_body<ks::Wave, true>(h->d_fast_args, lds.data());
  else ks::pack_nodes_body<ks::Wave, false>(h->d_fast_args, lds.data());
  const ks::FastRequeueArgs q = ksi::fast_requeue_args(h);
  for (int i = 0; i < (int)h->n_pods; ++i) ks::fast_requeue_body(i, q);
  for (int i = 0; i < (int)h->n_pods; ++i) ks::fast_remark_body(i, q);
}
static void be_launch_fast_unsched(ksolve_handle* h) {
  const ks::FastUnschedArgs a = ksi::fast_unsched_args(h);
  for (int i = 0; i < (int)h->n_pods; ++i) ks::fast_unsched_body(i, a);
}
static void be_launch_pack_topo_nodes(ksolve_handle* h) {
  std::vector<char> lds((size_t)h->tw.plan.total_bytes + 64, (char)0xA5);
  ks::TopoArgs a{h->pv, h->ws, h->fw, h->tw};
  be_h2d(h, h->d_topo_args, &a, sizeof(a));
  const ks::TopoArgs* a_ = h->d_topo_args;
  note_pack_kernel(h, ks::pack_topo_nodes_kernel(ks::topo_flavour(h->fw), spread_nodes_pn(h)));   // the kernel the device backend launches, from the same lookup (the one engine here has NP built in; FastWork::node_podops decides)
  ks::TopoEngine<ks::Wave, true> eng(&a_->pv, &a_->ws, &a_->fw, &a_->tw, lds.data());
  eng.solve();
}
// The emulated ksolve_pack_topo*_many launches (topo_many.h): a loop over the grid in which every block takes a ticket from the
// launch's counter and solves the member the order table names, one after another; the LDS segment is the launch's (the largest
// member's plan), each engine reading its own tw.plan offsets. (The emulation's engine has the set-aside list and the filters built in.)
static void be_launch_pack_topo_many(std::vector<ksolve_handle*>* groups) {
  for (int f = 0; f < ks::kTopoManyFlavours; ++f) {   // f: the row of ks::kPackTopoManyRows
    std::vector<ksolve_handle*>& g = groups[f];
    if (g.empty()) continue;
    const uint32_t n = (uint32_t)g.size();
    std::vector<uint32_t> order(n);
    int lds_bytes = 0;
    for (ksolve_handle* h : g) {
      ks::TopoArgs a{h->pv, h->ws, h->fw, h->tw};
      be_h2d(h, h->d_topo_args, &a, sizeof(a));
      note_pack_kernel(h, ks::kPackTopoManyRows[f].kernel);
      lds_bytes = std::max(lds_bytes, h->tw.plan.total_bytes);
    }
    ksi::topo_many_order(g, order.data());
    uint32_t next = 0;   // the launch's ticket counter
    be_tic(g[0], ksi::T_PACK);
    for (uint32_t block = 0; block < n; ++block) {
      const uint32_t t = next++;
      if (t >= n || order[t] >= n) continue;
      const ks::TopoArgs* a_ = g[order[t]]->d_topo_args;
      std::vector<char> lds((size_t)lds_bytes + 64, (char)0xA5);   // garbage, like the device's LDS at kernel start
      if (ks::kPackTopoManyRows[f].nodes) { ks::TopoEngine<ks::Wave, true> eng(&a_->pv, &a_->ws, &a_->fw, &a_->tw, lds.data()); eng.solve(); }
      else { ks::TopoEngine<ks::Wave> eng(&a_->pv, &a_->ws, &a_->fw, &a_->tw, lds.data()); eng.solve(); }
    }
    be_toc(g[0], ksi::T_PACK);
    for (ksolve_handle* h : g) h->timers.ms[ksi::T_PACK] = g[0]->timers.ms[ksi::T_PACK];
  }
}
// the emulation's export of ksolve_solve_many (its other exports live with its backend)
extern "C" ksolve_status ksolve_solve_many(ksolve_handle** hs, uint32_t n, ksolve_results* outs, ksolve_many_stats* stats) {
  if (!hs || !outs || n == 0) return KSOLVE_ERR_INVALID;
  return ksi::solve_many(hs, n, outs, stats);
}
