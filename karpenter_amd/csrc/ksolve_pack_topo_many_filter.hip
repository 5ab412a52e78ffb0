// ksolve_pack_topo_many_filter.hip — the spread engine that evaluates topology node filters (engines 24 / 25), many problems per
// launch (topo_many.h): the many-problem forms of ksolve_pack_topo_f and ksolve_pack_topo_nodes_f. A unit of its own.
#include "pack_kernels.h"

#include "topo_engine.h"
#include "topo_many.h"

__global__ void __launch_bounds__(64) ksolve_pack_topo_many_f(const ks::TopoArgs* const* items, const uint32_t* order, uint32_t* next, int n) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const ks::TopoArgs* a = ks::topo_many_take(items, order, next, n);
  if (!a) return;
  ks::TopoEngine<ks::Wave, false, true, true> eng(&a->pv, &a->ws, &a->fw, &a->tw, lds);
  eng.solve();
}
__global__ void __launch_bounds__(64) ksolve_pack_topo_nodes_many_f(const ks::TopoArgs* const* items, const uint32_t* order, uint32_t* next, int n) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const ks::TopoArgs* a = ks::topo_many_take(items, order, next, n);
  if (!a) return;
  ks::TopoEngine<ks::Wave, true, true, true> eng(&a->pv, &a->ws, &a->fw, &a->tw, lds);
  eng.solve();
}
