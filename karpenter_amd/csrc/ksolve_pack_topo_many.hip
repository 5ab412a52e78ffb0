// ksolve_pack_topo_many.hip — the spread engine (topo_engine.h), many problems per launch (topo_many.h): the many-problem forms of
// ksolve_pack_topo and ksolve_pack_topo_nodes. A unit of its own, so that the single-problem kernels keep their objects.
#include "pack_kernels.h"

#include "topo_engine.h"
#include "topo_many.h"

__global__ void __launch_bounds__(64) ksolve_pack_topo_many(const ks::TopoArgs* const* items, const uint32_t* order, uint32_t* next, int n) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const ks::TopoArgs* a = ks::topo_many_take(items, order, next, n);
  if (!a) return;
  ks::TopoEngine<ks::Wave> eng(&a->pv, &a->ws, &a->fw, &a->tw, lds);
  eng.solve();
}
__global__ void __launch_bounds__(64) ksolve_pack_topo_nodes_many(const ks::TopoArgs* const* items, const uint32_t* order, uint32_t* next, int n) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const ks::TopoArgs* a = ks::topo_many_take(items, order, next, n);
  if (!a) return;
  ks::TopoEngine<ks::Wave, true> eng(&a->pv, &a->ws, &a->fw, &a->tw, lds);
  eng.solve();
}
