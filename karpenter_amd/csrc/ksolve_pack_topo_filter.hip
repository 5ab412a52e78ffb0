// ksolve_pack_topo_filter.hip — the spread engine (topo_engine.h) that evaluates topology node filters which can say no (engines
// 24 / 25, FastWork::filt on a spread handle; "Topology node filters" in topo_engine.h): the engine without and with existing nodes,
// compiled with the filters' shape check, their static verdicts, the filter slots and the test at the Record sites (TopoEngine's FS),
// and with everything engines 22 / 23 keep (US). A unit of its own, so that the kernels every other setting runs are compiled
// without that code and keep their object.
#include "pack_kernels.h"

#include "topo_engine.h"

__global__ void __launch_bounds__(64) ksolve_pack_topo_f(const ks::TopoArgs* a) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  ks::TopoEngine<ks::Wave, false, true, true> eng(&a->pv, &a->ws, &a->fw, &a->tw, lds);
  eng.solve();
}
__global__ void __launch_bounds__(64) ksolve_pack_topo_nodes_f(const ks::TopoArgs* a) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  ks::TopoEngine<ks::Wave, true, true, true> eng(&a->pv, &a->ws, &a->fw, &a->tw, lds);
  eng.solve();
}
