// ksolve_pack_topo_podops.hip — the spread engine (topo_engine.h) that takes pod classes and topology node-filter terms with NotIn,
// Exists and DoesNotExist (engines 29 / 30, FastWork::podops on a spread handle; "The spread engine's pod operators" in
// topo_engine.h): the engine without and with existing nodes, compiled with the phantom value on top of every field of the packed
// requirement word, the widened filter terms and their test at the Record sites (TopoEngine's PO), and with everything engines
// 24 / 25 evaluate (FS, US). A unit of its own, so that the kernels every other setting runs are compiled without that code and keep
// their object.
#include "pack_kernels.h"

#include "topo_engine.h"

__global__ void __launch_bounds__(64) ksolve_pack_topo_p(const ks::TopoArgs* a) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  ks::TopoEngine<ks::Wave, false, true, true, true> eng(&a->pv, &a->ws, &a->fw, &a->tw, lds);
  eng.solve();
}
__global__ void __launch_bounds__(64) ksolve_pack_topo_nodes_p(const ks::TopoArgs* a) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  ks::TopoEngine<ks::Wave, true, true, true, true> eng(&a->pv, &a->ws, &a->fw, &a->tw, lds);
  eng.solve();
}
