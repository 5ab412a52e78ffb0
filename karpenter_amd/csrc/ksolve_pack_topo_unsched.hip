// ksolve_pack_topo_unsched.hip — the spread engine (topo_engine.h) that KEEPS unschedulable pods and retries them (engines 22 / 23,
// FastWork::unsched on a spread handle; "The spread engine's unschedulable pods" in topo_engine.h): the engine without and with
// existing nodes, compiled with the set-aside list, the error computation, the kept verdicts and the second round (TopoEngine's US).
// A unit of its own, so that the kernels every other setting runs are compiled without that code and keep their object.
#include "pack_kernels.h"

#include "topo_engine.h"

__global__ void __launch_bounds__(64) ksolve_pack_topo_u(const ks::TopoArgs* a) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  ks::TopoEngine<ks::Wave, false, true> eng(&a->pv, &a->ws, &a->fw, &a->tw, lds);
  eng.solve();
}
__global__ void __launch_bounds__(64) ksolve_pack_topo_nodes_u(const ks::TopoArgs* a) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  ks::TopoEngine<ks::Wave, true, true> eng(&a->pv, &a->ws, &a->fw, &a->tw, lds);
  eng.solve();
}
