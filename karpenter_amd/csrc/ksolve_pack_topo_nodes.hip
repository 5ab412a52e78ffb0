// ksolve_pack_topo_nodes.hip — the spread engine (topo_engine.h) for a problem with existing nodes: every pod is offered to the
// nodes first, inside the engine's per-pod step (topo_nodes.h). A translation unit of its own, so that ksolve_pack_topo — the
// kernel every problem without nodes runs — is compiled from exactly what it was compiled from before.
#include "pack_kernels.h"

#include "topo_engine.h"

__global__ void __launch_bounds__(64) ksolve_pack_topo_nodes(const ks::TopoArgs* a) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  ks::TopoEngine<ks::Wave, true> eng(&a->pv, &a->ws, &a->fw, &a->tw, lds);
  eng.solve();
}
