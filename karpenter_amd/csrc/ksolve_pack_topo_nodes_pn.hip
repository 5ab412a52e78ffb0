// ksolve_pack_topo_nodes_pn.hip — the spread engine with existing nodes AND the pod operators kept on beside them (engines 35 / 36;
// topo_nodes.h, "Pod operators beside existing nodes on the spread engine"): TopoEngine's NP on top of the PodOps flavour with nodes.
// One kernel outside the flavour matrix of pack_flavours.h (kPackTopoNodesPodOpsNodes, as ksolve_pack_nodes_lds_p is outside the
// cursor engine's), in a unit of its own that is compiled without -D flags, so that the objects of ksolve_pack_topo.hip — the kernels
// every other setting runs — are compiled from what they were compiled from.
#include "pack_kernels.h"

#include "topo_engine.h"

__global__ void __launch_bounds__(64) ksolve_pack_topo_nodes_pn(const ks::TopoArgs* a) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  constexpr ks::TopoFlavour fl = ks::TopoFlavour::PodOps;
  ks::TopoEngine<ks::Wave, true, ks::flavour_us(fl), ks::flavour_fs(fl), ks::flavour_po(fl), true> eng(&a->pv, &a->ws, &a->fw, &a->tw, lds);
  eng.solve();
}
