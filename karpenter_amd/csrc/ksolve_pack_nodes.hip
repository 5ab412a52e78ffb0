// ksolve_pack_nodes.hip — the cursor engine's existing-node stage (node_stage.h): one wavefront places the queue's pods on the
// existing nodes, first fit with a cursor per pod class, in front of the cursor loop (ksolve_pack_fast.hip). Two variants: the
// nodes' remaining resources and pod counts in LDS (while they fit ks::kNodeStageLdsRem), or in the HBM workspace.
#include "pack_kernels.h"

__global__ void __launch_bounds__(64) ksolve_pack_nodes_lds(const ks::FastArgs* a) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  ks::pack_nodes_body<ks::Wave, false>(a, lds);
}
__global__ void __launch_bounds__(64) ksolve_pack_nodes_hbm(const ks::FastArgs* a) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  ks::pack_nodes_body<ks::Wave, true>(a, lds);
}
