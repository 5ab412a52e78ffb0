// ksolve_pack_nodes.hip — the cursor engine's existing-node stage (node_stage.h): one wavefront places the queue's pods on the
// existing nodes, first fit with a cursor per pod class, in front of the cursor loop (ksolve_pack_fast.hip). Two variants: the
// nodes' remaining resources and pod counts in LDS (while they fit ks::kNodeStageLdsRem), or in the HBM workspace. Each again with
// the stage's pod operators compiled in (_p; engines 32 / 33, node_stage.h "Pod operators beside existing nodes"): kernels of their
// own, so that the two every other setting runs keep their code.
#include "pack_kernels.h"

__global__ void __launch_bounds__(64) ksolve_pack_nodes_lds(const ks::FastArgs* a) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  ks::pack_nodes_body<ks::Wave, false>(a, lds);
}
__global__ void __launch_bounds__(64) ksolve_pack_nodes_hbm(const ks::FastArgs* a) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  ks::pack_nodes_body<ks::Wave, true>(a, lds);
}
__global__ void __launch_bounds__(64) ksolve_pack_nodes_lds_p(const ks::FastArgs* a) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  ks::pack_nodes_body<ks::Wave, false, true>(a, lds);
}
__global__ void __launch_bounds__(64) ksolve_pack_nodes_hbm_p(const ks::FastArgs* a) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  ks::pack_nodes_body<ks::Wave, true, true>(a, lds);
}
