// ksolve_pack_topo.hip — the spread engine (topo_engine.h), compiled once per flavour (pack_flavours.h) with -DKS_PACK_FLAVOUR=<n>:
// every build defines the rows of its flavour in KS_PACK_TOPO_ROWS, in list order — the engine without and with existing nodes (every
// pod is offered to the nodes first, inside the engine's per-pod step: topo_nodes.h). An object per flavour, so that the kernels every
// other setting runs are compiled without a later switch's code and keep their object; the plain flavour is two objects,
// -DKS_PACK_NODES=0 and =1, so that ksolve_pack_topo — the kernel every problem without nodes runs — stands alone in its own.
#include "pack_kernels.h"

#include "topo_engine.h"

#ifndef KS_PACK_FLAVOUR
#error "ksolve_pack_topo.hip is compiled per flavour: -DKS_PACK_FLAVOUR=<TopoFlavour> [-DKS_PACK_NODES=<0|1>]"
#endif
// The spread engine (topo_engine.h): the cursor engine's shape plus topology spread / pod affinity on dictionary keys and spread /
// anti-affinity on the hostname — BASELINE configs[2]. One wavefront; claims in HBM (32 B each), the order's rings in HBM, the
// caches, the ring tables and the topology counters in LDS.
#define KS_PACK_TOPO_KERNEL(NAME, FL, ND)                                                                                      \
  __global__ void __launch_bounds__(64) NAME(const ks::TopoArgs* a) {                                                           \
    extern __shared__ __attribute__((aligned(16))) char lds[];                                                                  \
    ks::TopoEngine<ks::Wave, ND != 0, ks::flavour_us(ks::TopoFlavour::FL), ks::flavour_fs(ks::TopoFlavour::FL), ks::flavour_po(ks::TopoFlavour::FL)> \
        eng(&a->pv, &a->ws, &a->fw, &a->tw, lds);                                                                               \
    eng.solve();                                                                                                                \
  }
// a row without / with nodes: its kernel, or nothing in a build of the other nodes selector
#if !defined(KS_PACK_NODES)
#define KS_PACK_TOPO_0 KS_PACK_TOPO_KERNEL
#define KS_PACK_TOPO_1 KS_PACK_TOPO_KERNEL
#elif KS_PACK_NODES
#define KS_PACK_TOPO_0(NAME, FL, ND)
#define KS_PACK_TOPO_1 KS_PACK_TOPO_KERNEL
#else
#define KS_PACK_TOPO_0 KS_PACK_TOPO_KERNEL
#define KS_PACK_TOPO_1(NAME, FL, ND)
#endif
#define KS_PACK_TOPO(NAME, FL, ND) KS_PACK_TOPO_##ND(NAME, FL, ND)
KS_CAT(KS_PACK_TOPO_ROWS_, KS_PACK_FLAVOUR)(KS_PACK_TOPO)
#undef KS_PACK_TOPO
#undef KS_PACK_TOPO_0
#undef KS_PACK_TOPO_1
#undef KS_PACK_TOPO_KERNEL
