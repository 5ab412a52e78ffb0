// ksolve_pack_topo_many.hip — the spread engine (topo_engine.h), many problems per launch (topo_many.h), compiled once per flavour
// (pack_flavours.h) with -DKS_PACK_FLAVOUR=<n>: every build defines the rows of its flavour in KS_PACK_TOPO_MANY_ROWS, in list order —
// the many-problem forms of that flavour's ksolve_pack_topo* and ksolve_pack_topo_nodes*. Units of their own, so that the
// single-problem kernels keep their objects.
#include "pack_kernels.h"

#include "topo_engine.h"
#include "topo_many.h"

#ifndef KS_PACK_FLAVOUR
#error "ksolve_pack_topo_many.hip is compiled per flavour: -DKS_PACK_FLAVOUR=<TopoFlavour>"
#endif
#define KS_PACK_TOPO_MANY(NAME, FL, ND)                                                                                         \
  __global__ void __launch_bounds__(64) NAME(const ks::TopoArgs* const* items, const uint32_t* order, uint32_t* next, int n) {  \
    extern __shared__ __attribute__((aligned(16))) char lds[];                                                                  \
    const ks::TopoArgs* a = ks::topo_many_take(items, order, next, n);                                                          \
    if (!a) return;                                                                                                             \
    ks::TopoEngine<ks::Wave, ND != 0, ks::flavour_us(ks::TopoFlavour::FL), ks::flavour_fs(ks::TopoFlavour::FL), ks::flavour_po(ks::TopoFlavour::FL)> \
        eng(&a->pv, &a->ws, &a->fw, &a->tw, lds);                                                                               \
    eng.solve();                                                                                                                \
  }
KS_CAT(KS_PACK_TOPO_MANY_ROWS_, KS_PACK_FLAVOUR)(KS_PACK_TOPO_MANY)
#undef KS_PACK_TOPO_MANY
