// ksolve_pack_fast_unsched.hip — the cursor engine (fast_engine.h) that KEEPS unschedulable pods (engines 20 / 21, FastWork::unsched;
// "Unschedulable pods" in fast_engine.h): the same engine per memory plan and per number of class-slot rows as ksolve_pack_fast.hip,
// compiled with the set-aside list, the error computation and the retry pass (FastEngine's US). A unit of its own, so that the
// kernels every other setting runs are compiled without that code and keep their object.
#include "pack_kernels.h"

#define KS_PACK_FAST_U(NAME, GS, R)                                                 \
  __global__ void __launch_bounds__(64) NAME(const ks::FastArgs* a) {               \
    extern __shared__ __attribute__((aligned(16))) char lds[];                      \
    ks::FastEngine<ks::Wave, GS, R, false, true> eng(&a->pv, &a->ws, &a->fw, lds);  \
    eng.solve();                                                                    \
  }
KS_PACK_FAST_U(ksolve_pack_fast_u_g0r1, 0, 1)
KS_PACK_FAST_U(ksolve_pack_fast_u_g1r1, 1, 1)
KS_PACK_FAST_U(ksolve_pack_fast_u_g2r1, 2, 1)
KS_PACK_FAST_U(ksolve_pack_fast_u_g0r4, 0, ks::kFastRows)
KS_PACK_FAST_U(ksolve_pack_fast_u_g1r4, 1, ks::kFastRows)
KS_PACK_FAST_U(ksolve_pack_fast_u_g2r4, 2, ks::kFastRows)
#undef KS_PACK_FAST_U
