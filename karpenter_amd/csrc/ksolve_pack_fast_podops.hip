// ksolve_pack_fast_podops.hip — the cursor engine (fast_engine.h) that takes pod classes with NotIn, Exists and DoesNotExist
// requirements (engines 26 / 27, FastWork::podops; "The cursor engine's pod operators" in fast_engine.h): the same engine per memory
// plan and per number of class-slot rows as ksolve_pack_fast_unsched.hip — the set-aside list compiled in (FastEngine's US) — with the
// classes' packed form, the static verdicts and the instance-type filter of such classes (FastEngine's PO). A unit of its own, so that
// the kernels every other setting runs are compiled without that code and keep their object.
#include "pack_kernels.h"

#define KS_PACK_FAST_P(NAME, GS, R)                                                       \
  __global__ void __launch_bounds__(64) NAME(const ks::FastArgs* a) {                     \
    extern __shared__ __attribute__((aligned(16))) char lds[];                            \
    ks::FastEngine<ks::Wave, GS, R, false, true, true> eng(&a->pv, &a->ws, &a->fw, lds);  \
    eng.solve();                                                                          \
  }
KS_PACK_FAST_P(ksolve_pack_fast_p_g0r1, 0, 1)
KS_PACK_FAST_P(ksolve_pack_fast_p_g1r1, 1, 1)
KS_PACK_FAST_P(ksolve_pack_fast_p_g2r1, 2, 1)
KS_PACK_FAST_P(ksolve_pack_fast_p_g0r4, 0, ks::kFastRows)
KS_PACK_FAST_P(ksolve_pack_fast_p_g1r4, 1, ks::kFastRows)
KS_PACK_FAST_P(ksolve_pack_fast_p_g2r4, 2, ks::kFastRows)
#undef KS_PACK_FAST_P
