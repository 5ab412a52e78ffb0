// ksolve_test_fast_cold.hip — TEST BUILDS ONLY (-DKSOLVE_TEST_HOOKS; build_ksolve leaves this unit out of the product library, and
// without the define it is empty): the one-wavefront kernels of ksolve_test_fast_cold (fast_cold_probe.h), one per instantiation of
// FastCold the product's kernels use — the engine without the set-aside list, with it (ksolve_pack_fast_u_*) and with the pod
// operators as well (ksolve_pack_fast_p_*), one row and four rows of class slots on the LDS plan; plan 1 with one row; plan 2 with four.
#ifdef KSOLVE_TEST_HOOKS
#include "pack_kernels.h"
#include "fast_cold_probe.h"

#define KS_FAST_COLD(NAME, GS, R, US, PO)                                             \
  __global__ void __launch_bounds__(64) NAME(const ks::FastColdArgs* a) {             \
    extern __shared__ __attribute__((aligned(16))) char lds[];                        \
    ks::fast_cold_probe_body<ks::Wave, GS, R, US, PO>(a, lds);                        \
  }
KS_FAST_COLD(ksolve_test_fast_cold_g0r1, 0, 1, false, false)
KS_FAST_COLD(ksolve_test_fast_cold_g0r4, 0, ks::kFastRows, false, false)
KS_FAST_COLD(ksolve_test_fast_cold_u_g0r1, 0, 1, true, false)
KS_FAST_COLD(ksolve_test_fast_cold_u_g0r4, 0, ks::kFastRows, true, false)
KS_FAST_COLD(ksolve_test_fast_cold_p_g0r1, 0, 1, true, true)
KS_FAST_COLD(ksolve_test_fast_cold_p_g0r4, 0, ks::kFastRows, true, true)
KS_FAST_COLD(ksolve_test_fast_cold_g1r1, 1, 1, false, false)
KS_FAST_COLD(ksolve_test_fast_cold_u_g2r4, 2, ks::kFastRows, true, false)
#undef KS_FAST_COLD
#endif
