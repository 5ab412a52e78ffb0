// ksolve_test_fast_cold.hip — TEST BUILDS ONLY (-DKSOLVE_TEST_HOOKS; build_ksolve leaves this unit out of the product library, and
// without the define it is empty): the one-wavefront kernels of ksolve_test_fast_cold (fast_cold_probe.h), the rows of
// KS_FAST_COLD_ROWS (pack_flavours.h) — one per instantiation of FastCold the product's kernels use: every flavour with one row and
// four rows of class slots on the LDS plan; plan 1 with one row; plan 2 with four.
#ifdef KSOLVE_TEST_HOOKS
#include "pack_kernels.h"
#include "fast_cold_probe.h"

#define KS_FAST_COLD(NAME, FL, GS, R)                                                                                            \
  __global__ void __launch_bounds__(64) NAME(const ks::FastColdArgs* a) {                                                        \
    extern __shared__ __attribute__((aligned(16))) char lds[];                                                                   \
    ks::fast_cold_probe_body<ks::Wave, GS, R, ks::flavour_us(ks::FastFlavour::FL), ks::flavour_po(ks::FastFlavour::FL)>(a, lds); \
  }
KS_FAST_COLD_ROWS(KS_FAST_COLD)
#undef KS_FAST_COLD
#endif
