// TEST-ONLY host build of the claim-order sort (karpenter_amd/csrc/pdq_emul.h) for tests/test_small_order_sort.py: the same
// array sorted by ClaimOrder (arrays in memory) and by RegOrder (one claim per lane), and the wide searches against the
// scalar ones. Built by the test with g++, with and without -DKS_EMU_REVERSE_LANES.
#define KSOLVE_HOST_EMULATION 1
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../karpenter_amd/csrc/pdq_emul.h"

extern "C" {
// mode 0: sort() on "sorted except position `defect`" (append != 0: the defect is a claim appended with one pod);
// mode 1: pdqsort() on any array (the outermost call, as sort() makes it for 12 < n).
// key / ord [n] in; key_mem / ord_mem and key_reg / ord_reg [n] out; slow[2] = slow_sorts of the two.
void small_order_sort(const uint32_t* key, const uint32_t* ord, int n, int defect, int append, int mode,
                      uint32_t* key_mem, uint32_t* ord_mem, uint32_t* key_reg, uint32_t* ord_reg, unsigned long long* slow) {
  typedef ks::ClaimOrder<ks::Wave, uint32_t*, false> Mem;
  typedef ks::RegOrder<ks::Wave> Reg;
  memcpy(key_mem, key, sizeof(uint32_t) * n); memcpy(ord_mem, ord, sizeof(uint32_t) * n);
  Mem m;
  m.key = key_mem; m.ord = ord_mem; m.pos = nullptr; m.n = n; m.defect = defect; m.defect_append = append != 0;
  if (mode == 0) m.sort(); else ks::PdqSort<Mem>::pdqsort(m, 0, n, ks::PdqSort<Mem>::bits_len((unsigned)n));
  memcpy(key_reg, key, sizeof(uint32_t) * n); memcpy(ord_reg, ord, sizeof(uint32_t) * n);
  Reg r;
  r.load(key_reg, ord_reg, n); r.defect = defect; r.defect_append = append != 0;
  memset(key_reg, 0xEE, sizeof(uint32_t) * n); memset(ord_reg, 0xEE, sizeof(uint32_t) * n);   // only store() brings them back
  if (mode == 0) r.sort(); else ks::PdqSort<Reg>::pdqsort(r, 0, n, ks::PdqSort<Reg>::bits_len((unsigned)n));
  r.store(key_reg, ord_reg);
  slow[0] = m.slow_sorts; slow[1] = r.slow_sorts;
}
// The five scans of pdqsort over keys[0, n) (16-bit, 16-byte aligned, readable up to the next multiple of eight): op 0 first_ge, 1 first_gt,
// 2 last_le, 3 last_lt (against v), 4 first_descent. out[0] = the wide form, out[1] = the one-position-per-lane form.
void small_order_scan(const uint16_t* keys, int n, int op, int lo, int hi, uint32_t v, int* out) {
  ks::ClaimOrder<ks::Wave, uint16_t*, false, true> w;
  ks::ClaimOrder<ks::Wave, uint16_t*, false, false> s;
  w.key = (uint16_t*)keys; s.key = (uint16_t*)keys; w.n = s.n = n;
  switch (op) {
    case 0: out[0] = w.first_ge(lo, hi, v); out[1] = s.first_ge(lo, hi, v); break;
    case 1: out[0] = w.first_gt(lo, hi, v); out[1] = s.first_gt(lo, hi, v); break;
    case 2: out[0] = w.last_le(lo, hi, v); out[1] = s.last_le(lo, hi, v); break;
    case 3: out[0] = w.last_lt(lo, hi, v); out[1] = s.last_lt(lo, hi, v); break;
    default: out[0] = w.first_descent(lo, hi); out[1] = s.first_descent(lo, hi); break;
  }
}
}
