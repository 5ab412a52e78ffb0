// TEST-ONLY: the wavefront primitives (karpenter_amd/csrc/wave.h), fast_umin_s, the claim orders (pdq_emul.h, run_order.h) and
// shift_right16 alone, one wavefront per launch. ONE source, compiled twice by tests/parity.py build_wave_order():
//   hipcc -x hip --offload-arch=gfx950            -> tests/emu/libwave_order_dev.so     kernels of 64 lanes, one block
//   g++ -DKSOLVE_HOST_EMULATION [-DKS_EMU_REVERSE_LANES] -> libwave_order_host[_reversed].so   the same bodies on the loop-over-lanes Wave
// with the same C entry points (tests/wave_order_cases.py drives both). Every primitive is called the way the engines call it:
// all 64 lanes active, wave-uniform arguments where the signature asks for them. Every entry point checks the indices its kernel
// forms from the caller's tables BEFORE anything is launched, and returns 0, -1 (refused: nothing ran) or a positive runtime error;
// after a runtime error nothing more is launched by this process.
#include <stdint.h>
#include <string.h>
#include <stddef.h>
#include <vector>
#if defined(__HIPCC__) && !defined(KSOLVE_HOST_EMULATION)
#include <hip/hip_runtime.h>
#endif
#include "../../karpenter_amd/csrc/engine.h"        // (fast_engine.h is not self-contained: the order pack_kernels.h includes them in)
#include "../../karpenter_amd/csrc/fast_engine.h"   // fast_umin_s (and wave.h, pdq_emul.h with shift_right16)
#include "../../karpenter_amd/csrc/run_order.h"

typedef ks::Wave W;

// ---------------------------------------------------------------------------------------------------------------------------
// plumbing: a kernel is a function; buffers live on the device or are the caller's own
#if KS_DEVICE
#include <hip/hip_runtime.h>
#define PROBE_KERNEL __global__ void __launch_bounds__(64)
#define PROBE_SHARED(T, name, count) __shared__ __attribute__((aligned(16))) T name[count]
static int g_err = 0;
template <class T> struct Buf {
  T* p = nullptr; T* h; size_t n;
  Buf(const T* host, size_t count) : h((T*)host), n(count) {
    if (g_err) return;
    if (hipMalloc((void**)&p, (n ? n : 1) * sizeof(T)) != hipSuccess) { p = nullptr; g_err = 1; return; }
    if ((h && n ? hipMemcpy(p, h, n * sizeof(T), hipMemcpyHostToDevice) : hipMemset(p, 0, (n ? n : 1) * sizeof(T))) != hipSuccess) g_err = 1;
  }
  void back() { if (!g_err && p && h && n && hipMemcpy(h, p, n * sizeof(T), hipMemcpyDeviceToHost) != hipSuccess) g_err = 1; }
  ~Buf() { if (p) (void)hipFree(p); }
};
template <class... A, class... B> static void launch(void (*k)(A...), B... args) {
  if (g_err) return;
  k<<<dim3(1), dim3(64), 0, 0>>>(args...);
  if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) g_err = 2;
}
#else
#define PROBE_KERNEL static void
#define PROBE_SHARED(T, name, count) alignas(16) static T name[count]
static int g_err = 0;
template <class T> struct Buf {
  T* p; std::vector<T> own;
  Buf(const T* host, size_t count) : p((T*)host) { if (!host) { own.assign(count ? count : 1, T()); p = own.data(); } }
  void back() {}
};
template <class... A, class... B> static void launch(void (*k)(A...), B... args) { k(args...); }
#endif

static KS_DEV int U(int v) { return (int)W::uniform((uint64_t)(uint32_t)v); }   // a value read from a table, as a wave-uniform one

// ---------------------------------------------------------------------------------------------------------------------------
// Part A: wave.h
constexpr int kBallotOut = 7 + 9 * 9;   // ballot, ballot2 (2), ballot4 (4), then per n = 0..8: eight words of ballots8 and the number of g() calls
PROBE_KERNEL k_ballots(const uint32_t* pat, int ncase, unsigned long long* out) {
  for (int c = 0; c < ncase; ++c) {
    const uint32_t* p = pat + (size_t)c * 64;
    unsigned long long* o = out + (size_t)c * kBallotOut;
    W::store(&o[0], W::ballot([&](int l) { return (p[l] & 1u) != 0; }));
    uint64_t a0, a1, b0, b1, b2, b3;
    W::ballot2([&](int l) { return (int)(p[l] & 3u); }, a0, a1);
    W::store(&o[1], a0); W::store(&o[2], a1);
    W::ballot4([&](int l) { return (int)(p[l] & 15u); }, b0, b1, b2, b3);
    W::store(&o[3], b0); W::store(&o[4], b1); W::store(&o[5], b2); W::store(&o[6], b3);
    for (int n = 0; n <= 8; ++n) {
      int calls = 0;
      unsigned long long* on = o + 7 + n * 9;
      W::ballots8(n, [&](int l, int j) { return (p[l] >> j) & 1u; }, [&](int j, uint64_t m) { W::store(&on[j], m); calls++; });
      W::store(&on[8], calls);
    }
  }
  W::sync();
}

// flags[kFindPad + i] is what the predicate reads for position i: true outside [lo, hi) (the padding on both sides included), true at h1 and h2
constexpr int kFindPad = 512, kFindMax = 513 + 1025, kFindFlags = kFindPad + kFindMax + kFindPad;
PROBE_KERNEL k_find(const int* cases, int ncase, uint8_t* flags, int* out) {
  for (int c = 0; c < ncase; ++c) {
    const int fn = U(cases[5 * c]), lo = U(cases[5 * c + 1]), hi = U(cases[5 * c + 2]), h1 = U(cases[5 * c + 3]), h2 = U(cases[5 * c + 4]);
    W::for_n(kFindFlags, [&](int j) { const int i = j - kFindPad; flags[j] = (i < lo || i >= hi || i == h1 || i == h2) ? 1 : 0; });
    auto pred = [&](int i) { return flags[kFindPad + i] != 0; };
    int r;
    if (fn == 0) r = W::find_first(lo, hi, pred); else if (fn == 1) r = W::find_last(lo, hi, pred);
    else if (fn == 2) r = W::find_first8(lo, hi, pred); else r = W::find_last8(lo, hi, pred);
    W::store(&out[c], r);
    W::sync();
  }
}

// fn 0 reduce_min, 1 reduce_max_i64, 2 reduce_or (n values from off); 3 lanes_max_i64, 4 argmin_u32 / min_u32 (64 values from off);
// 5 uniform (one value), 6 fast_umin_s (two values). Three words out per case.
PROBE_KERNEL k_reduce(const int* cases, int ncase, const unsigned long long* v, unsigned long long* out) {
  for (int c = 0; c < ncase; ++c) {
    const int fn = U(cases[3 * c]), off = U(cases[3 * c + 1]), n = U(cases[3 * c + 2]);
    const unsigned long long* x = v + off;
    uint64_t r0 = 0, r1 = 0, r2 = 0;
    if (fn == 0) r0 = W::reduce_min(n, [&](int i) { return (uint64_t)x[i]; });
    else if (fn == 1) r0 = (uint64_t)W::reduce_max_i64(n, [&](int i) { return (int64_t)x[i]; });
    else if (fn == 2) r0 = W::reduce_or(n, [&](int i) { return (uint64_t)x[i]; });
    else if (fn == 3) r0 = (uint64_t)W::lanes_max_i64([&](int l) { return (int64_t)x[l]; });
    else if (fn == 4) {
      int who = -7;
      r0 = W::argmin_u32([&](int l) { return (uint32_t)x[l]; }, &who);
      r1 = (uint64_t)(int64_t)who;
#if KS_DEVICE
      r2 = W::min_u32((uint32_t)x[W::lane()]);   // the DPP reduction alone (the emulation has no form of its own: argmin_u32's value)
#else
      r2 = r0;
#endif
    } else if (fn == 5) r0 = W::uniform((uint64_t)x[0]);
    else r0 = ks::fast_umin_s((uint32_t)W::uniform((uint64_t)x[0]), (uint32_t)W::uniform((uint64_t)x[1]));
    W::store(&out[3 * c], r0); W::store(&out[3 * c + 1], r1); W::store(&out[3 * c + 2], r2);
  }
  W::sync();
}

constexpr int kForNStride = 200 + 64;
PROBE_KERNEL k_for_n(const int* ns, int ncase, uint32_t* cnt) {
  for (int c = 0; c < ncase; ++c) {
    uint32_t* q = cnt + (size_t)c * kForNStride;
    W::for_n(U(ns[c]), [&](int i) {
#if KS_DEVICE
      atomicAdd(&q[i], 1u);   // (two lanes that visited one index would otherwise both write 1)
#else
      q[i] += 1u;
#endif
    });
  }
}

// copy8 on the element types of its call site (fast_engine.h slow_sort: claim ids of 16 bits, into the snapshot in HBM from an order in
// LDS — plan 1 — or in HBM — plan 2)
constexpr int kCopyMax = 1536;
PROBE_KERNEL k_copy8(const uint16_t* src, uint16_t* dst_from_lds, uint16_t* dst_from_hbm, int n) {
  PROBE_SHARED(uint16_t, sh, kCopyMax);
  KS_LDS uint16_t* const s = (KS_LDS uint16_t*)sh;
  W::for_n(kCopyMax, [&](int i) { s[i] = src[i]; });
  W::copy8(dst_from_lds, s, n);
  W::copy8(dst_from_hbm, src, n);
}

PROBE_KERNEL k_store_leader(uint32_t* g, uint32_t* out) {
  PROBE_SHARED(uint32_t, sh, 8);
  KS_LDS uint32_t* const s = (KS_LDS uint32_t*)sh;
  W::for_n(8, [&](int i) { s[i] = 0x11110000u + (uint32_t)i; });
  W::store(&g[1], 0x12345678u);            // a pointer into HBM
  W::store(&s[2], 0x9ABCDEF0ull);          // a pointer into LDS, a wider value (truncated to the pointee)
  W::store((uint16_t*)&g[2], 0x1BEEFu);    // a narrower pointee: the low half only
  if (W::leader()) g[3] = g[3] + 1u;       // once per wavefront
  W::sync();
  W::each([&](int l) { out[l] = g[1]; out[64 + l] = s[2]; out[128 + l] = s[(l & 7)]; });
  W::sync();
}

// 64 v_writelane rounds with run-time lanes: two LaneVar written alternately, a LaneVec64, and an LDS and an HBM access behind each
// (m0 is put back by hand inside the asm)
PROBE_KERNEL k_lane_set(const int* idx, const unsigned long long* val, uint32_t* g, uint32_t* out_a, uint32_t* out_b, unsigned long long* out_v, uint32_t* out_lds) {
  PROBE_SHARED(uint32_t, sh, 64);
  KS_LDS uint32_t* const s = (KS_LDS uint32_t*)sh;
  ks::LaneVar<uint32_t> a, b;
  ks::LaneVec64 vv;
  W::each([&](int l) { a.at(l) = 0xA0000000u | (uint32_t)l; b.at(l) = 0xB0000000u | (uint32_t)l; });
  W::for_n(64, [&](int i) { s[i] = 0; });
  for (int i = 0; i < 64; ++i) {
    const int ln = U(idx[i]) & 63;
    const uint64_t x = W::uniform((uint64_t)val[i]);
    a.set(ln, (uint32_t)x);
    W::store(&s[i], (uint32_t)(x >> 32) + s[(i + 63) & 63]);   // LDS read and write behind the sequence
    W::sync();
    b.set(63 - ln, (uint32_t)(x >> 32) ^ (uint32_t)i);
    vv.set(ln, x);
    W::store(&g[i], (uint32_t)x + g[64 + i]);                  // HBM read and write behind it
    W::sync();
  }
  W::each([&](int l) { out_a[l] = a.at(l); out_b[l] = b.at(l); out_v[l] = vv.get(l); out_lds[l] = s[l]; });
  W::sync();
}

PROBE_KERNEL k_bcast(const unsigned long long* val, uint32_t* o32, unsigned long long* o64) {
  ks::LaneVar<uint32_t> a;
  ks::LaneVar<uint64_t> b;
  W::each([&](int l) { a.at(l) = (uint32_t)(val[l] >> 32) ^ (uint32_t)val[l]; b.at(l) = (uint64_t)val[l]; });
  for (int s = 0; s < 64; ++s) { W::store(&o32[s], a.bcast(s)); W::store(&o64[s], b.bcast(s)); }
  W::sync();
}

PROBE_KERNEL k_shuffle(const int* src, int npat, const unsigned long long* val, uint32_t* o32, unsigned long long* o64) {
  ks::LaneVar<uint32_t> a;
  ks::LaneVar<uint64_t> b;
  W::each([&](int l) { a.at(l) = (uint32_t)(val[l] >> 32) ^ (uint32_t)val[l]; b.at(l) = (uint64_t)val[l]; });
  for (int p = 0; p < npat; ++p)
    W::each([&](int l) { const int from = src[p * 64 + l]; o32[p * 64 + l] = a.shuffle(l, from); o64[p * 64 + l] = b.shuffle(l, from); });
  W::sync();
}

// ---------------------------------------------------------------------------------------------------------------------------
// Part B: the orders. kCap claims at most; the 16-bit arrays are 16-byte aligned and whole 16-byte pieces of them are readable.
constexpr int kCap = 4104;

// one case: off, n, defect, append, mode (0: sort() on "sorted except position defect"; 1: the outermost pdqsort() call on any array)
template <class O, bool POS, class P>
static KS_DEV void sort_cases(P key, P ord, P pos, const uint32_t* kin, const uint32_t* oin, const int* cases, int ncase, uint32_t* kout, uint32_t* oout, uint32_t* pout, unsigned long long* slow) {
  for (int c = 0; c < ncase; ++c) {
    const int off = U(cases[5 * c]), n = U(cases[5 * c + 1]), defect = U(cases[5 * c + 2]), app = U(cases[5 * c + 3]), mode = U(cases[5 * c + 4]);
    W::for_n(n, [&](int i) { key[i] = kin[off + i]; ord[i] = oin[off + i]; if constexpr (POS) pos[oin[off + i]] = (uint32_t)i; });
    O o;
    o.key = key; o.ord = ord; o.pos = pos; o.n = n; o.defect = defect; o.defect_append = app != 0;
    if (mode == 0) o.sort(); else ks::PdqSort<O>::pdqsort(o, 0, n, ks::PdqSort<O>::bits_len((unsigned)n));
    W::sync();
    W::for_n(n, [&](int i) { kout[off + i] = key[i]; oout[off + i] = ord[i]; if constexpr (POS) pout[off + i] = pos[i]; });
    W::store(&slow[c], o.slow_sorts);
  }
  W::sync();
}
typedef ks::ClaimOrder<W, KS_LDS uint16_t*, false, true> Form1;   // cursor plans 0 and 1
typedef ks::ClaimOrder<W, uint16_t*, false, false> Form2;          // cursor plan 2
typedef ks::RegOrder<W> Form3;
typedef ks::ClaimOrder<W, KS_LDS uint32_t*> Form4;                 // the general engine
typedef ks::ClaimOrder<W, uint32_t*, false> Form5;                 // inside RunOrder::sort, topo_engine.h
typedef ks::RunOrder<W> Form6;
struct Form7 : ks::RegOrder<W> { typedef ks::PdqFrameArray FrameStack; };   // RegOrder with pdqsort's waiting calls in scratch, not in a register

#define SORT_ARGS const uint32_t* kin, const uint32_t* oin, const int* cases, int ncase, uint32_t* kout, uint32_t* oout, uint32_t* pout, unsigned long long* slow
PROBE_KERNEL k_sort1(SORT_ARGS) {
  PROBE_SHARED(uint16_t, k, kCap); PROBE_SHARED(uint16_t, o, kCap);
  sort_cases<Form1, false>((KS_LDS uint16_t*)k, (KS_LDS uint16_t*)o, (KS_LDS uint16_t*)nullptr, kin, oin, cases, ncase, kout, oout, pout, slow);
}
PROBE_KERNEL k_sort2(uint16_t* k, uint16_t* o, SORT_ARGS) { sort_cases<Form2, false>(k, o, (uint16_t*)nullptr, kin, oin, cases, ncase, kout, oout, pout, slow); }
PROBE_KERNEL k_sort4(SORT_ARGS) {
  PROBE_SHARED(uint32_t, k, kCap); PROBE_SHARED(uint32_t, o, kCap); PROBE_SHARED(uint32_t, p, kCap);
  sort_cases<Form4, true>((KS_LDS uint32_t*)k, (KS_LDS uint32_t*)o, (KS_LDS uint32_t*)p, kin, oin, cases, ncase, kout, oout, pout, slow);
}
PROBE_KERNEL k_sort5(uint32_t* k, uint32_t* o, SORT_ARGS) { sort_cases<Form5, false>(k, o, (uint32_t*)nullptr, kin, oin, cases, ncase, kout, oout, pout, slow); }
template <class R>
static KS_DEV void sort_cases_reg(SORT_ARGS) {
  for (int c = 0; c < ncase; ++c) {
    const int off = U(cases[5 * c]), n = U(cases[5 * c + 1]), defect = U(cases[5 * c + 2]), app = U(cases[5 * c + 3]), mode = U(cases[5 * c + 4]);
    R r;
    r.load(kin + off, oin + off, n); r.defect = defect; r.defect_append = app != 0;
    if (mode == 0) ks::PdqSort<R>::sort(r); else ks::PdqSort<R>::pdqsort(r, 0, n, ks::PdqSort<R>::bits_len((unsigned)n));
    r.store(kout + off, oout + off);
    W::store(&slow[c], r.slow_sorts);
  }
  (void)pout;
  W::sync();
}
PROBE_KERNEL k_sort3(SORT_ARGS) { sort_cases_reg<Form3>(kin, oin, cases, ncase, kout, oout, pout, slow); }
PROBE_KERNEL k_sort7(SORT_ARGS) { sort_cases_reg<Form7>(kin, oin, cases, ncase, kout, oout, pout, slow); }

// RunOrder's memory, laid out as ksolve_impl.h alloc_run_order lays it out (the loop is restated in run_alloc below)
struct RunMem { uint32_t* ring; uint32_t* cnt; uint32_t* slot; uint32_t* key; uint32_t* ord; uint32_t* tabs; const uint32_t* off; const uint8_t* lg; int kmax; };
static KS_DEV void run_read_back(Form6& ro, const RunMem& m, int n, uint32_t* kout, uint32_t* oout, uint32_t* pout) {
  const uint32_t* cc = m.cnt;
  W::for_n(n, [&](int p) { const uint32_t x = ro.claim_at(p); oout[p] = x; kout[p] = cc[x]; pout[p] = ro.position(p); });   // claim ids are 0 .. n-1
}
// mode 0 only: the rings are built from the sorted array the case had before its claim was touched (rebuild), then the claim is
// touched the way the engine does it (increment / append) and sort() runs
PROBE_KERNEL k_sort6(RunMem m, SORT_ARGS) {
  PROBE_SHARED(ks::RunTables, T, 1);
  for (int c = 0; c < ncase; ++c) {
    const int off = U(cases[5 * c]), n = U(cases[5 * c + 1]), defect = U(cases[5 * c + 2]), app = U(cases[5 * c + 3]);
    Form6 ro;
    ro.init((KS_LDS ks::RunTables*)T, m.ring, m.cnt, m.slot, m.key, m.ord, m.tabs, m.off, m.lg, m.kmax);
    const int nb = app ? n - 1 : n;
    uint32_t* kk = m.key; uint32_t* oo = m.ord;
    W::for_n(nb, [&](int i) { kk[i] = kin[off + i] - ((!app && i == defect) ? 1u : 0u); oo[i] = oin[off + i]; });
    ro.n = nb;
    ro.rebuild();
    W::sync();
    if (app) ro.append((int)W::uniform((uint64_t)oin[off + n - 1])); else ro.increment((int)W::uniform((uint64_t)oin[off + defect]));
    ro.sort();
    W::sync();
    run_read_back(ro, m, n, kout + off, oout + off, pout + off);
    W::store(&slow[c], ro.slow_sorts | (ro.overflow ? 1ull << 63 : 0ull));
  }
  W::sync();
}

// A commit trace: sort() before every op and after the last; op < 0 appends the next claim id, op >= 0 adds a pod to that claim.
// res[0] = claims, res[1] = slow_sorts. An order without `pos` is told the position (the cursor engine knows it; here it is searched for).
template <class O, bool POS, class P>
static KS_DEV void trace_body(P key, P ord, P pos, const int* ops, int nops, uint32_t* kout, uint32_t* oout, uint32_t* pout, unsigned long long* res) {
  O o;
  o.key = key; o.ord = ord; o.pos = pos;
  int claims = 0;
  for (int i = 0; i < nops; ++i) {
    o.sort();
    const int op = U(ops[i]);
    if (op < 0) o.append(claims++);
    else if constexpr (POS) o.increment(op);
    else {
      const int p = W::find_first(0, o.n, [&](int x) { return (uint32_t)ord[x] == (uint32_t)op; });
      W::store(&key[p], (uint32_t)key[p] + 1u);
      W::sync();
      o.defect = p; o.defect_append = false;
    }
  }
  o.sort();
  W::sync();
  W::for_n(o.n, [&](int i) { kout[i] = key[i]; oout[i] = ord[i]; if constexpr (POS) pout[i] = pos[i]; });
  W::store(&res[0], o.n); W::store(&res[1], o.slow_sorts);
  W::sync();
}
#define TRACE_ARGS const int* ops, int nops, uint32_t* kout, uint32_t* oout, uint32_t* pout, unsigned long long* res
PROBE_KERNEL k_trace1(TRACE_ARGS) {
  PROBE_SHARED(uint16_t, k, kCap); PROBE_SHARED(uint16_t, o, kCap);
  trace_body<Form1, false>((KS_LDS uint16_t*)k, (KS_LDS uint16_t*)o, (KS_LDS uint16_t*)nullptr, ops, nops, kout, oout, pout, res);
}
PROBE_KERNEL k_trace2(uint16_t* k, uint16_t* o, TRACE_ARGS) { trace_body<Form2, false>(k, o, (uint16_t*)nullptr, ops, nops, kout, oout, pout, res); }
PROBE_KERNEL k_trace4(TRACE_ARGS) {
  PROBE_SHARED(uint32_t, k, kCap); PROBE_SHARED(uint32_t, o, kCap); PROBE_SHARED(uint32_t, p, kCap);
  trace_body<Form4, true>((KS_LDS uint32_t*)k, (KS_LDS uint32_t*)o, (KS_LDS uint32_t*)p, ops, nops, kout, oout, pout, res);
}
PROBE_KERNEL k_trace5(uint32_t* k, uint32_t* o, TRACE_ARGS) { trace_body<Form5, false>(k, o, (uint32_t*)nullptr, ops, nops, kout, oout, pout, res); }
// RegOrder: load / sort / store around every op, the arrays in HBM between (fast_engine.h slow_sort with n <= 64)
PROBE_KERNEL k_trace3(TRACE_ARGS) {
  int n = 0, defect = -1, claims = 0;
  bool app = false;
  uint64_t slow = 0;
  auto sort = [&]() {
    Form3 r;
    r.load(kout, oout, n); r.defect = defect; r.defect_append = app;
    r.sort();
    slow += r.slow_sorts;
    r.store(kout, oout);
    defect = -1;
  };
  for (int i = 0; i < nops; ++i) {
    sort();
    const int op = U(ops[i]);
    if (op < 0) { W::store(&kout[n], 1u); W::store(&oout[n], (uint32_t)claims++); defect = n; app = true; n++; }
    else {
      const int p = W::find_first(0, n, [&](int x) { return oout[x] == (uint32_t)op; });
      W::store(&kout[p], kout[p] + 1u);
      defect = p; app = false;
    }
    W::sync();
  }
  sort();
  (void)pout;
  W::store(&res[0], n); W::store(&res[1], slow);
  W::sync();
}
// RunOrder; res[2] / res[3] = how often the head of one of the rings 1 .. 8 stepped up / down across the ring's end
PROBE_KERNEL k_trace6(RunMem m, TRACE_ARGS) {
  PROBE_SHARED(ks::RunTables, T, 1);
  Form6 ro;
  ro.init((KS_LDS ks::RunTables*)T, m.ring, m.cnt, m.slot, m.key, m.ord, m.tabs, m.off, m.lg, m.kmax);
  int claims = 0;
  unsigned long long up = 0, down = 0;
  auto sort = [&]() {
    uint32_t h[8];
    for (int k = 1; k <= 8; ++k) h[k - 1] = k <= ro.max_cnt ? ro.head_(k) : 0u;   // (a run that does not exist yet starts with its head at 0: grow_to)
    ro.sort();
    W::sync();
    for (int k = 1; k <= 8 && k <= ro.max_cnt; ++k) {
      const uint32_t now = ro.head_(k), msk = ro.mask_of(k);
      if (now == ((h[k - 1] + 1u) & msk) && now < h[k - 1]) up++;
      if (now == ((h[k - 1] - 1u) & msk) && now > h[k - 1]) down++;
    }
  };
  for (int i = 0; i < nops; ++i) {
    sort();
    const int op = U(ops[i]);
    if (op < 0) ro.append(claims++); else ro.increment(op);
  }
  sort();
  run_read_back(ro, m, ro.n, kout, oout, pout);
  W::store(&res[0], ro.n); W::store(&res[1], ro.slow_sorts | (ro.overflow ? 1ull << 63 : 0ull)); W::store(&res[2], up); W::store(&res[3], down);
  W::sync();
}

// The five scans over 16-bit keys: out[2c] = form 1 (LDS, 512 positions per step), out[2c + 1] = form 2 (HBM, one position per lane).
// op 0 first_ge, 1 first_gt, 2 last_le, 3 last_lt (against v), 4 first_descent
constexpr int kScanMax = 1616;
template <class O>
static KS_DEV int scan_one(const O& o, int op, int lo, int hi, uint32_t v) {
  switch (op) {
    case 0: return o.first_ge(lo, hi, v);
    case 1: return o.first_gt(lo, hi, v);
    case 2: return o.last_le(lo, hi, v);
    case 3: return o.last_lt(lo, hi, v);
    default: return o.first_descent(lo, hi);
  }
}
PROBE_KERNEL k_scans(uint16_t* keys, int n, const int* cases, int ncase, int* out) {
  PROBE_SHARED(uint16_t, k, kScanMax);
  KS_LDS uint16_t* const kl = (KS_LDS uint16_t*)k;
  W::for_n(kScanMax, [&](int i) { kl[i] = keys[i]; });
  Form1 w; Form2 s;
  w.key = kl; w.n = n; s.key = keys; s.n = n;
  for (int c = 0; c < ncase; ++c) {
    const int op = U(cases[4 * c]), lo = U(cases[4 * c + 1]), hi = U(cases[4 * c + 2]);
    const uint32_t v = (uint32_t)U(cases[4 * c + 3]);
    W::store(&out[2 * c], scan_one(w, op, lo, hi, v));
    W::store(&out[2 * c + 1], scan_one(s, op, lo, hi, v));
  }
  W::sync();
}

// shift_right16: every case on a fresh copy of arr[kShiftLen]; the whole array comes back
constexpr int kShiftLen = 1536;
PROBE_KERNEL k_shift(const uint16_t* arr, const int* cases, int ncase, uint16_t* out) {
  PROBE_SHARED(uint16_t, sh, kShiftLen);
  KS_LDS uint16_t* const s = (KS_LDS uint16_t*)sh;
  for (int c = 0; c < ncase; ++c) {
    const int b = U(cases[2 * c]), a = U(cases[2 * c + 1]);
    W::for_n(kShiftLen, [&](int i) { s[i] = arr[i]; });
    ks::shift_right16<W>(s, b, a);
    W::sync();
    uint16_t* o = out + (size_t)c * kShiftLen;
    W::for_n(kShiftLen, [&](int i) { o[i] = s[i]; });
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// entry points
static int done() { return g_err; }
static bool sort_cases_ok(int form, const uint32_t* oin, int total, const int* cases, int ncase) {
  if (total < 0 || ncase < 0) return false;
  for (int c = 0; c < ncase; ++c) {
    const int off = cases[5 * c], n = cases[5 * c + 1], defect = cases[5 * c + 2], app = cases[5 * c + 3], mode = cases[5 * c + 4];
    if (off < 0 || n < 1 || n > kCap || off > total - n || defect < -1 || defect >= n || (mode != 0 && mode != 1)) return false;
    if ((form == 3 || form == 7) && n > 64) return false;
    if (app && defect != n - 1) return false;
    if (form == 6 && (mode != 0 || defect < 0 || n < 2)) return false;
    for (int i = 0; i < n; ++i) if (oin[off + i] >= (uint32_t)n) return false;   // claim ids index pos / cnt / slot
  }
  return true;
}
// ksolve_impl.h alloc_run_order, restated: ring k holds min(max_claims, n_pods / k + 2) + 2 claims, rounded up to a power of two
struct RunAlloc {
  std::vector<uint32_t> off; std::vector<uint8_t> lg; uint64_t total = 0; size_t kmax;
  RunAlloc(int n_pods, int max_claims) : kmax((size_t)n_pods + 2) {
    off.assign(kmax, 0); lg.assign(kmax, 0);
    for (size_t k = 1; k < kmax; ++k) {
      uint64_t need = (uint64_t)max_claims < (uint64_t)n_pods / k + 2 ? (uint64_t)max_claims : (uint64_t)n_pods / k + 2;
      need += 2;
      int l2 = 1;
      while ((1ull << l2) < need) ++l2;
      off[k] = (uint32_t)total; lg[k] = (uint8_t)l2;
      total += 1ull << l2;
    }
  }
};
struct RunBufs {
  RunAlloc a; Buf<uint32_t> ring, cnt, slot, key, ord, tabs, off; Buf<uint8_t> lg;
  RunBufs(int n_pods, int max_claims) : a(n_pods, max_claims), ring(nullptr, a.total), cnt(nullptr, max_claims), slot(nullptr, max_claims), key(nullptr, max_claims), ord(nullptr, max_claims),
    tabs(nullptr, 3 * a.kmax), off(a.off.data(), a.off.size()), lg(a.lg.data(), a.lg.size()) {}
  RunMem mem() { return RunMem{ring.p, cnt.p, slot.p, key.p, ord.p, tabs.p, off.p, lg.p, (int)a.kmax}; }
};

extern "C" {
int probe_is_device() { return KS_DEVICE; }
int probe_ballot_out_words() { return kBallotOut; }
int probe_ballots(const uint32_t* pat, int ncase, unsigned long long* out) {
  if (ncase < 0) return -1;
  Buf<uint32_t> p(pat, (size_t)ncase * 64); Buf<unsigned long long> o(out, (size_t)ncase * kBallotOut);
  launch(k_ballots, p.p, ncase, o.p);
  o.back();
  return done();
}
int probe_find(const int* cases, int ncase, int* out) {
  for (int c = 0; c < ncase; ++c) {
    const int fn = cases[5 * c], lo = cases[5 * c + 1], hi = cases[5 * c + 2];
    if (fn < 0 || fn > 3 || lo < 0 || hi < lo || hi > kFindMax) return -1;
  }
  Buf<int> cs(cases, (size_t)ncase * 5); Buf<uint8_t> fl(nullptr, kFindFlags); Buf<int> o(out, ncase);
  launch(k_find, cs.p, ncase, fl.p, o.p);
  o.back();
  return done();
}
int probe_reduce(const int* cases, int ncase, const unsigned long long* v, int nv, unsigned long long* out) {
  for (int c = 0; c < ncase; ++c) {
    const int fn = cases[3 * c], off = cases[3 * c + 1], n = cases[3 * c + 2];
    const int reads = fn <= 2 ? n : fn <= 4 ? 64 : fn == 5 ? 1 : 2;
    if (fn < 0 || fn > 6 || off < 0 || n < 0 || off > nv - reads) return -1;
  }
  Buf<int> cs(cases, (size_t)ncase * 3); Buf<unsigned long long> vv(v, nv); Buf<unsigned long long> o(out, (size_t)ncase * 3);
  launch(k_reduce, cs.p, ncase, vv.p, o.p);
  o.back();
  return done();
}
int probe_for_n_stride() { return kForNStride; }
int probe_for_n(const int* ns, int ncase, uint32_t* cnt) {
  for (int c = 0; c < ncase; ++c) if (ns[c] < 0 || ns[c] > kForNStride - 64) return -1;
  Buf<int> n(ns, ncase); Buf<uint32_t> o(cnt, (size_t)ncase * kForNStride);
  launch(k_for_n, n.p, ncase, o.p);
  o.back();
  return done();
}
int probe_copy8(const uint16_t* src, uint16_t* dst_from_lds, uint16_t* dst_from_hbm, int n) {   // all three [1536]
  if (n < 0 || n > kCopyMax) return -1;
  Buf<uint16_t> s(src, kCopyMax), a(dst_from_lds, kCopyMax), b(dst_from_hbm, kCopyMax);
  launch(k_copy8, s.p, a.p, b.p, n);
  a.back(); b.back();
  return done();
}
int probe_store_leader(uint32_t* g /*[4]*/, uint32_t* out /*[192]*/) {
  Buf<uint32_t> gg(g, 4), o(out, 192);
  launch(k_store_leader, gg.p, o.p);
  gg.back(); o.back();
  return done();
}
int probe_lane_set(const int* idx, const unsigned long long* val, uint32_t* g /*[128]*/, uint32_t* out_a, uint32_t* out_b, unsigned long long* out_v, uint32_t* out_lds) {
  Buf<int> i(idx, 64); Buf<unsigned long long> v(val, 64), ov(out_v, 64); Buf<uint32_t> gg(g, 128), oa(out_a, 64), ob(out_b, 64), ol(out_lds, 64);
  launch(k_lane_set, i.p, v.p, gg.p, oa.p, ob.p, ov.p, ol.p);
  gg.back(); oa.back(); ob.back(); ov.back(); ol.back();
  return done();
}
int probe_bcast(const unsigned long long* val, uint32_t* o32, unsigned long long* o64) {
  Buf<unsigned long long> v(val, 64), b(o64, 64); Buf<uint32_t> a(o32, 64);
  launch(k_bcast, v.p, a.p, b.p);
  a.back(); b.back();
  return done();
}
int probe_shuffle(const int* src, int npat, const unsigned long long* val, uint32_t* o32, unsigned long long* o64) {
  if (npat < 0) return -1;
  for (int i = 0; i < npat * 64; ++i) if (src[i] < 0 || src[i] > 63) return -1;   // the engines' sources are lanes
  Buf<int> s(src, (size_t)npat * 64); Buf<unsigned long long> v(val, 64), b(o64, (size_t)npat * 64); Buf<uint32_t> a(o32, (size_t)npat * 64);
  launch(k_shuffle, s.p, npat, v.p, a.p, b.p);
  a.back(); b.back();
  return done();
}

// forms 1 .. 7 (see the typedefs); n_pods / max_claims: form 6's ring layout (sum of the keys of a case <= n_pods, n <= max_claims)
int probe_sort(int form, const uint32_t* key, const uint32_t* ord, int total, const int* cases, int ncase, uint32_t* kout, uint32_t* oout, uint32_t* pout, unsigned long long* slow, int n_pods, int max_claims) {
  if (form < 1 || form > 7 || !sort_cases_ok(form, ord, total, cases, ncase)) return -1;
  if (form == 1 || form == 2) for (int i = 0; i < total; ++i) if (key[i] > 0xFFFFu) return -1;
  if (form == 6) {
    if (n_pods < 1 || n_pods > 1000000 || max_claims < 1 || max_claims > kCap) return -1;
    for (int c = 0; c < ncase; ++c) {
      unsigned long long sum = 0;
      const int off = cases[5 * c], n = cases[5 * c + 1];
      for (int i = 0; i < n; ++i) { sum += key[off + i]; if (key[off + i] < 1 || key[off + i] + 3 >= (uint32_t)n_pods) return -1; }
      if (sum > (unsigned long long)n_pods || n > max_claims) return -1;
    }
  }
  Buf<uint32_t> k(key, total), o(ord, total), ko(kout, total), oo(oout, total), po(pout, total);
  Buf<int> cs(cases, (size_t)ncase * 5); Buf<unsigned long long> sl(slow, ncase);
  if (form == 1) launch(k_sort1, k.p, o.p, cs.p, ncase, ko.p, oo.p, po.p, sl.p);
  else if (form == 2) { Buf<uint16_t> wk(nullptr, kCap), wo(nullptr, kCap); launch(k_sort2, wk.p, wo.p, k.p, o.p, cs.p, ncase, ko.p, oo.p, po.p, sl.p); }
  else if (form == 3) launch(k_sort3, k.p, o.p, cs.p, ncase, ko.p, oo.p, po.p, sl.p);
  else if (form == 4) launch(k_sort4, k.p, o.p, cs.p, ncase, ko.p, oo.p, po.p, sl.p);
  else if (form == 5) { Buf<uint32_t> wk(nullptr, kCap), wo(nullptr, kCap); launch(k_sort5, wk.p, wo.p, k.p, o.p, cs.p, ncase, ko.p, oo.p, po.p, sl.p); }
  else if (form == 6) { RunBufs rb(n_pods, max_claims); launch(k_sort6, rb.mem(), k.p, o.p, cs.p, ncase, ko.p, oo.p, po.p, sl.p); }
  else launch(k_sort7, k.p, o.p, cs.p, ncase, ko.p, oo.p, po.p, sl.p);
  ko.back(); oo.back(); po.back(); sl.back();
  return done();
}
// kout / oout / pout [kCap], res [4]
int probe_trace(int form, const int* ops, int nops, uint32_t* kout, uint32_t* oout, uint32_t* pout, unsigned long long* res, int n_pods, int max_claims) {
  if (form < 1 || form > 6 || nops < 0) return -1;
  int claims = 0, pods = 0;
  for (int i = 0; i < nops; ++i) {
    if (ops[i] < 0) claims++; else if (ops[i] >= claims) return -1;
    pods++;
  }
  if (claims > kCap - 8 || (form == 3 && claims > 64) || ((form == 1 || form == 2) && pods > 0xFFFF)) return -1;
  if (form == 6 && (n_pods < pods + 4 || n_pods > 1000000 || max_claims < claims || max_claims > kCap)) return -1;
  Buf<int> op(ops, nops); Buf<uint32_t> ko(kout, kCap), oo(oout, kCap), po(pout, kCap); Buf<unsigned long long> r(res, 4);
  if (form == 1) launch(k_trace1, op.p, nops, ko.p, oo.p, po.p, r.p);
  else if (form == 2) { Buf<uint16_t> wk(nullptr, kCap), wo(nullptr, kCap); launch(k_trace2, wk.p, wo.p, op.p, nops, ko.p, oo.p, po.p, r.p); }
  else if (form == 3) launch(k_trace3, op.p, nops, ko.p, oo.p, po.p, r.p);
  else if (form == 4) launch(k_trace4, op.p, nops, ko.p, oo.p, po.p, r.p);
  else if (form == 5) { Buf<uint32_t> wk(nullptr, kCap), wo(nullptr, kCap); launch(k_trace5, wk.p, wo.p, op.p, nops, ko.p, oo.p, po.p, r.p); }
  else { RunBufs rb(n_pods, max_claims); launch(k_trace6, rb.mem(), op.p, nops, ko.p, oo.p, po.p, r.p); }
  ko.back(); oo.back(); po.back(); r.back();
  return done();
}
int probe_scan_len() { return kScanMax; }
int probe_scans(const uint16_t* keys /*[kScanMax]*/, int n, const int* cases, int ncase, int* out) {
  if (n < 0 || n > kScanMax - 512) return -1;
  for (int c = 0; c < ncase; ++c) {
    const int op = cases[4 * c], lo = cases[4 * c + 1], hi = cases[4 * c + 2];
    if (op < 0 || op > 4 || lo < (op == 4 ? 1 : 0) || hi < lo || hi > n) return -1;
  }
  Buf<uint16_t> k(keys, kScanMax); Buf<int> cs(cases, (size_t)ncase * 4), o(out, (size_t)ncase * 2);
  launch(k_scans, k.p, n, cs.p, ncase, o.p);
  o.back();
  return done();
}
int probe_shift_len() { return kShiftLen; }
int probe_shift(const uint16_t* arr /*[kShiftLen]*/, const int* cases, int ncase, uint16_t* out /*[ncase][kShiftLen]*/) {
  for (int c = 0; c < ncase; ++c) if (cases[2 * c] < 0 || cases[2 * c] > cases[2 * c + 1] || cases[2 * c + 1] + 8 > kShiftLen) return -1;
  Buf<uint16_t> a(arr, kShiftLen), o(out, (size_t)ncase * kShiftLen); Buf<int> cs(cases, (size_t)ncase * 2);
  launch(k_shift, a.p, cs.p, ncase, o.p);
  o.back();
  return done();
}

#if !KS_DEVICE
// Which paths of pdqsort a case takes, from the calls the algorithm makes on its accessor (form 5), host twin only:
//   [0] slow_sorts  [1] heap_sort: the only caller of less(i, i + 1)   [2] partition_equal: the only caller of first_gt
//   [3] partition: the only caller of last_lt   [4] partialInsertionSort below the outermost call: the only caller of first_descent
//   [5] reverse_range: four swaps in a row, each nested inside the one before, nothing asked in between
//   [6] break_patterns: three swaps in a row whose first index steps up by one, not nested   [7] rotate_right  [8] rotate_left
//   [9] rotate_left with same_keys  [10] the binary searches over a sorted range
struct Counted : Form5 {
  unsigned long long c[11] = {};
  int run = 0, inc = 0, li = -9, lj = -9;
  void asked() { run = 0; inc = 0; }
  bool less(int i, int j) { asked(); if (j == i + 1) c[1]++; return Form5::less(i, j); }
  uint32_t key_at(int i) { asked(); return Form5::key_at(i); }
  void swap(int i, int j) {
    const bool nested = run > 0 && i == li + 1 && j == lj - 1;
    run = nested ? run + 1 : 1;
    inc = (inc > 0 && i == li + 1 && !nested) ? inc + 1 : 1;
    li = i; lj = j;
    if (run == 4) c[5]++;
    if (inc == 3) c[6]++;
    Form5::swap(i, j);
  }
  int first_ge(int lo, int hi, uint32_t v) { asked(); return Form5::first_ge(lo, hi, v); }
  int first_gt(int lo, int hi, uint32_t v) { asked(); c[2]++; return Form5::first_gt(lo, hi, v); }
  int last_le(int lo, int hi, uint32_t v) { asked(); return Form5::last_le(lo, hi, v); }
  int last_lt(int lo, int hi, uint32_t v) { asked(); c[3]++; return Form5::last_lt(lo, hi, v); }
  int first_descent(int lo, int hi) { asked(); c[4]++; return Form5::first_descent(lo, hi); }
  int first_ge_sorted(int lo, int hi, uint32_t v) { asked(); c[10]++; return Form5::first_ge_sorted(lo, hi, v); }
  int last_le_sorted(int lo, int hi, uint32_t v) { asked(); c[10]++; return Form5::last_le_sorted(lo, hi, v); }
  void rotate_right(int to, int from) { asked(); if (to < from) c[7]++; Form5::rotate_right(to, from); }
  void rotate_left(int from, int to, bool same = false) { asked(); if (to > from) { c[8]++; if (same) c[9]++; } Form5::rotate_left(from, to, same); }
};
int probe_sort_paths(uint32_t* key, uint32_t* ord, int n, int defect, int append, int mode, unsigned long long* counters /*[11]*/) {
  Counted o;
  o.key = key; o.ord = ord; o.pos = nullptr; o.n = n; o.defect = defect; o.defect_append = append != 0;
  if (mode == 0) ks::PdqSort<Counted>::sort(o); else ks::PdqSort<Counted>::pdqsort(o, 0, n, ks::PdqSort<Counted>::bits_len((unsigned)n));
  o.c[0] = o.slow_sorts;
  memcpy(counters, o.c, sizeof(o.c));
  return 0;
}
#endif
}
