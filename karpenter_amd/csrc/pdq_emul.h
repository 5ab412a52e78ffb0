// pdq_emul.h — bit-exact emulation of the claim ordering the reference maintains with
//     sort.Slice(s.newNodeClaims, func(a, b int) bool { return len(a.Pods) < len(b.Pods) })     scheduler.go:598
// which runs before every in-flight scan and is Go's UNSTABLE pattern-defeating quicksort (go1.26 sort/zsortfunc.go:
// insertion sort <= 12, ninther pivot, partialInsertionSort, partitionEqual, breakPatterns xorshift, heapsort
// fallback). Which of two equally-full claims a pod lands in depends on the permutation that algorithm leaves, so
// the device keeps the claims in exactly that permutation.
//
// The array is always "sorted except for the one claim the previous step touched" (its count went up by one, or it
// was appended with count 1). For that input pdqsort almost always takes the partialInsertionSort path, whose effect
// is a stable move of one element; that case is handled with a vector search + rotate (O(distance/64) wave steps).
// Every other path (pivot samples that see the defect, 12 < n < 50, ...) runs the full algorithm below with its
// sequential scans replaced by ballot searches. Keys are the per-position pod counts; `ord` holds the claim id at
// each position and `pos` its inverse.
//
// The algorithm is written once (PdqSort) over the thing that holds the array: ClaimOrder (arrays in LDS or HBM) or
// RegOrder (at most 64 claims in two vector registers of the wavefront).
#pragma once
#include "wave.h"

namespace ks {

// The algorithm, written once over an accessor S that holds the array: ClaimOrder below (the arrays in LDS or HBM) and
// RegOrder (at most 64 claims, one per lane, in two vector registers). S provides
//   n, defect, defect_append, slow_sorts          the state sort.Slice is called on (see ClaimOrder)
//   key_at(i), less(i, j), swap(i, j)             wave-uniform element access
//   FrameStack                                    where the explicit stack of waiting calls lives: push(sp, frame), pop(sp)
//   rotate_right(to, from), rotate_left(from, to, same_keys)   the stable move of one element
//   first_ge / first_gt / last_le / last_lt (lo, hi, v)         Go's sequential scans, "key OP v" over [lo, hi)
//   first_descent(lo, hi)                         first x with key[x] < key[x-1]
//   first_ge_sorted / last_le_sorted              the same answers as first_ge / last_le over a range known to be sorted
// Comparisons, swaps, `limit` and the xorshift are the same for every accessor: the unstable permutation is the result.
struct PdqFrame { int a, b, limit; bool was_balanced, was_partitioned; };   // a pdqsort call that waits for its recursive call
struct PdqFrameArray {   // the explicit stack, in memory (scratch on the device)
  PdqFrame f[40];
  KS_FN void push(int sp, const PdqFrame& x) { f[sp] = x; }
  KS_FN PdqFrame pop(int sp) const { return f[sp]; }
};

template <class S>
struct PdqSort {
  static KS_FN int bits_len(unsigned x) { return x ? 32 - __builtin_clz(x) : 0; }

  static KS_FN void insertion_sort(S& s, int a, int b) {
    for (int i = a + 1; i < b; i++)
      for (int j = i; j > a && s.less(j, j - 1); j--) s.swap(j, j - 1);
  }
  static KS_FN void sift_down(S& s, int lo, int hi, int first) {
    int root = lo;
    for (;;) {
      int child = 2 * root + 1;
      if (child >= hi) return;
      if (child + 1 < hi && s.less(first + child, first + child + 1)) child++;
      if (!s.less(first + root, first + child)) return;
      s.swap(first + root, first + child);
      root = child;
    }
  }
  static KS_FN void heap_sort(S& s, int a, int b) {
    int first = a, lo = 0, hi = b - a;
    for (int i = (hi - 1) / 2; i >= 0; i--) sift_down(s, i, hi, first);
    for (int i = hi - 1; i >= 0; i--) { s.swap(first, first + i); sift_down(s, lo, i, first); }
  }
  // order2/median on preloaded keys: indices are permuted, data is not touched
  static KS_FN void order2(int& a, int& b, uint32_t& ka, uint32_t& kb, int& swaps) {
    if (kb < ka) { swaps++; int t = a; a = b; b = t; uint32_t tk = ka; ka = kb; kb = tk; }
  }
  static KS_FN void median3(int a, int b, int c, uint32_t ka, uint32_t kb, uint32_t kc, int& swaps, int& out, uint32_t& kout) {
    order2(a, b, ka, kb, swaps); order2(b, c, kb, kc, swaps); order2(a, b, ka, kb, swaps);
    out = b; kout = kb;
  }
  static KS_FN int choose_pivot(S& s, int a, int b, int& hint) {  // hint: 0 unknown, 1 increasing, 2 decreasing
    int l = b - a, swaps = 0;
    int i = a + l / 4 * 1, j = a + l / 4 * 2, k = a + l / 4 * 3;
    if (l >= 8) {
      uint32_t ki, kj, kk;
      if (l >= 50) {
        uint32_t s0 = s.key_at(i - 1), s1 = s.key_at(i), s2 = s.key_at(i + 1), s3 = s.key_at(j - 1), s4 = s.key_at(j), s5 = s.key_at(j + 1), s6 = s.key_at(k - 1), s7 = s.key_at(k), s8 = s.key_at(k + 1);
        int oi, oj, ok;
        median3(i - 1, i, i + 1, s0, s1, s2, swaps, oi, ki);
        median3(j - 1, j, j + 1, s3, s4, s5, swaps, oj, kj);
        median3(k - 1, k, k + 1, s6, s7, s8, swaps, ok, kk);
        i = oi; j = oj; k = ok;
      } else { ki = s.key_at(i); kj = s.key_at(j); kk = s.key_at(k); }
      int oj2; uint32_t dummy;
      median3(i, j, k, ki, kj, kk, swaps, oj2, dummy);
      j = oj2;
    }
    hint = swaps == 0 ? 1 : (swaps == 12 ? 2 : 0);
    return j;
  }
  static KS_FN void reverse_range(S& s, int a, int b) { int i = a, j = b - 1; while (i < j) { s.swap(i, j); i++; j--; } }

  // first x in [i,b) with key[x] < key[x-1]; at the top level the only possible descents are at the defect
  static KS_FN int next_descent(S& s, int i, int b, bool top) {
    if (top) {
      if (s.defect < 0) return b;
      for (int x = s.defect; x <= s.defect + 1; ++x) if (x >= i && x >= 1 && x < b && s.key_at(x) < s.key_at(x - 1)) return x;
      return b;
    }
    return s.first_descent(i, b);
  }
  static KS_FN bool partial_insertion_sort(S& s, int a, int b, bool top) {
    int i = a + 1;
    for (int step = 0; step < 5; step++) {
      i = next_descent(s, i, b, top);
      if (i == b) return true;
      if (b - a < 50) return false;
      if (top) {
        // Single known defect: Go's swap(i,i-1) + the two shift loops amount to ONE rotation of the touched claim to
        // its stable place (see the derivation in DESIGN.md §4); do it with one search + one rotate.
        if (s.defect_append) {           // i == n-1: the new claim moves left behind the last claim with <= its count
          uint32_t mv = s.key_at(i);
          int t = s.last_le(0, i, mv);
          s.rotate_right(t + 1, i);
        } else {                       // i == p+1: the incremented claim at p moves right past the claims with a smaller count
          uint32_t mv = s.key_at(i - 1);
          int e = s.first_ge(i, b, mv);
          s.rotate_left(i - 1, e - 1);
        }
        s.defect = -1;
        return true;
      }
      s.swap(i, i - 1);
      if (i - a >= 2) {  // shift the smaller one to the left (Go uses the absolute bound j >= 1)
        uint32_t mv = s.key_at(i - 1);
        int t = s.last_le(0, i - 1, mv);
        s.rotate_right(t + 1, i - 1);
      }
      if (b - i >= 2) {  // shift the greater one to the right
        uint32_t mv = s.key_at(i);
        int e = s.first_ge(i + 1, b, mv);
        s.rotate_left(i, e - 1);
      }
      if (top) s.defect = -1;  // the single defect is repaired: the rest of the array is known sorted
    }
    return false;
  }
  static KS_FN void break_patterns(S& s, int a, int b) {
    int length = b - a;
    if (length >= 8) {
      uint64_t r = (uint64_t)length;
      unsigned modulus = 1u << bits_len((unsigned)length);
      int idx = a + (length / 4) * 2 - 1;
      for (int t = 0; t < 3; t++) {
        r ^= r << 13; r ^= r >> 7; r ^= r << 17;
        int other = (int)((unsigned)r & (modulus - 1));
        if (other >= length) other -= length;
        s.swap(idx - 1 + t, a + other);
      }
    }
  }
  static KS_FN int partition_equal(S& s, int a, int b, int pivot) {
    s.swap(a, pivot);
    uint32_t pv = s.key_at(a);
    int i = a + 1, j = b - 1;
    for (;;) {
      i = s.first_gt(i, j + 1, pv);
      j = s.last_le(i, j + 1, pv);
      if (i > j) break;
      s.swap(i, j); i++; j--;
    }
    return i;
  }
  static KS_FN int partition(S& s, int a, int b, int pivot, bool& already) {
    s.swap(a, pivot);
    uint32_t pv = s.key_at(a);
    int i = a + 1, j = b - 1;
    i = s.first_ge(i, j + 1, pv);
    j = s.last_lt(i, j + 1, pv);
    if (i > j) { s.swap(j, a); already = true; return j; }
    s.swap(i, j); i++; j--;
    for (;;) {
      i = s.first_ge(i, j + 1, pv);
      j = s.last_lt(i, j + 1, pv);
      if (i > j) break;
      s.swap(i, j); i++; j--;
    }
    s.swap(j, a);
    already = false;
    return j;
  }

  typedef PdqFrame Frame;

  // pdqsort_func with the recursion turned into an explicit stack (the recursive call always takes the smaller
  // side, so the depth is bounded by log2 n).
  static KS_FN void pdqsort(S& s, int a0, int b0, int limit0) {
    typename S::FrameStack stack;
    int sp = 0;
    Frame cur{a0, b0, limit0, true, true};
    bool top = true;  // still the outermost call, nothing swapped yet
    for (;;) {
      bool done = false;
      for (;;) {
        int a = cur.a, b = cur.b;
        int length = b - a;
        if (length <= 12) { insertion_sort(s, a, b); done = true; break; }
        if (cur.limit == 0) { heap_sort(s, a, b); done = true; break; }
        if (!cur.was_balanced) { break_patterns(s, a, b); cur.limit--; }
        int hint;
        int pivot = choose_pivot(s, a, b, hint);
        if (hint == 2) { reverse_range(s, a, b); pivot = (b - 1) - (pivot - a); hint = 1; top = false; }
        if (cur.was_balanced && cur.was_partitioned && hint == 1) {
          if (partial_insertion_sort(s, a, b, top)) { done = true; break; }
        }
        if (top) s.slow_sorts++;  // the outermost call leaves the single-defect fast path: full pdqsort from here on
        top = false;
        if (a > 0 && !s.less(a - 1, pivot)) { cur.a = partition_equal(s, a, b, pivot); continue; }
        bool already;
        int mid = partition(s, a, b, pivot, already);
        cur.was_partitioned = already;
        int left_len = mid - a, right_len = b - mid;
        int balance_threshold = length / 8;
        Frame child;
        if (left_len < right_len) {
          cur.was_balanced = left_len >= balance_threshold;
          child = Frame{a, mid, cur.limit, true, true};
          cur.a = mid + 1;
        } else {
          cur.was_balanced = right_len >= balance_threshold;
          child = Frame{mid + 1, b, cur.limit, true, true};
          cur.b = mid;
        }
        stack.push(sp++, cur);  // the parent continues after the child has run to completion
        cur = child;
      }
      (void)done;
      if (sp == 0) break;
      cur = stack.pop(--sp);
    }
  }

  // sort.Slice on the current array
  static KS_FN void sort(S& s) {
    const int n = s.n;
    if (s.defect < 0 || n <= 1) { s.defect = -1; return; }  // sorted input: pdqsort performs no swap
    if (n <= 12) {
      // insertionSort_func is a stable sort; with a single defect that is one stable move
      if (s.defect_append) {
        uint32_t mv = s.key_at(n - 1);
        int t = s.last_le(0, n - 1, mv);
        s.rotate_right(t + 1, n - 1);
      } else {
        int p = s.defect;
        uint32_t mv = s.key_at(p);
        int e = s.first_ge(p + 1, n, mv);
        s.rotate_left(p, e - 1, true);   // everything between carries the claim's old count
      }
      s.defect = -1;
      return;
    }
    if (n >= 50) {
      // The outermost pdqsort call on "sorted except position p": choosePivot samples the keys around n/4, n/2 and 3n/4
      // (zsortfunc.go choosePivot_func); unless p is one of those nine positions every sampled comparison sees sorted
      // data, so swaps == 0, the hint is "increasing" and the call goes straight to partialInsertionSort, which repairs
      // the single defect with one stable move (see partial_insertion_sort). Skip the sampling in that case.
      const int q = n / 4, p = s.defect;
      const bool sampled = (p >= q - 1 && p <= q + 1) || (p >= 2 * q - 1 && p <= 2 * q + 1) || (p >= 3 * q - 1 && p <= 3 * q + 1);
      if (!sampled) {
        // (both ranges are sorted: an accessor whose order lives in HBM, where runs of equally full claims can be tens of thousands
        // long, answers these two with a binary search)
        if (s.defect_append) {
          const int i = n - 1;
          if (i >= 1 && s.key_at(i) < s.key_at(i - 1)) {
            const uint32_t mv = s.key_at(i);
            const int t = s.last_le_sorted(0, i, mv);   // [0, i) is sorted
            s.rotate_right(t + 1, i);
          }
        } else if (p + 1 < n && s.key_at(p + 1) < s.key_at(p)) {
          const uint32_t mv = s.key_at(p);
          const int e = s.first_ge_sorted(p + 1, n, mv);   // [p+1, n) is sorted
          s.rotate_left(p, e - 1, true);   // everything between carries the claim's old count
        }
        s.defect = -1;
        return;
      }
    }
    pdqsort(s, 0, n, bits_len((unsigned)n));
    s.defect = -1;
  }
};

// P32 = pointer type of the three arrays: LDS for problems whose claims fit the CU's LDS, HBM for larger ones.
// POS = false drops the inverse array (the cursor engine always knows the position of the claim it touches).
// WIDE = the keys are 16-bit entries of a 16-byte aligned LDS array (the cursor engine's LDS plans): the scans read eight keys per lane.
template <class W, class P32 = KS_LDS uint32_t*, bool POS = true, bool WIDE = false>
struct ClaimOrder {
  P32 key;   // [cap] pod count of the claim at position i
  P32 ord;   // [cap] claim id at position i
  P32 pos;   // [cap] position of claim id
  int n = 0;
  int defect = -1;        // position whose key changed since the array was last sorted, -1 = sorted
  bool defect_append = false;
  uint64_t slow_sorts = 0;

  // ---- lookups (the BIG engine's RunOrder answers the same two questions from its rings) ----
  KS_FN uint32_t position(int c) const { return pos[c]; }
  KS_FN uint32_t claim_at(int i) const { return ord[i]; }
  // ---- element access (uniform) ----
  KS_FN bool less(int i, int j) const { return key[i] < key[j]; }
  KS_FN void swap(int i, int j) {
    if (i == j) return;
    uint32_t ki = key[i], kj = key[j], oi = ord[i], oj = ord[j];
    W::store(&key[i], kj); W::store(&key[j], ki);
    W::store(&ord[i], oj); W::store(&ord[j], oi);
    if constexpr (POS) { W::store(&pos[oj], (uint32_t)i); W::store(&pos[oi], (uint32_t)j); }
    W::sync();
  }
  // move element at `from` to `to` (to < from), shifting [to, from) right by one
  KS_FN void rotate_right(int to, int from) {
    if (to >= from) return;
    uint32_t mk = key[from], mo = ord[from];
    for (int top = from; top > to; top -= kRound) {  // high to low so a round never reads what an earlier round wrote
      int lo = top - kRound > to ? top - kRound : to;
      shift_round(lo, top, +1, false);
    }
    W::store(&key[to], mk); W::store(&ord[to], mo); if constexpr (POS) W::store(&pos[mo], (uint32_t)to);
    W::sync();
  }
  // move element at `from` to `to` (to > from), shifting (from, to] left by one. same_keys: the elements that shift all carry
  // ONE count (the stable move of a claim that gained a pod passes claims of exactly its old count): their keys need not
  // move at all — one key written at each end instead of one per element.
  KS_FN void rotate_left(int from, int to, bool same_keys = false) {
    if (to <= from) return;
    uint32_t mk = key[from], mo = ord[from];
    const uint32_t passed = key[from + 1];
    for (int lo = from + 1; lo <= to; lo += kRound) {
      int hi = lo + kRound <= to + 1 ? lo + kRound : to + 1;
      shift_round(lo, hi, -1, same_keys);
    }
    if (same_keys) W::store(&key[from], passed);
    W::store(&key[to], mk); W::store(&ord[to], mo); if constexpr (POS) W::store(&pos[mo], (uint32_t)to);
    W::sync();
  }
  // elements [lo,hi) (at most kRound) move by delta (+1 / -1): all reads of the round precede its writes, and
  // all of them are in flight together (a long move — tens of thousands of equally full claims — is bound by round trips)
  static constexpr int kPerLane = sizeof(P32) == 8 ? 16 : 1;   // HBM-resident order (64-bit pointers): sixteen elements per lane per round
  static constexpr int kRound = 64 * kPerLane;
  // searches over the order: one round trip per 64 elements in LDS; eight rounds in flight over an HBM-resident order
  template <class F> KS_FN int ff(int lo, int hi, F pred) const { if constexpr (kPerLane > 1) return W::find_first8(lo, hi, pred); else return W::find_first(lo, hi, pred); }
  template <class F> KS_FN int fl(int lo, int hi, F pred) const { if constexpr (kPerLane > 1) return W::find_last8(lo, hi, pred); else return W::find_last(lo, hi, pred); }
  KS_FN void shift_round(int lo, int hi, int delta, bool same_keys) {
#if KS_DEVICE
    uint32_t k[kPerLane], o[kPerLane];
    if (same_keys) {
#pragma unroll
      for (int j = 0; j < kPerLane; ++j) { const int i = lo + j * 64 + W::lane(); if (i < hi) o[j] = ord[i]; }
      W::sync();
#pragma unroll
      for (int j = 0; j < kPerLane; ++j) { const int i = lo + j * 64 + W::lane(); if (i < hi) { ord[i + delta] = o[j]; if constexpr (POS) pos[o[j]] = (uint32_t)(i + delta); } }
      W::sync();
      return;
    }
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) { const int i = lo + j * 64 + W::lane(); if (i < hi) { k[j] = key[i]; o[j] = ord[i]; } }
    W::sync();
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) { const int i = lo + j * 64 + W::lane(); if (i < hi) { key[i + delta] = k[j]; ord[i + delta] = o[j]; if constexpr (POS) pos[o[j]] = (uint32_t)(i + delta); } }
    W::sync();
#else
    if (delta > 0) for (int i = hi - 1; i >= lo; --i) { if (!same_keys) key[i + 1] = key[i]; ord[i + 1] = ord[i]; if constexpr (POS) pos[ord[i + 1]] = i + 1; }
    else for (int i = lo; i < hi; ++i) { if (!same_keys) key[i - 1] = key[i]; ord[i - 1] = ord[i]; if constexpr (POS) pos[ord[i - 1]] = i - 1; }
#endif
  }
  // first x in [lo,hi) with key[x] >= v, hi if none — [lo,hi) is sorted ascending (binary search: a long run of equal keys
  // costs log2 n round trips instead of n/64)
  KS_FN int lower_bound_sorted(int lo, int hi, uint32_t v) const {
    while (lo < hi) { const int mid = lo + (hi - lo) / 2; if (key[mid] < v) lo = mid + 1; else hi = mid; }
    return lo;
  }
  // last x in [lo,hi) with key[x] <= v, lo-1 if none — [lo,hi) sorted ascending
  KS_FN int upper_last_sorted(int lo, int hi, uint32_t v) const {
    int a = lo, b = hi;
    while (a < b) { const int mid = a + (b - a) / 2; if (!(v < key[mid])) a = mid + 1; else b = mid; }
    return a - 1;
  }

  // ---- the scans of Go's pdqsort (PdqSort above), as searches ----
  KS_FN uint32_t key_at(int i) const { return key[i]; }
  typedef PdqFrameArray FrameStack;
  // every scan is "key OP v" or "key[x] < key[x-1]": pred(key, the key one position down)
  template <bool LAST, bool PREV, class F> KS_FN int scan(int lo, int hi, F pred) const {
    if constexpr (WIDE) return wide_scan<LAST, PREV>(lo, hi, pred);
    else {
      const P32 kp = key;
      auto at = [kp, pred](int x) { return pred((uint32_t)kp[x], PREV ? (uint32_t)kp[x - 1] : 0u); };
      if constexpr (LAST) return fl(lo, hi, at); else return ff(lo, hi, at);
    }
  }
  KS_FN int first_ge(int lo, int hi, uint32_t v) const { return scan<false, false>(lo, hi, [v](uint32_t k, uint32_t) { return !(k < v); }); }
  KS_FN int first_gt(int lo, int hi, uint32_t v) const { return scan<false, false>(lo, hi, [v](uint32_t k, uint32_t) { return v < k; }); }
  KS_FN int last_le(int lo, int hi, uint32_t v) const { return scan<true, false>(lo, hi, [v](uint32_t k, uint32_t) { return !(v < k); }); }
  KS_FN int last_lt(int lo, int hi, uint32_t v) const { return scan<true, false>(lo, hi, [v](uint32_t k, uint32_t) { return k < v; }); }
  KS_FN int first_descent(int lo, int hi) const { return scan<false, true>(lo, hi, [](uint32_t k, uint32_t below) { return k < below; }); }   // lo >= 1
  // The wide form, 512 positions per LDS round trip where ff / fl take 64: every lane reads one aligned 16-byte piece (eight 16-bit
  // keys; a piece that reaches past the range is read whole, as the cursor engine's snapshot compare does), evaluates the predicate
  // on its eight keys into an 8-bit mask and masks the range ends off; the answer is the first (last) set bit of the first (last)
  // lane with any. "The key one position down" of a piece's first key is the last key of the lane below (a cross-lane move), and
  // for lane 0 key[base - 1], read once per step. A full scan of 2,763 keys is 6 dependent reads instead of 44.
  template <bool LAST, bool PREV, class F> KS_FN int wide_scan(int lo, int hi, F pred) const {
    if (lo >= hi) return LAST ? lo - 1 : hi;
    const int rlo = PREV ? lo - 1 : lo;   // lowest position that is read
    const auto pieces = pieces16(key);
    const P32 kp = key;
    const int base_lo = rlo & ~511, base_hi = (hi - 1) & ~511;
    for (int base = LAST ? base_hi : base_lo; LAST ? base >= base_lo : base <= base_hi; base += LAST ? -512 : 512) {
      LaneVar<uint32_t> w0, w1, w2, w3, dn, m8;
      const uint32_t under = (PREV && base > 0) ? (uint32_t)kp[base - 1] : 0u;
      W::each([&](int l) {
        const int e = base + 8 * l;
        w0.at(l) = 0; w1.at(l) = 0; w2.at(l) = 0; w3.at(l) = 0;
        if (e < hi && e + 7 >= rlo) { const u32x4_alias x = pieces[(base >> 3) + l]; w0.at(l) = x[0]; w1.at(l) = x[1]; w2.at(l) = x[2]; w3.at(l) = x[3]; }
      });
      if constexpr (PREV) {   // (the exchange runs on every lane: a lane switched off during the cross-lane move reads as zero for its neighbour)
        LaneVar<uint32_t> up;
        W::each([&](int l) { up.at(l) = w3.shuffle(l, (l + 63) & 63); });
        W::each([&](int l) { dn.at(l) = l ? up.at(l) >> 16 : under; });
      }
      W::each([&](int l) {
        const int e = base + 8 * l;
        const uint32_t w[4] = {w0.at(l), w1.at(l), w2.at(l), w3.at(l)};
        uint32_t below = 0, m = 0;
        if constexpr (PREV) below = dn.at(l);
#pragma unroll
        for (int j = 0; j < 8; ++j) { const uint32_t kx = (w[j >> 1] >> (16 * (j & 1))) & 0xFFFFu; m |= (pred(kx, below) ? 1u : 0u) << j; below = kx; }
        const int a = lo - e, b = hi - e;   // keys [a, b) of the piece lie inside [lo, hi): the range ends are masked, not branched
        const uint32_t in = (b >= 8 ? 0xFFu : b <= 0 ? 0u : (1u << b) - 1u) & (a <= 0 ? 0xFFu : a >= 8 ? 0u : (0xFFu << a) & 0xFFu);
        m8.at(l) = m & in;
      });
      const uint64_t any = W::ballot([&](int l) { return m8.at(l) != 0; });
      if (any) {
        const int who = LAST ? 63 - __builtin_clzll(any) : ctz64(any);
        const uint32_t bits = m8.bcast(who);
        return base + 8 * who + (LAST ? 31 - __builtin_clz(bits) : __builtin_ctz(bits));
      }
    }
    return LAST ? lo - 1 : hi;
  }
  // over a sorted range. LDS-resident order: a vector search (usually one round); HBM-resident order: runs of equally full claims
  // can be tens of thousands long, binary search instead
  KS_FN int first_ge_sorted(int lo, int hi, uint32_t v) const { return kPerLane > 1 ? lower_bound_sorted(lo, hi, v) : first_ge(lo, hi, v); }
  KS_FN int last_le_sorted(int lo, int hi, uint32_t v) const { return kPerLane > 1 ? upper_last_sorted(lo, hi, v) : last_le(lo, hi, v); }

  // ---- mutation by the scheduler ----
  KS_FN void increment(int claim) {  // a pod was added to an in-flight claim (nodeclaim.go:249)
    int p = (int)pos[claim];
    W::store(&key[p], key[p] + 1);
    W::sync();
    defect = p; defect_append = false;
  }
  KS_FN void append(int claim) {     // a new claim with its first pod (scheduler.go:785)
    W::store(&key[n], 1u); W::store(&ord[n], (uint32_t)claim); if constexpr (POS) W::store(&pos[claim], (uint32_t)n);
    W::sync();
    defect = n; defect_append = true;
    n++;
  }

  // sort.Slice on the current array
  KS_FN void sort() { PdqSort<ClaimOrder>::sort(*this); }
};

// An order of at most 64 claims held by one wavefront, lane i = position i: key and claim id in two vector registers
// (arrays of 64 in the host emulation). Element access is v_readlane / v_writelane with wave-uniform indices, a scan is one
// ballot, a stable move one cross-lane permute of each register: between load() and store() the sort touches no memory and
// waits for none. The cursor engine sorts its small orders here (fast_engine.h slow_sort): with 12 < n < 50 Go's pdqsort has
// no single-move shortcut, so every re-sort with something to move is the full algorithm.
template <class W>
struct RegOrder {
  LaneVar<uint32_t> k, o;   // key / claim id of position lane; lanes >= n hold copies of position 0 and are never looked at
  int n = 0;
  int defect = -1;
  bool defect_append = false;
  uint64_t slow_sorts = 0;

  template <class P> KS_FN void load(P key, P ord, int n_) {
    n = n_;
    W::each([&](int l) { const int i = l < n_ ? l : 0; k.at(l) = key[i]; o.at(l) = ord[i]; });
  }
  template <class P> KS_FN void store(P key, P ord) {
    const int n_ = n;
    W::each([&](int l) { if (l < n_) { key[l] = k.at(l); ord[l] = o.at(l); } });
    W::sync();
  }
  // ---- element access (uniform) ----
  KS_FN uint32_t key_at(int i) const { return k.bcast(i); }
  // pdqsort's waiting calls, one per lane of a register: positions are at most 64 (7 bits each), `limit` at most bits_len(64) = 7, and
  // the recursion takes the smaller side, so there are at most log2(64) + 1 of them. (In scratch every return would be a trip to memory.)
  struct FrameStack {
    LaneVar<uint32_t> v;
    KS_FN void push(int sp, const PdqFrame& x) { v.set(sp, (uint32_t)x.a | ((uint32_t)x.b << 7) | ((uint32_t)x.limit << 14) | ((uint32_t)x.was_balanced << 18) | ((uint32_t)x.was_partitioned << 19)); }
    KS_FN PdqFrame pop(int sp) const {
      const uint32_t p = v.bcast(sp);
      return PdqFrame{(int)(p & 127u), (int)((p >> 7) & 127u), (int)((p >> 14) & 15u), ((p >> 18) & 1u) != 0, ((p >> 19) & 1u) != 0};
    }
  };
  KS_FN bool less(int i, int j) const { return k.bcast(i) < k.bcast(j); }
  KS_FN void swap(int i, int j) {
    if (i == j) return;
    const uint32_t ki = k.bcast(i), kj = k.bcast(j), oi = o.bcast(i), oj = o.bcast(j);
    W::each([&](int l) { k.at(l) = l == i ? kj : l == j ? ki : k.at(l); o.at(l) = l == i ? oj : l == j ? oi : o.at(l); });   // (two compares and four selects: fewer instructions than four v_writelane with their lane selects)
  }
  // position l takes the element of position src(l): every lane reads before any lane is written
  template <class F> KS_FN void permute(F src) {
    LaneVar<uint32_t> tk, to;
    W::each([&](int l) { const int from = src(l); tk.at(l) = k.shuffle(l, from); to.at(l) = o.shuffle(l, from); });
    W::each([&](int l) { k.at(l) = tk.at(l); o.at(l) = to.at(l); });
  }
  KS_FN void rotate_right(int to, int from) {
    if (to >= from) return;
    permute([to, from](int l) { return l == to ? from : (l > to && l <= from) ? l - 1 : l; });
  }
  KS_FN void rotate_left(int from, int to, bool = false) {   // (equal keys that pass each other: the same registers either way)
    if (to <= from) return;
    permute([to, from](int l) { return l == to ? from : (l >= from && l < to) ? l + 1 : l; });
  }
  // ---- searches: one ballot over the lanes of [lo, hi); an empty range answers like Wave::find_first / find_last ----
  template <class F> KS_FN int first(int lo, int hi, F pred) const {
    const uint64_t m = W::ballot([&](int l) { return l >= lo && l < hi && pred(l); });
    return m ? ctz64(m) : hi;
  }
  template <class F> KS_FN int last(int lo, int hi, F pred) const {
    const uint64_t m = W::ballot([&](int l) { return l >= lo && l < hi && pred(l); });
    return m ? 63 - __builtin_clzll(m) : lo - 1;
  }
  KS_FN int first_ge(int lo, int hi, uint32_t v) const { return first(lo, hi, [&](int l) { return !(k.v_of(l) < v); }); }
  KS_FN int first_gt(int lo, int hi, uint32_t v) const { return first(lo, hi, [&](int l) { return v < k.v_of(l); }); }
  KS_FN int last_le(int lo, int hi, uint32_t v) const { return last(lo, hi, [&](int l) { return !(v < k.v_of(l)); }); }
  KS_FN int last_lt(int lo, int hi, uint32_t v) const { return last(lo, hi, [&](int l) { return k.v_of(l) < v; }); }
  KS_FN int first_descent(int lo, int hi) const {
    LaneVar<uint32_t> below;   // the key one position down (lane 0 wraps round and is masked: a descent needs x >= 1)
    W::each([&](int l) { below.at(l) = k.shuffle(l, (l + 63) & 63); });
    return first(lo, hi, [&](int l) { return l >= 1 && k.v_of(l) < below.v_of(l); });
  }
  KS_FN int first_ge_sorted(int lo, int hi, uint32_t v) const { return first_ge(lo, hi, v); }
  KS_FN int last_le_sorted(int lo, int hi, uint32_t v) const { return last_le(lo, hi, v); }

  KS_FN void sort() { PdqSort<RegOrder>::sort(*this); }
};

// arr[b+1 .. a] = arr[b .. a-1] for an LDS-resident array of 16-bit entries, 512 entries per step: every lane takes a 16-byte
// piece (eight entries), shifts it by one entry through its registers (the entry that crosses into the piece comes from the lane
// below it) and writes it back in place — from the top piece down, so that a step reads nothing an earlier step wrote. The
// one-entry-per-lane move this replaces cost a new claim's sort.Slice 43 dependent read-write rounds at 2,763 claims.
template <class W>
KS_DEV void shift_right16(KS_LDS uint16_t* arr, int b, int a) {
  KS_LDS u32x4_alias* const v = (KS_LDS u32x4_alias*)arr;
  const KS_LDS uint32_t* const dw = (const KS_LDS uint32_t*)arr;
  for (int e0 = a & ~511; e0 >= 0 && e0 + 511 >= b; e0 -= 512) {
    LaneVar<uint32_t> d0, d1, d2, d3, pv;
    const uint32_t below = e0 > 0 ? dw[(e0 >> 1) - 1] : 0u;      // the two entries under the step's first piece
    W::each([&](int l) {
      const int e = e0 + 8 * l;
      d0.at(l) = 0; d1.at(l) = 0; d2.at(l) = 0; d3.at(l) = 0;
      if (e <= a && e + 7 >= b) { const u32x4_alias x = v[(e0 >> 3) + l]; d0.at(l) = x[0]; d1.at(l) = x[1]; d2.at(l) = x[2]; d3.at(l) = x[3]; }
    });
    // (the exchange runs on EVERY lane, then lane 0 takes the word below the step: a lane that is switched off during ds_bpermute
    // reads as zero for its neighbour — the first build had the exchange inside the select and lane 1 got a zero from lane 0)
    LaneVar<uint32_t> up;
    W::each([&](int l) { up.at(l) = d3.shuffle(l, (l + 63) & 63); });
    W::each([&](int l) { pv.at(l) = l ? up.at(l) : below; });
    W::each([&](int l) {
      const int e = e0 + 8 * l;
      if (!(e <= a && e + 7 > b)) return;
      auto mix = [&](uint32_t cur, uint32_t prev, int elo) {   // entries elo (low half) and elo + 1 (high half) of one word
        const uint32_t sh = (cur << 16) | (prev >> 16);
        const uint32_t m = ((elo > b && elo <= a) ? 0xFFFFu : 0u) | ((elo + 1 > b && elo + 1 <= a) ? 0xFFFF0000u : 0u);
        return (sh & m) | (cur & ~m);
      };
      u32x4_alias y;
      y[0] = mix(d0.at(l), pv.at(l), e); y[1] = mix(d1.at(l), d0.at(l), e + 2); y[2] = mix(d2.at(l), d1.at(l), e + 4); y[3] = mix(d3.at(l), d2.at(l), e + 6);
      v[(e0 >> 3) + l] = y;
    });
    W::sync();
  }
}

}  // namespace ks
