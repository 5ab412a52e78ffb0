// Makes tests/golden/pdqsort_killer_1000.json: n distinct keys on which Go's pdqsort (csrc/go_sort.h) runs out of its bad-partition
// allowance and falls back to heapsort — the one path of go_sort.h no pattern of the price families reaches at 1,000 types. The keys
// come from McIlroy's adversary ("A Killer Adversary for Quicksort", 1999) played against go_sort.h itself: a key stays undecided
// ("gas") until a comparison needs it, and is then frozen at the lowest value still free, so that every pivot ends up among the
// smallest keys of its range. A tool, not a test:
//     g++ -O2 -std=c++17 -o /tmp/pdqsort_killer tests/tools/pdqsort_killer.cpp && /tmp/pdqsort_killer 1000 2 > tests/golden/pdqsort_killer_1000.json
// (`pdqsort_killer 64 2` made tests/golden/pdqsort_killer_64.json: heap_sort within the 64 claims RegOrder holds, tests/wave_order_cases.py.)
// It prints to stderr how many comparisons the replay of the finished keys takes (25,744 at 1,000 keys, against some 7,000 where the
// allowance is never used up). tests/tools/result_mutations.py shows that the heapsort runs: without it the case `heapsort` fails.
#define KSOLVE_HOST_EMULATION 1
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>
#include "../../karpenter_amd/csrc/go_sort.h"

int main(int argc, char** argv) {
  const int n = argc > 1 ? atoi(argv[1]) : 1000;
  const int d = argc > 2 ? atoi(argv[2]) : 2;   // keys are frozen values / d: ties, without which every correct sort leaves the same order
  const int gas = n;
  std::vector<int> val(n, gas), item(n);
  std::iota(item.begin(), item.end(), 0);
  int nsolid = 0, candidate = 0;
  // (a few keys frozen out of order first: on keys that are all undecided the adversary answers "sorted already", and pdqsort's partial
  // insertion sort ends the game in one pass)
  for (int i = 0; i < 8 && i < n; ++i) val[i * (n / 8)] = 7 - i;
  nsolid = 8;
  auto cmp = [&](int x, int y) {
    if (val[x] == gas && val[y] == gas) { if (x == candidate) val[x] = nsolid++; else val[y] = nsolid++; }
    if (val[x] == gas) candidate = x; else if (val[y] == gas) candidate = y;
    return val[x] / d < val[y] / d;   // (gas / d is above every frozen key)
  };
  ks::go_sort_slice(n, [&](int i, int j) { return cmp(item[i], item[j]); }, [&](int i, int j) { std::swap(item[i], item[j]); });
  for (int i = 0; i < n; ++i) if (val[i] == gas) val[i] = nsolid++;
  // replay: count the comparisons (quadratic behaviour shows as far more than n log n; heapsort bounds it)
  for (int& v : val) v /= d;
  std::vector<int> k(val);
  long long compares = 0;
  ks::go_sort_slice(n, [&](int i, int j) { ++compares; return k[i] < k[j]; }, [&](int i, int j) { std::swap(k[i], k[j]); });
  fprintf(stderr, "%d keys, %lld comparisons in the replay\n", n, compares);
  printf("[");
  for (int i = 0; i < n; ++i) printf("%s%d", i ? ", " : "", val[i]);
  printf("]\n");
  return 0;
}
