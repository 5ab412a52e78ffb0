// topo_many.h — the spread engine, many problems per launch (ksolve_solve_many): what the six ksolve_pack_topo*_many kernels share.
// Grid = members of the launch, one wavefront each. A block does not solve member blockIdx.x: it takes a ticket from the launch's
// counter and solves member order[ticket] — the host fills `order` with the members by pod count, largest first, and HIP promises no
// dispatch order, so the ticket is what makes "largest first" hold when the launch has more members than the chip holds at once (the
// launch then lasts about as long as its largest member, not as long as the unluckiest CU's share). The ticket is handed out exactly
// as ksolve_pack_sweep4 hands out probes: lane 0's atomicAdd on the counter in HBM, the value broadcast with readfirstlane.
// From there on the block IS the single-problem kernel: TopoEngine on its member's record, each engine reading its own tw.plan
// offsets (the launch's dynamic LDS is the largest member's plan).
#pragma once
#include <hip/hip_runtime.h>
#include "topo_types.h"

namespace ks {

// the member this block solves, or null (a ticket past the end: the grid is the member count, so none is)
__device__ __forceinline__ const TopoArgs* topo_many_take(const TopoArgs* const* items, const uint32_t* order, uint32_t* next, int n) {
  unsigned t = 0;
  if (threadIdx.x == 0) t = atomicAdd(next, 1u);
  t = (unsigned)__builtin_amdgcn_readfirstlane((int)t);
  if (t >= (unsigned)n) return nullptr;
  const unsigned m = (unsigned)__builtin_amdgcn_readfirstlane((int)order[t]);
  if (m >= (unsigned)n) return nullptr;
  // (readfirstlane on the halves: the record's address is wave-uniform, and the engine's reads through it stay scalar as in the single-problem kernels)
  const uint64_t p = (uint64_t)items[m];
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)p), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(p >> 32));
  return (const TopoArgs*)(((uint64_t)hi << 32) | lo);
}

}  // namespace ks
