// pack_kernels.h — the pack kernels (one wavefront per scheduling problem) live in translation units of their own, so that build()
// compiles them side by side (the general engine's instantiations alone are minutes of one hipcc): the general engine's
// ksolve_pack_general.hip, ksolve_pack_batch.hip and ksolve_pack_sweep4.hip, the node stage's ksolve_pack_nodes.hip, ksolve_pack_topo_nodes_pn.hip, and the three
// units of the fast engines — ksolve_pack_fast.hip, ksolve_pack_topo.hip, ksolve_pack_topo_many.hip — each compiled once per flavour.
// The fast engines' kernels are declared from the lists of pack_flavours.h, which the units define them from. ksolve.hip (the HIP
// backend of the C ABI) launches them through these declarations; no device function crosses a translation unit.
#pragma once
#include <hip/hip_runtime.h>
#include "engine.h"
#include "fast_engine.h"
#include "node_stage.h"
#include "topo_types.h"
#include "pack_flavours.h"

__global__ void ksolve_pack(ks::ProblemView pv, ks::Workspace ws);
__global__ void ksolve_pack_lite(ks::ProblemView pv, ks::Workspace ws);
__global__ void ksolve_pack_big(ks::ProblemView pv, ks::Workspace ws);
__global__ void ksolve_pack_batch(ks::BatchItem* items);
__global__ void ksolve_pack_batch_lite(ks::BatchItem* items);
__global__ void ksolve_pack_sweep(const ks::ProblemView* pv, ks::Workspace* items, int n, ks::LdsPlan plan);
__global__ void ksolve_pack_sweep4(const ks::ProblemView* pv, ks::Workspace* items, int n, ks::LdsPlan plan, const uint32_t* order, uint32_t* next);
// the cursor engine per flavour, memory plan and rows of class slots; the two-wavefront kernel and the batched form of the plain flavour
typedef void (*ksolve_pack_fast_fn)(const ks::FastArgs*);
#define KS_DECLARE(NAME, FL, GS, R) __global__ void NAME(const ks::FastArgs* a);
KS_PACK_FAST_ROWS(KS_DECLARE)
#undef KS_DECLARE
__global__ void ksolve_pack_fast2(const ks::FastArgs* a);
__global__ void ksolve_pack_fast_batch(const ks::FastArgs* const* items);
// the spread engine per flavour, without / with existing nodes
typedef void (*ksolve_pack_topo_fn)(const ks::TopoArgs*);
#define KS_DECLARE(NAME, FL, ND) __global__ void NAME(const ks::TopoArgs* a);
KS_PACK_TOPO_ROWS(KS_DECLARE)
#undef KS_DECLARE
__global__ void ksolve_pack_topo_nodes_pn(const ks::TopoArgs* a);   // engines 35 / 36, outside the matrix (ksolve_pack_topo_nodes_pn.hip)
// ... many problems per launch (ksolve_solve_many; topo_many.h: block = one ticket = one member, largest first)
typedef void (*ksolve_pack_topo_many_fn)(const ks::TopoArgs* const*, const uint32_t*, uint32_t*, int);
#define KS_DECLARE(NAME, FL, ND) __global__ void NAME(const ks::TopoArgs* const* items, const uint32_t* order, uint32_t* next, int n);
KS_PACK_TOPO_MANY_ROWS(KS_DECLARE)
#undef KS_DECLARE
// the cursor engine's existing-node stage (node_stage.h), `remaining` in LDS / in the HBM workspace
__global__ void ksolve_pack_nodes_lds(const ks::FastArgs* a);
__global__ void ksolve_pack_nodes_hbm(const ks::FastArgs* a);
__global__ void ksolve_pack_nodes_lds_p(const ks::FastArgs* a);
__global__ void ksolve_pack_nodes_hbm_p(const ks::FastArgs* a);
#ifdef KSOLVE_TEST_HOOKS
// test builds only: FastCold alone, per instantiation (ksolve_test_fast_cold.hip, fast_cold_probe.h)
namespace ks { struct FastColdArgs; }
typedef void (*ksolve_test_fast_cold_fn)(const ks::FastColdArgs*);
#define KS_DECLARE(NAME, FL, GS, R) __global__ void NAME(const ks::FastColdArgs* a);
KS_FAST_COLD_ROWS(KS_DECLARE)
#undef KS_DECLARE
#endif
