// pack_kernels.h — the pack kernels (one wavefront per scheduling problem) live in translation units of their own, so that build()
// compiles them side by side (the general engine's instantiations alone are minutes of one hipcc): ksolve_pack_general.hip,
// ksolve_pack_batch.hip, ksolve_pack_sweep4.hip, ksolve_pack_fast.hip, ksolve_pack_fast_unsched.hip, ksolve_pack_fast_podops.hip, ksolve_pack_nodes.hip, ksolve_pack_topo.hip, ksolve_pack_topo_nodes.hip, ksolve_pack_topo_unsched.hip, ksolve_pack_topo_filter.hip, ksolve_pack_topo_podops.hip, ksolve_pack_topo_many.hip, ksolve_pack_topo_many_unsched.hip, ksolve_pack_topo_many_filter.hip. ksolve.hip (the HIP backend of the C
// ABI) launches them through these declarations; no device function crosses a translation unit.
#pragma once
#include <hip/hip_runtime.h>
#include "engine.h"
#include "fast_engine.h"
#include "node_stage.h"
#include "topo_types.h"

__global__ void ksolve_pack(ks::ProblemView pv, ks::Workspace ws);
__global__ void ksolve_pack_lite(ks::ProblemView pv, ks::Workspace ws);
__global__ void ksolve_pack_big(ks::ProblemView pv, ks::Workspace ws);
__global__ void ksolve_pack_batch(ks::BatchItem* items);
__global__ void ksolve_pack_batch_lite(ks::BatchItem* items);
__global__ void ksolve_pack_sweep(const ks::ProblemView* pv, ks::Workspace* items, int n, ks::LdsPlan plan);
__global__ void ksolve_pack_sweep4(const ks::ProblemView* pv, ks::Workspace* items, int n, ks::LdsPlan plan, const uint32_t* order, uint32_t* next);
// the cursor engine per memory plan (g: FastPlan::global_state) and rows of class slots (r: 1 or ks::kFastRows)
__global__ void ksolve_pack_fast_g0r1(const ks::FastArgs* a);
__global__ void ksolve_pack_fast_g1r1(const ks::FastArgs* a);
__global__ void ksolve_pack_fast_g2r1(const ks::FastArgs* a);
__global__ void ksolve_pack_fast_g0r4(const ks::FastArgs* a);
__global__ void ksolve_pack_fast_g1r4(const ks::FastArgs* a);
__global__ void ksolve_pack_fast_g2r4(const ks::FastArgs* a);
// ... and the same six with the set-aside list of engines 20 / 21 compiled in (ksolve_pack_fast_unsched.hip)
__global__ void ksolve_pack_fast_u_g0r1(const ks::FastArgs* a);
__global__ void ksolve_pack_fast_u_g1r1(const ks::FastArgs* a);
__global__ void ksolve_pack_fast_u_g2r1(const ks::FastArgs* a);
__global__ void ksolve_pack_fast_u_g0r4(const ks::FastArgs* a);
__global__ void ksolve_pack_fast_u_g1r4(const ks::FastArgs* a);
__global__ void ksolve_pack_fast_u_g2r4(const ks::FastArgs* a);
// ... and the same six with the pod operators of engines 26 / 27 compiled in as well (ksolve_pack_fast_podops.hip)
__global__ void ksolve_pack_fast_p_g0r1(const ks::FastArgs* a);
__global__ void ksolve_pack_fast_p_g1r1(const ks::FastArgs* a);
__global__ void ksolve_pack_fast_p_g2r1(const ks::FastArgs* a);
__global__ void ksolve_pack_fast_p_g0r4(const ks::FastArgs* a);
__global__ void ksolve_pack_fast_p_g1r4(const ks::FastArgs* a);
__global__ void ksolve_pack_fast_p_g2r4(const ks::FastArgs* a);
__global__ void ksolve_pack_fast2(const ks::FastArgs* a);
__global__ void ksolve_pack_fast_batch(const ks::FastArgs* const* items);
__global__ void ksolve_pack_topo(const ks::TopoArgs* a);
__global__ void ksolve_pack_topo_nodes(const ks::TopoArgs* a);   // ... with existing nodes (topo_nodes.h)
// ... and the two with the set-aside list and the second round of engines 22 / 23 compiled in (ksolve_pack_topo_unsched.hip)
__global__ void ksolve_pack_topo_u(const ks::TopoArgs* a);
__global__ void ksolve_pack_topo_nodes_u(const ks::TopoArgs* a);
// ... and those two with the topology node filters of engines 24 / 25 compiled in as well (ksolve_pack_topo_filter.hip)
__global__ void ksolve_pack_topo_f(const ks::TopoArgs* a);
__global__ void ksolve_pack_topo_nodes_f(const ks::TopoArgs* a);
// ... and those two with the pod operators of engines 29 / 30 compiled in as well (ksolve_pack_topo_podops.hip)
__global__ void ksolve_pack_topo_p(const ks::TopoArgs* a);
__global__ void ksolve_pack_topo_nodes_p(const ks::TopoArgs* a);
// ... and the six once more, many problems per launch (ksolve_solve_many; topo_many.h: block = one ticket = one member, largest first;
// ksolve_pack_topo_many.hip, ksolve_pack_topo_many_unsched.hip, ksolve_pack_topo_many_filter.hip)
__global__ void ksolve_pack_topo_many(const ks::TopoArgs* const* items, const uint32_t* order, uint32_t* next, int n);
__global__ void ksolve_pack_topo_nodes_many(const ks::TopoArgs* const* items, const uint32_t* order, uint32_t* next, int n);
__global__ void ksolve_pack_topo_many_u(const ks::TopoArgs* const* items, const uint32_t* order, uint32_t* next, int n);
__global__ void ksolve_pack_topo_nodes_many_u(const ks::TopoArgs* const* items, const uint32_t* order, uint32_t* next, int n);
__global__ void ksolve_pack_topo_many_f(const ks::TopoArgs* const* items, const uint32_t* order, uint32_t* next, int n);
__global__ void ksolve_pack_topo_nodes_many_f(const ks::TopoArgs* const* items, const uint32_t* order, uint32_t* next, int n);
// the cursor engine's existing-node stage (node_stage.h), `remaining` in LDS / in the HBM workspace
__global__ void ksolve_pack_nodes_lds(const ks::FastArgs* a);
__global__ void ksolve_pack_nodes_hbm(const ks::FastArgs* a);
#ifdef KSOLVE_TEST_HOOKS
// test builds only: FastCold alone, per instantiation (ksolve_test_fast_cold.hip, fast_cold_probe.h)
namespace ks { struct FastColdArgs; }
__global__ void ksolve_test_fast_cold_g0r1(const ks::FastColdArgs* a);
__global__ void ksolve_test_fast_cold_g0r4(const ks::FastColdArgs* a);
__global__ void ksolve_test_fast_cold_u_g0r1(const ks::FastColdArgs* a);
__global__ void ksolve_test_fast_cold_u_g0r4(const ks::FastColdArgs* a);
__global__ void ksolve_test_fast_cold_p_g0r1(const ks::FastColdArgs* a);
__global__ void ksolve_test_fast_cold_p_g0r4(const ks::FastColdArgs* a);
__global__ void ksolve_test_fast_cold_g1r1(const ks::FastColdArgs* a);
__global__ void ksolve_test_fast_cold_u_g2r4(const ks::FastColdArgs* a);
#endif
