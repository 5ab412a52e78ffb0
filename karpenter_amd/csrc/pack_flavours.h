// pack_flavours.h — the flavours of the cursor and the spread engine's pack kernels and the kernel matrix, ONCE. Every opt-in switch
// of the fast engines is a compile-time template bool with kernels of its own, so that the kernels every other setting runs keep
// their code; which kernels exist, what each is called and which one a handle launches is written here and nowhere else:
//   the kernel definitions (ksolve_pack_fast.hip, ksolve_pack_topo.hip, ksolve_pack_topo_many.hip, ksolve_test_fast_cold.hip), their
//   declarations (pack_kernels.h), the function-pointer tables of the HIP backend (ksolve.hip), the names the host emulation reports
//   (tests/emu/ksolve_emu.cpp) and the compile jobs of the build are all generated from, or checked against, the lists below.
// Host-only plain C++, no device code (as engine_setting.h). A new flavour is a new enumerator, its rows in the lists, and a compile
// job per unit; tests/test_kernel_table.py holds the lists against a literal table.
#pragma once
#include <cstdint>

namespace ks {

// Each flavour is the one before it plus one switch (the static_asserts of FastEngine / TopoEngine say so).
enum class FastFlavour : int { Plain = 0, Unsched = 1, PodOps = 2 };               // + the set-aside list (engines 20 / 21); + pod operators (26 / 27)
enum class TopoFlavour : int { Plain = 0, Unsched = 1, Filter = 2, PodOps = 3 };   // + set-aside list and second round (22 / 23); + topology node filters (24 / 25); + pod operators (29 / 30)
constexpr int kFastFlavours = 3, kTopoFlavours = 4;
// the template bools of a flavour: FastEngine's / FastCold's US, PO and TopoEngine's US, FS, PO
constexpr bool flavour_us(FastFlavour f) { return f >= FastFlavour::Unsched; }
constexpr bool flavour_po(FastFlavour f) { return f >= FastFlavour::PodOps; }
constexpr bool flavour_us(TopoFlavour f) { return f >= TopoFlavour::Unsched; }
constexpr bool flavour_fs(TopoFlavour f) { return f >= TopoFlavour::Filter; }
constexpr bool flavour_po(TopoFlavour f) { return f >= TopoFlavour::PodOps; }
// The flavour a handle's work record asks for: the only places that read FastWork's switches to choose a kernel. (Templates only so
// that this header stands without fast_engine.h; Work is ks::FastWork.)
template <class Work> inline FastFlavour fast_flavour(const Work& fw) { return fw.podops ? FastFlavour::PodOps : fw.unsched ? FastFlavour::Unsched : FastFlavour::Plain; }
template <class Work> inline TopoFlavour topo_flavour(const Work& fw) { return fw.podops ? TopoFlavour::PodOps : fw.filt ? TopoFlavour::Filter : fw.unsched ? TopoFlavour::Unsched : TopoFlavour::Plain; }

}  // namespace ks

// ---- the kernel matrix: one X-macro list per family and flavour number, in the order the units define them ----
// the cursor engine, X(kernel, flavour, plan, rows): per memory plan (g: FastPlan::global_state) and rows of class slots (r: 1 or ks::kFastRows)
#define KS_PACK_FAST_ROWS_0(X) \
  X(ksolve_pack_fast_g0r1, Plain, 0, 1) X(ksolve_pack_fast_g1r1, Plain, 1, 1) X(ksolve_pack_fast_g2r1, Plain, 2, 1) \
  X(ksolve_pack_fast_g0r4, Plain, 0, 4) X(ksolve_pack_fast_g1r4, Plain, 1, 4) X(ksolve_pack_fast_g2r4, Plain, 2, 4)
#define KS_PACK_FAST_ROWS_1(X) \
  X(ksolve_pack_fast_u_g0r1, Unsched, 0, 1) X(ksolve_pack_fast_u_g1r1, Unsched, 1, 1) X(ksolve_pack_fast_u_g2r1, Unsched, 2, 1) \
  X(ksolve_pack_fast_u_g0r4, Unsched, 0, 4) X(ksolve_pack_fast_u_g1r4, Unsched, 1, 4) X(ksolve_pack_fast_u_g2r4, Unsched, 2, 4)
#define KS_PACK_FAST_ROWS_2(X) \
  X(ksolve_pack_fast_p_g0r1, PodOps, 0, 1) X(ksolve_pack_fast_p_g1r1, PodOps, 1, 1) X(ksolve_pack_fast_p_g2r1, PodOps, 2, 1) \
  X(ksolve_pack_fast_p_g0r4, PodOps, 0, 4) X(ksolve_pack_fast_p_g1r4, PodOps, 1, 4) X(ksolve_pack_fast_p_g2r4, PodOps, 2, 4)
#define KS_PACK_FAST_ROWS(X) KS_PACK_FAST_ROWS_0(X) KS_PACK_FAST_ROWS_1(X) KS_PACK_FAST_ROWS_2(X)
// the spread engine, X(kernel, flavour, nodes): without / with existing nodes (topo_nodes.h)
#define KS_PACK_TOPO_ROWS_0(X) X(ksolve_pack_topo, Plain, 0) X(ksolve_pack_topo_nodes, Plain, 1)
#define KS_PACK_TOPO_ROWS_1(X) X(ksolve_pack_topo_u, Unsched, 0) X(ksolve_pack_topo_nodes_u, Unsched, 1)
#define KS_PACK_TOPO_ROWS_2(X) X(ksolve_pack_topo_f, Filter, 0) X(ksolve_pack_topo_nodes_f, Filter, 1)
#define KS_PACK_TOPO_ROWS_3(X) X(ksolve_pack_topo_p, PodOps, 0) X(ksolve_pack_topo_nodes_p, PodOps, 1)
#define KS_PACK_TOPO_ROWS(X) KS_PACK_TOPO_ROWS_0(X) KS_PACK_TOPO_ROWS_1(X) KS_PACK_TOPO_ROWS_2(X) KS_PACK_TOPO_ROWS_3(X)
// ... many problems per launch (ksolve_solve_many; topo_many.h), X(kernel, flavour, nodes). The pod operators have no such form: a
// member of that flavour runs alone.
#define KS_PACK_TOPO_MANY_ROWS_0(X) X(ksolve_pack_topo_many, Plain, 0) X(ksolve_pack_topo_nodes_many, Plain, 1)
#define KS_PACK_TOPO_MANY_ROWS_1(X) X(ksolve_pack_topo_many_u, Unsched, 0) X(ksolve_pack_topo_nodes_many_u, Unsched, 1)
#define KS_PACK_TOPO_MANY_ROWS_2(X) X(ksolve_pack_topo_many_f, Filter, 0) X(ksolve_pack_topo_nodes_many_f, Filter, 1)
#define KS_PACK_TOPO_MANY_ROWS(X) KS_PACK_TOPO_MANY_ROWS_0(X) KS_PACK_TOPO_MANY_ROWS_1(X) KS_PACK_TOPO_MANY_ROWS_2(X)
// test builds only: FastCold alone (fast_cold_probe.h), X(kernel, flavour, plan, rows) — one unit, every flavour
#define KS_FAST_COLD_ROWS(X) \
  X(ksolve_test_fast_cold_g0r1, Plain, 0, 1) X(ksolve_test_fast_cold_g0r4, Plain, 0, 4) \
  X(ksolve_test_fast_cold_u_g0r1, Unsched, 0, 1) X(ksolve_test_fast_cold_u_g0r4, Unsched, 0, 4) \
  X(ksolve_test_fast_cold_p_g0r1, PodOps, 0, 1) X(ksolve_test_fast_cold_p_g0r4, PodOps, 0, 4) \
  X(ksolve_test_fast_cold_g1r1, Plain, 1, 1) X(ksolve_test_fast_cold_u_g2r4, Unsched, 2, 4)
#define KS_CAT_(a, b) a##b
#define KS_CAT(a, b) KS_CAT_(a, b)   // KS_CAT(KS_PACK_FAST_ROWS_, KS_PACK_FLAVOUR): the rows a unit compiled with -DKS_PACK_FLAVOUR=<n> defines

namespace ks {

struct PackFastRow { const char* kernel; FastFlavour flavour; int plan, rows; };
struct PackTopoRow { const char* kernel; TopoFlavour flavour; bool nodes; };
#define KS_ROW_FAST(NAME, FL, GS, R) {#NAME, FastFlavour::FL, GS, R},
#define KS_ROW_TOPO(NAME, FL, ND) {#NAME, TopoFlavour::FL, ND != 0},
inline constexpr PackFastRow kPackFastRows[] = {KS_PACK_FAST_ROWS(KS_ROW_FAST)};
inline constexpr PackTopoRow kPackTopoRows[] = {KS_PACK_TOPO_ROWS(KS_ROW_TOPO)};
inline constexpr PackTopoRow kPackTopoManyRows[] = {KS_PACK_TOPO_MANY_ROWS(KS_ROW_TOPO)};
inline constexpr PackFastRow kFastColdRows[] = {KS_FAST_COLD_ROWS(KS_ROW_FAST)};
#undef KS_ROW_FAST
#undef KS_ROW_TOPO
// the many-problem kernels there are: solve_many groups its spread members by the index of their row
constexpr int kTopoManyFlavours = (int)(sizeof(kPackTopoManyRows) / sizeof(kPackTopoManyRows[0]));
// the cursor engine's kernels outside the matrix: the two-wavefront kernel of the LDS plan, the batched form (both of the plain
// flavour only) and the existing-node stage in front of the loop (node_stage.h; `remaining` in LDS / in the HBM workspace; _p: with
// the stage's pod operators, engines 32 / 33 — a bool of the stage's own, not a FastFlavour: the loop behind it is the PodOps flavour's)
inline constexpr char kPackFastPair[] = "ksolve_pack_fast2", kPackFastBatch[] = "ksolve_pack_fast_batch";
inline constexpr char kPackNodesLds[] = "ksolve_pack_nodes_lds", kPackNodesHbm[] = "ksolve_pack_nodes_hbm";
inline constexpr char kPackNodesLdsPodOps[] = "ksolve_pack_nodes_lds_p", kPackNodesHbmPodOps[] = "ksolve_pack_nodes_hbm_p";
inline const char* pack_nodes_kernel(bool hbm, bool pod_ops) { return pod_ops ? (hbm ? kPackNodesHbmPodOps : kPackNodesLdsPodOps) : (hbm ? kPackNodesHbm : kPackNodesLds); }
// the spread engine's kernel outside the matrix: the PodOps flavour with existing nodes and the pod operators kept on beside them
// (engines 35 / 36, TopoEngine's NP; ksolve_pack_topo_nodes_pn.hip) — a bool of the node path's own, not a TopoFlavour. pn: the setting
// has the switch, the handle carries the pod operators, and its problem has nodes and a negative class or node-filter term
// (ksolve_impl.h spread_nodes_pn); every other handle with nodes runs the row of its flavour.
inline constexpr char kPackTopoNodesPodOpsNodes[] = "ksolve_pack_topo_nodes_pn";   // (looked up by pack_topo_nodes_kernel, below)

// The row of the kernel both backends launch; nullptr where no kernel exists.
template <class Row, int N, class F> inline const Row* pack_row_where(const Row (&rows)[N], F match) {
  for (const Row& r : rows) if (match(r)) return &r;
  return nullptr;
}
inline const PackFastRow* pack_fast_row(FastFlavour f, int plan, int rows) { return pack_row_where(kPackFastRows, [&](const PackFastRow& r) { return r.flavour == f && r.plan == plan && r.rows == rows; }); }
inline const PackFastRow* fast_cold_row(FastFlavour f, int plan, int rows) { return pack_row_where(kFastColdRows, [&](const PackFastRow& r) { return r.flavour == f && r.plan == plan && r.rows == rows; }); }
inline const PackTopoRow* pack_topo_row(TopoFlavour f, bool nodes) { return pack_row_where(kPackTopoRows, [&](const PackTopoRow& r) { return r.flavour == f && r.nodes == nodes; }); }
inline const char* pack_topo_nodes_kernel(TopoFlavour f, bool pn) { return pn && f == TopoFlavour::PodOps ? kPackTopoNodesPodOpsNodes : pack_topo_row(f, true)->kernel; }
inline const PackTopoRow* pack_topo_many_row(TopoFlavour f, bool nodes) { return pack_row_where(kPackTopoManyRows, [&](const PackTopoRow& r) { return r.flavour == f && r.nodes == nodes; }); }

}  // namespace ks
