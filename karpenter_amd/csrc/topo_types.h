// topo_types.h — what the host side (ksolve_impl.h: buffers, LDS plan, kernel arguments) shares with the spread engine
// (topo_engine.h, compiled into ksolve_pack_topo.hip, ksolve_pack_topo_many.hip and the test emulation only).
#pragma once
#include "fast_engine.h"
#include "run_order.h"

namespace ks {

constexpr int kTopoMaxGroups = 128;   // topology groups of a problem this engine takes
constexpr int kTopoMaxHost = 16;      // of them on kubernetes.io/hostname (regular + inverse): one 4-bit field each
constexpr int kTopoMaxZg = 64;        // ... and on dictionary keys
constexpr int kTopoMaxDom = 16;       // domains of such a key
constexpr int kTopoTrack = 4;         // anti-affinity counters with a list of the claims that hold no member
constexpr int kTopoFreeCap = 1024;    // entries of such a list (more: the list is dropped, its classes scan the order)
constexpr int kTopoFiltSlots = 16;    // topology node filters of a problem that are decided per claim / node (engines 24 / 25); more: DECLINE_TOPO_NODE_FILTER
constexpr int kTopoFiltSlotsPodOps = 32;   // ... of a batch with negative pods or terms under engines 29 / 30: every bit of TopoClass::pad (the handle's TopoFilt is two in a row)
constexpr int kTopoFiltTerms = 4;     // node-affinity terms of such a filter
constexpr uint64_t kTopoGuard = 0x8888888888888888ull, kTopoOnes = 0x1111111111111111ull;

KS_FN uint64_t topo_host_add(uint64_t hcnt, uint64_t hinc) {   // per-field +1, saturating at 7
  const uint64_t full = hcnt & (hcnt >> 1) & (hcnt >> 2) & kTopoOnes;
  return hcnt + (hinc & ~full);
}
struct TopoRec { uint64_t vmask; int32_t req[4]; uint64_t hcnt; };   // 32 B: an in-flight claim (requirement set, requests, hostname-group counters)
// a pod class's topology: limits on the hostname counters it is tested against (field = 8 | limit; 8 | 7 where it has none),
// the counters and dictionary-key groups a pod of the class is counted by, the dictionary-key group it owns
struct TopoClass { uint64_t hlim, hinc, zsel; int16_t zg[2]; uint32_t zself; uint32_t excl; uint32_t pad; };   // 48 B; pad: engines 24 / 25, the filter slots (TopoFilt) of the groups that count the class; zg: up to two dictionary-key groups it is tested against (-1: none), zself bit i: it is selected by zg[i] itself
struct TopoZg {   // a group on a dictionary key (LDS): sixteen counters and name ranks, then one 16-byte header
  int32_t cnt[kTopoMaxDom];
  uint16_t rank[kTopoMaxDom];
  uint32_t dom;        // registered domains (TopologyGroup.domains)
  int32_t nonzero;     // domains with a positive count
  int16_t skew, min_domains;   // maxSkew; minDomains (-1: nil)
  uint8_t type, var, off, width;   // 0 spread / 1 affinity / 2 anti-affinity (also the inverse groups); index of its key among the variable keys (FastMisc::vkey); the key's field inside vmask
};
struct TopoZgHead { uint32_t dom; int32_t nonzero; int16_t skew, min_domains; uint8_t type, var, off, width; };   // TopoZg from `dom` on
static_assert(sizeof(TopoZg) == 112 && sizeof(TopoZgHead) == 16, "TopoZg layout");
struct TopoState {   // LDS
  TopoZg zg[kTopoMaxZg];
  uint32_t freel[kTopoTrack][kTopoFreeCap];
  int32_t n_free[kTopoTrack];
  uint32_t track_field[kTopoTrack];   // hostname counter of list t; 0xFF: none / dropped
  int16_t gmap[kTopoMaxGroups];       // group -> hostname counter (0..15) | 0x100 + dictionary-key group | -1
  // what the loop needs once per block of 64 pods or per new claim, kept out of its scalar registers
  const uint32_t* q_class; uint32_t* q_claim; uint32_t* q_cnt; const TopoClass* tcls; const FastSlot* fcls; uint32_t* hostseq;
  int32_t last[4];                    // the move of the last step: kind (1: a claim gained a pod, 2: a new claim, 0: pending in the order / none), claim, position it left
};
struct TopoPlan { int total_bytes, off_run, off_state; };   // (the cursor engine's tables sit where FastWork::plan says)
// The existing-node path of the spread engine (topo_nodes.h, kernel ksolve_pack_topo_nodes), all in HBM; dom == null: the problem has
// no nodes (or the engine may not take them: engines 0 and 6). Reset by the kernel at the start of every solve.
struct TopoNodes {
  uint64_t* alive;        // [n_classes][node_words] nodes that have not failed the class on a test that only moves towards rejection
  uint32_t* cursor;       // [n_classes] first 64-node block whose alive word is not zero (node_words: none)
  uint64_t* hword;        // [n_nodes] the node's hostname-group counters, laid out like TopoRec::hcnt
  const uint8_t* dom;     // [n_keys][n_nodes] the node's domain on a dictionary key some group uses: the value's bit inside the key's words
  const uint64_t* dead0;  // [n_classes][node_words] the static (class, node) verdicts (ksolve_node_dead0) for this solve's class ids
};
// Engines 24 / 25 (topo_engine.h, "Topology node filters"): a spread group whose TopologyNodeFilter cannot be decided per class at
// set-up. Each node-affinity term is packed like a pod class: fvm = the values it admits per field of the packed requirement word,
// fdm = the fields it selects on. In HBM, written by setup_topo, read on the commits of the classes that carry the slot only.
struct TopoFiltSlot {
  uint64_t fvm[kTopoFiltTerms], fdm[kTopoFiltTerms];
  uint64_t hbit, zbit;    // the group's bit in TopoClass::hinc / zsel (one of them)
  uint32_t tmask;         // templates whose taints the group's owner tolerates (every bit set: nodeTaintsPolicy Ignore)
  uint16_t group;         // the group, for f_tolerates against a node's taints
  uint8_t n_terms;        // 0: nodeAffinityPolicy Ignore, or nothing required
  uint8_t taint;          // nodeTaintsPolicy Honor
};
struct TopoFilt { TopoFiltSlot slot[kTopoFiltSlots]; };
struct TopoFiltCut { uint64_t h, z; };   // the bits of hinc / zsel whose filters say no to one claim or node
struct TopoWork { TopoClass* cls; TopoRec* rec; TopoPlan plan; int enabled; TopoNodes nd; TopoFilt* filt; };   // filt: engines 24 / 25 only, null otherwise
struct TopoArgs { ProblemView pv; Workspace ws; FastWork fw; TopoWork tw; };

}  // namespace ks
