// decline.h — why a fast engine (cursor: fast_engine.h, node_stage.h; spread: topo_engine.h, topo_nodes.h) handed a problem to the
// general engine: the values of ksolve_results::engine_fallback_reason. The numbers are public output and do not change; DESIGN.md
// ("Decline reasons") has the table with who raises each and what the handle does afterwards. Device and host code.
#pragma once

namespace ks {

enum Decline : int {
  DECLINE_KERNEL_CAPACITY = -1,        // inside a kernel only: more claims than Workspace::max_claims — the kernel ends with status 1, not 3, and the host reports DECLINE_CAPACITY
  DECLINE_NONE = 0,                    // the fast engine solved the problem
  // FastCold::setup(), for both engines
  DECLINE_NOT_PLAIN = 1,               // outside the view's plain / plain_topo / plain_nodes (/ plain_ops under engines 15 / 16), relaxation rows, more than 4 resources, 32 templates or kMaxItWords
                                       // words of types; the host raises it for a batch that Gt / Lt NodePools alone keep from the cursor engine (ksolve_impl.h, plain_ops),
                                       // and under engines 18 / 19 for a topology batch outside plain_topo (pod-side bounds, minValues, ...)
  DECLINE_TEMPLATE_NOT_POSITIVE = 3,   // a NodePool requirement that is not an In set (NotIn, Exists, DoesNotExist; Gt, Lt on the spread engine) — not the cursor engine under engines 15 / 16, not the spread engine under 18 / 19
  DECLINE_CLASS_NOT_POSITIVE = 4,      // a pod requirement that is not an In set (requirements.go:260-265 would apply) — not the cursor engine under engines 26 / 27, which take NotIn, Exists and
                                       // DoesNotExist on pods (fast_engine.h, "The cursor engine's pod operators"), not the spread engine under 29 / 30 (topo_engine.h, "The spread engine's
                                       // pod operators") — but for a batch with existing nodes: the cursor engine's existing-node stage raises it under every setting but engines 32 / 33
                                       // (node_stage.h, "Pod operators beside existing nodes"); the spread engine with nodes under every setting but engines 35 / 36
                                       // (topo_nodes.h, "Pod operators beside existing nodes on the spread engine")
  DECLINE_SELECTS_HOST_OR_TYPE = 5,    // pods (or a dictionary-key group) select on kubernetes.io/hostname or the instance type
  DECLINE_KEYS_DO_NOT_PACK = 6,        // the keys pods select on: more than kFastMaxVar, wider than one word, or beyond kFastVarBits bits
  DECLINE_QUANTITY_RANGE = 7,          // an allocatable, effective allocatable or request outside 31 bits
  DECLINE_CLASS_EMPTY_IN = 8,          // a pod requirement In [] (== DoesNotExist: not positive) — as 4: not the cursor engine under engines 26 / 27, not the spread engine under 29 / 30; with existing nodes
                                       // the cursor engine's stage raises it under every setting but 32 / 33, the spread engine under every setting but 35 / 36
  // engines 26 / 27 and 29 / 30 only: what the pod operators leave to the general engine (fast_engine.h, "The cursor engine's pod operators"; under topology a group's key counts as an In user for 9)
  DECLINE_CLASS_KEY_DEFINEDNESS = 9,   // a custom key some NodePool leaves undefined, with a NotIn / DoesNotExist class and an In / Exists class on it: whether the second kind is
                                       // admissible depends on whether a pod of the first kind joined the claim before (requirements.go:185-193)
  DECLINE_CLASS_DNE_MIXED = 10,        // a key with a DoesNotExist class and a NotIn class or a NotIn NodePool: the packed set "no dictionary value left" would stand for both
  DECLINE_CLASS_NOTIN_BOUNDS = 11,     // a pod's NotIn on a key where a NodePool carries Gt / Lt: the claim would print the pod's values outside the bounds
  DECLINE_CLASS_EXISTS_UNDEFINED = 12, // a pod's Exists on a well-known key some NodePool leaves undefined: the claim would print Exists
  // the cursor engine's loop
  DECLINE_CACHE_FULL = 20,             // no room for a requirement set's cache entry or Pareto vectors (a claim's acceptance words, a new class slot)
  DECLINE_REFRESH_FAILED = 21,         // the same while the driver recomputed a claim's acceptance words
  DECLINE_UNKNOWN_EVENT = 22,          // the loop returned an event the driver does not know
  DECLINE_LIMIT_NODES = 23,            // a NodePool's `nodes` limit is used up (filterByRemainingResources, scheduler.go:1069-1085); both engines — not under the settings with limit stages (cursor: 11-13, spread: 13 / 14)
  DECLINE_LIMIT_EXCLUDES_TYPE = 24,    // a NodePool limit excludes an instance type of the template (scheduler.go:1069-1085); both engines, as 23
  DECLINE_CACHE_FULL_NEW_CLAIM = 25,   // no room for the cache entry of a new claim's requirement set (addToNewNodeClaim, scheduler.go:695-790); both engines
  DECLINE_CLAIM_SLOTS = 26,            // more in-flight claims than the cursor engine's memory plan holds: the host moves to the next plan
  DECLINE_UNSCHEDULABLE_POD = 27,      // a pod no claim and no template takes: error codes and diagnostics are the general engine's; both engines — the cursor engine not under engines 20 / 21, which set the pod aside with its error (there only the retry's safety net names 27), the spread engine not under 22 / 23, which set it aside and retry it for real
  DECLINE_REFRESHER_DEAD = 28,         // two-wavefront kernel: the refresher wavefront does not answer
  DECLINE_LIMIT_STAGES = 29,           // engines 11-14, both engines: NodePool limits narrowed the templates' type lists more often than there are free template ids (limit stages)
  // existing nodes, decided by create() (cursor: engines 7 / 8, spread: engines 9 / 10)
  DECLINE_NODE_CONSOLIDATE_AFTER = 30, // a node under consolidateAfter that some pod must skip (scheduler.go:628)
  DECLINE_NODE_BOUNDS = 31,            // node requirement sets with Gt / Lt bounds
  DECLINE_NODE_LABELS = 32,            // a node label set that is not single-valued In (existingnode.go:172-185 would change it)
  DECLINE_NODE_CLASSES = 33,           // more pod classes than the node stage keeps cursors for (kNodeStageMaxClasses); decided by solve()
  DECLINE_NODES_NOT_PLAIN = 34,        // existing nodes, and otherwise outside the engine's shape (host ports, volumes, minValues, reservations, resident pods ...)
  DECLINE_NODE_LACKS_KEY = 35,         // spread: a node without a label for a dictionary key some topology group uses
  DECLINE_NODE_DOMAIN_RANGE = 36,      // spread: a node whose value of such a key lies beyond the kTopoMaxDom domains a group's counters hold (engines 35 / 36, a batch under the phantom layout: beyond the fifteen it leaves)
  DECLINE_NODE_KEY_DEFINEDNESS = 37,   // engines 32 / 33, the cursor engine's existing-node stage: a key some node lacks, with a NotIn class and an In / Exists class on it — a NotIn pod
                                       // that lands on such a node defines the key there, and the second kind passes from then on (requirements.go:189): the (class, node) rows are not static.
                                       // Engines 35 / 36, the spread engine's node path (topo_nodes.h topo_nodes_definedness): the same, and an In / Exists TERM of a topology node filter on the
                                       // key counts like an In / Exists class (the filter reads the node's pristine label row)
  // TopoEngine::setup_topo()
  DECLINE_TOPO_GROUPS = 40,            // no topology group, more than kTopoMaxGroups, or aliased groups
  DECLINE_TOPO_PREFERENCES = 41,       // a pod with preferences: podDomains = StrictRequirements differs from its requirements (topology.go:230)
  DECLINE_TOPO_RELAXATION_GROUP = 42,  // a group created by a relaxing pod (topology.go:162-194)
  DECLINE_TOPO_NODE_FILTER = 43,       // a group's TopologyNodeFilter can reject a claim or node (topologynodefilter.go:68-96); create() raises it for tainted nodes.
                                       // Engines 24 / 25 evaluate such filters themselves and keep 43 for what their slots do not hold: a term that is not positive In sets on
                                       // packed variable keys, more than kTopoFiltTerms terms, more than kTopoFiltSlots filters decided per claim, a filter on a group that is no spread group.
                                       // Engines 29 / 30 over a batch with negative pods or terms pack NotIn / Exists / DoesNotExist terms too and hold kTopoFiltSlotsPodOps filters; 43 there also for
                                       // an Exists term on a key with a DoesNotExist class or NodePool and a DoesNotExist term on a key with an Exists / Gt / Lt NodePool (the word cannot tell the bins apart)
  DECLINE_TOPO_SKEW_RANGE = 44,        // dictionary-key spread: maxSkew outside 1..30000, or minDomains above 30000
  DECLINE_TOPO_HOST_AFFINITY = 45,     // pod affinity on the hostname
  DECLINE_TOPO_HOST_GROUPS = 46,       // more hostname groups than kTopoMaxHost
  DECLINE_TOPO_HOST_SKEW = 47,         // hostname spread with maxSkew outside 1..6 (the counters saturate at 7)
  DECLINE_TOPO_INVERSE_KIND = 48,      // an inverse group on a dictionary key that is not anti-affinity
  DECLINE_TOPO_KEY_GROUPS = 49,        // more dictionary-key groups than kTopoMaxZg
  DECLINE_TOPO_DOMAINS = 50,           // a group's key is not a packed variable key, or has more than kTopoMaxDom domains (29 / 30 over a batch with negative pods or terms: the phantom bit is one of them — fifteen dictionary values)
  DECLINE_TOPO_CLASS = 51,             // a pod class with a hostname limit outside 0..6 or three dictionary-key groups
  // the spread engine's loop
  DECLINE_TOPO_CACHE_FULL = 60,        // no room for a requirement set's cache entry (resolve)
  DECLINE_TOPO_LIST_BEYOND_RINGS = 61, // a listed claim holds more pods than the LDS ring tables cover (kRunMaxCount)
  DECLINE_TOPO_RUN_BEYOND_RINGS = 62,  // a run at the front of the order lies beyond the LDS ring tables
  // the host
  DECLINE_CAPACITY = 100,              // the kernel ended with status 1: more claims than max_claims — the general engine reports it (or moves to BIG)
};

}  // namespace ks
