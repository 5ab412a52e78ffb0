// engine_setting.h — ksolve_options.engine decoded ONCE: a table with a row per public value, and the policy a row stands for.
// Host-only plain C++, no device code: ksolve_impl.h looks a handle's value up in create() and reads the policy from then on
// (ksolve_handle::eng; the options keep what the caller passed); the host library (host/ksched.cpp) looks the option's NAME up in the
// same table. include/ksolve.h documents the values for callers; a new value is a new row here and a new line there.
// The table has kEngineTableRows rows. kEngineSettingCount keeps its value and its meaning, "rows 0-33": what the table held before
// 35 / 36 were added (callers and tests compiled against that number stay right); 34 is a hole like 17, 28 and 31, and the lookups
// below walk the longer table.
#pragma once
#include <cstdint>
#include <cstring>

namespace ksi {

struct EnginePolicy {
  enum Run : uint8_t {
    Auto,      // the fast engine whose shape the problem has, the general engine otherwise or whenever a fast engine declines (a fallback, with a reason)
    General,   // the general engine only
    Cursor,    // the cursor engine only: a problem it cannot take, or declines, is KSOLVE_ERR_UNSUPPORTED
    Spread     // the spread engine only, likewise
  };
  Run run;
  uint8_t first_plan;   // the cursor engine's memory plan a handle starts on (fast_plan_set): 0 = LDS, 1 = the claims' state in HBM, 2 = their order too
  bool pick_plan;       // ... unless the problem's size says that a later plan is needed anyway (create(), "Which plan will hold ...")
  bool pair;            // the two-wavefront kernel of the LDS plan (ksolve_pack_fast2; measurements only)
  bool nodes;           // the cursor engine may take a problem with existing nodes (node_stage.h)
  bool spread_nodes;    // the spread engine may (topo_nodes.h)
  bool limits;          // the cursor engine goes on when a NodePool limit binds (fast_engine.h FastLimits)
  bool spread_limits;   // the spread engine does (topo_engine.h limit_stage)
  bool operators;       // the cursor engine takes NodePools whose requirements are not In sets (fast_engine.h, "Complement templates")
  bool spread_operators; // the spread engine does (topo_engine.h, "Complement templates on the spread engine")
  bool unschedulable;   // the cursor engine keeps a pod that can go nowhere and reports its error (fast_engine.h, "Unschedulable pods")
  bool spread_unschedulable; // the spread engine does, and retries such pods for real (topo_engine.h, "The spread engine's unschedulable pods")
  bool spread_filters;  // the spread engine counts pods through topology node filters that can say no (topo_engine.h, "Topology node filters")
  bool pod_operators;   // the cursor engine takes pod classes with NotIn, Exists and DoesNotExist requirements (fast_engine.h, "The cursor engine's pod operators")
  bool spread_pod_operators; // the spread engine takes such pod classes too, and node-filter terms of those operators (topo_engine.h, "The spread engine's pod operators")
  bool node_pod_operators;   // the cursor engine's existing-node stage takes such pod classes too (node_stage.h, "Pod operators beside existing nodes")
  bool spread_node_pod_operators; // the spread engine's existing-node path takes such pod classes too (topo_nodes.h, "Pod operators beside existing nodes on the spread engine")
  const char* name;     // options.engine of the host library's problem document; nullptr = no name

  constexpr bool general_only() const { return run == General; }
  constexpr bool cursor_only() const { return run == Cursor; }
  constexpr bool spread_only() const { return run == Spread; }
  constexpr bool refuses() const { return run == Cursor || run == Spread; }    // a decline is an error, not a fallback
  constexpr bool may_spread() const { return run == Auto || run == Spread; }   // (a cursor-only handle never tries the spread engine)
};

// A row is a run kind on a first plan, or the row it extends plus the switches it adds.
constexpr EnginePolicy engine_row(EnginePolicy::Run run, uint8_t first_plan, bool pick_plan, const char* name) {
  EnginePolicy p{};
  p.run = run; p.first_plan = first_plan; p.pick_plan = pick_plan; p.name = name;
  return p;
}
template <class... Switch>
constexpr EnginePolicy engine_row(EnginePolicy from, const char* name, Switch... adds) {
  from.name = name;
  ((from.*adds = true), ...);
  return from;
}
// A value without a row is not an error (yet): the cursor engine only, on the LDS plan as it stands, no switch, no name. 17, 28, 31 and 34
// were such values for every caller that passed them when the rows behind them were added, and stay that.
inline constexpr EnginePolicy kEngineSettingPastTable = engine_row(EnginePolicy::Cursor, 0, false, nullptr);
inline constexpr uint32_t kEngineSettingCount = 34;   // rows 0-33 (kept: see the head of this file)
inline constexpr uint32_t kEngineTableRows = 37;      // rows 0-36: what the table holds
struct EngineTable { EnginePolicy row[kEngineTableRows]; };
constexpr EngineTable engine_table() {
  using P = EnginePolicy;
  EngineTable t{};
  EnginePolicy* r = t.row;
  r[0] = engine_row(P::Auto, 0, true, "auto");
  r[1] = engine_row(P::General, 0, false, "general");
  r[2] = engine_row(P::Cursor, 0, true, "cursor");
  r[3] = engine_row(P::Cursor, 1, false, "cursor-wide");
  r[4] = engine_row(P::Cursor, 2, false, "cursor-hbm");
  r[5] = engine_row(engine_row(P::Cursor, 0, false, nullptr), "cursor-pair", &P::pair);
  r[6] = engine_row(P::Spread, 0, false, "spread");
  r[7] = engine_row(r[0], "auto-nodes", &P::nodes);
  r[8] = engine_row(r[2], "cursor-nodes", &P::nodes);
  r[9] = engine_row(r[7], "auto-nodes-spread", &P::spread_nodes);
  r[10] = engine_row(r[6], "spread-nodes", &P::spread_nodes);
  r[11] = engine_row(r[7], "auto-limits", &P::limits);
  r[12] = engine_row(r[8], "cursor-limits", &P::limits);
  r[13] = engine_row(r[9], "auto-limits-spread", &P::limits, &P::spread_limits);
  r[14] = engine_row(r[10], "spread-limits", &P::spread_limits);
  r[15] = engine_row(r[13], "auto-operators", &P::operators);
  r[16] = engine_row(r[12], "cursor-operators", &P::operators);
  r[17] = kEngineSettingPastTable;
  r[18] = engine_row(r[15], "auto-operators-spread", &P::spread_operators);
  r[19] = engine_row(r[14], "spread-operators", &P::spread_operators);
  r[20] = engine_row(r[18], "auto-unschedulable", &P::unschedulable);
  r[21] = engine_row(r[16], "cursor-unschedulable", &P::unschedulable);
  r[22] = engine_row(r[20], "auto-unschedulable-spread", &P::spread_unschedulable);
  r[23] = engine_row(r[19], "spread-unschedulable", &P::spread_unschedulable);
  r[24] = engine_row(r[22], "auto-filters-spread", &P::spread_filters);
  r[25] = engine_row(r[23], "spread-filters", &P::spread_filters);
  r[26] = engine_row(r[24], "auto-pod-operators", &P::pod_operators);
  r[27] = engine_row(r[21], "cursor-pod-operators", &P::pod_operators);
  r[28] = kEngineSettingPastTable;
  r[29] = engine_row(r[26], "auto-pod-operators-spread", &P::spread_pod_operators);
  r[30] = engine_row(r[25], "spread-pod-operators", &P::spread_pod_operators);
  r[31] = kEngineSettingPastTable;
  r[32] = engine_row(r[29], "auto-pod-operators-nodes", &P::node_pod_operators);
  r[33] = engine_row(r[27], "cursor-pod-operators-nodes", &P::node_pod_operators);
  r[34] = kEngineSettingPastTable;
  r[35] = engine_row(r[32], "auto-pod-operators-spread-nodes", &P::spread_node_pod_operators);
  r[36] = engine_row(r[30], "spread-pod-operators-nodes", &P::spread_node_pod_operators);
  return t;
}
inline constexpr EngineTable kEngineSettings = engine_table();

inline const EnginePolicy& engine_policy(uint32_t value) { return value < kEngineTableRows ? kEngineSettings.row[value] : kEngineSettingPastTable; }

// The value an option name stands for; 0 ("auto") for a name the table does not hold. (A row without a name has none to match.)
inline uint32_t engine_value(const char* name) {
  for (uint32_t v = 0; v < kEngineTableRows; ++v) if (kEngineSettings.row[v].name && !strcmp(kEngineSettings.row[v].name, name)) return v;
  return 0;
}

}  // namespace ksi
