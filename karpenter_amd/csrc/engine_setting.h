// engine_setting.h — ksolve_options.engine decoded ONCE: a table with a row per public value (and a second one for the values from 29
// on, below), and the policy a row stands for.
// Host-only plain C++, no device code: ksolve_impl.h looks a handle's value up in create() and reads the policy from then on
// (ksolve_handle::eng; the options keep what the caller passed); the host library (host/ksched.cpp) looks the option's NAME up in the
// same table. include/ksolve.h documents the values for callers; a new value is a new row here and a new line there.
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
  const char* name;     // options.engine of the host library's problem document; nullptr = no name
  bool spread_pod_operators = false;   // the spread engine takes such pod classes too, and node-filter terms of those operators (topo_engine.h, "The spread engine's pod operators"); behind
                                       // `name`, so that the rows of the first table stay as they are written

  constexpr bool general_only() const { return run == General; }
  constexpr bool cursor_only() const { return run == Cursor; }
  constexpr bool spread_only() const { return run == Spread; }
  constexpr bool refuses() const { return run == Cursor || run == Spread; }    // a decline is an error, not a fallback
  constexpr bool may_spread() const { return run == Auto || run == Spread; }   // (a cursor-only handle never tries the spread engine)
};

//                                              run                    plan pick   pair   nodes  s-nodes limits s-lim  ops    s-ops  unsched s-uns  s-filt p-ops  name
inline constexpr EnginePolicy kEngineSettings[] = {
  /*  0 */ {EnginePolicy::Auto,    0, true,  false, false, false, false, false, false, false, false, false, false, false, "auto"},
  /*  1 */ {EnginePolicy::General, 0, false, false, false, false, false, false, false, false, false, false, false, false, "general"},
  /*  2 */ {EnginePolicy::Cursor,  0, true,  false, false, false, false, false, false, false, false, false, false, false, "cursor"},
  /*  3 */ {EnginePolicy::Cursor,  1, false, false, false, false, false, false, false, false, false, false, false, false, "cursor-wide"},
  /*  4 */ {EnginePolicy::Cursor,  2, false, false, false, false, false, false, false, false, false, false, false, false, "cursor-hbm"},
  /*  5 */ {EnginePolicy::Cursor,  0, false, true,  false, false, false, false, false, false, false, false, false, false, "cursor-pair"},
  /*  6 */ {EnginePolicy::Spread,  0, false, false, false, false, false, false, false, false, false, false, false, false, "spread"},
  /*  7 */ {EnginePolicy::Auto,    0, true,  false, true,  false, false, false, false, false, false, false, false, false, "auto-nodes"},
  /*  8 */ {EnginePolicy::Cursor,  0, true,  false, true,  false, false, false, false, false, false, false, false, false, "cursor-nodes"},
  /*  9 */ {EnginePolicy::Auto,    0, true,  false, true,  true,  false, false, false, false, false, false, false, false, "auto-nodes-spread"},
  /* 10 */ {EnginePolicy::Spread,  0, false, false, false, true,  false, false, false, false, false, false, false, false, "spread-nodes"},
  /* 11 */ {EnginePolicy::Auto,    0, true,  false, true,  false, true,  false, false, false, false, false, false, false, "auto-limits"},
  /* 12 */ {EnginePolicy::Cursor,  0, true,  false, true,  false, true,  false, false, false, false, false, false, false, "cursor-limits"},
  /* 13 */ {EnginePolicy::Auto,    0, true,  false, true,  true,  true,  true,  false, false, false, false, false, false, "auto-limits-spread"},
  /* 14 */ {EnginePolicy::Spread,  0, false, false, false, true,  false, true,  false, false, false, false, false, false, "spread-limits"},
  /* 15 */ {EnginePolicy::Auto,    0, true,  false, true,  true,  true,  true,  true,  false, false, false, false, false, "auto-operators"},
  /* 16 */ {EnginePolicy::Cursor,  0, true,  false, true,  false, true,  false, true,  false, false, false, false, false, "cursor-operators"},
  /* 17 */ {EnginePolicy::Cursor,  0, false, false, false, false, false, false, false, false, false, false, false, false, nullptr},   // no name: what a value past the table stands for (below), kept as it was
  /* 18 */ {EnginePolicy::Auto,    0, true,  false, true,  true,  true,  true,  true,  true,  false, false, false, false, "auto-operators-spread"},
  /* 19 */ {EnginePolicy::Spread,  0, false, false, false, true,  false, true,  false, true,  false, false, false, false, "spread-operators"},
  /* 20 */ {EnginePolicy::Auto,    0, true,  false, true,  true,  true,  true,  true,  true,  true,  false, false, false, "auto-unschedulable"},
  /* 21 */ {EnginePolicy::Cursor,  0, true,  false, true,  false, true,  false, true,  false, true,  false, false, false, "cursor-unschedulable"},
  /* 22 */ {EnginePolicy::Auto,    0, true,  false, true,  true,  true,  true,  true,  true,  true,  true,  false, false, "auto-unschedulable-spread"},
  /* 23 */ {EnginePolicy::Spread,  0, false, false, false, true,  false, true,  false, true,  false, true,  false, false, "spread-unschedulable"},
  /* 24 */ {EnginePolicy::Auto,    0, true,  false, true,  true,  true,  true,  true,  true,  true,  true,  true,  false, "auto-filters-spread"},
  /* 25 */ {EnginePolicy::Spread,  0, false, false, false, true,  false, true,  false, true,  false, true,  true,  false, "spread-filters"},
  /* 26 */ {EnginePolicy::Auto,    0, true,  false, true,  true,  true,  true,  true,  true,  true,  true,  true,  true,  "auto-pod-operators"},
  /* 27 */ {EnginePolicy::Cursor,  0, true,  false, true,  false, true,  false, true,  false, true,  false, false, true,  "cursor-pod-operators"},
};
inline constexpr uint32_t kEngineSettingCount = (uint32_t)(sizeof(kEngineSettings) / sizeof(kEngineSettings[0]));
// A value past the table is not an error (yet): the cursor engine only, on the LDS plan as it stands, no switch.
inline constexpr EnginePolicy kEngineSettingPastTable = {EnginePolicy::Cursor, 0, false, false, false, false, false, false, false, false, false, false, false, false, nullptr};

// The second table: the rows added since the first one was pinned with its length (28 rows; value 28 is "past the table" for every
// caller that passed it, as 17 was before it, and stays that). Its first row is value kEngineSettingsMoreFirst; a value behind its
// last row is past the table again.
inline constexpr uint32_t kEngineSettingsMoreFirst = 29;
inline constexpr EnginePolicy kEngineSettingsMore[] = {
  /* 29 */ {EnginePolicy::Auto,    0, true,  false, true,  true,  true,  true,  true,  true,  true,  true,  true,  true,  "auto-pod-operators-spread", true},   // 26 + the spread engine's pod operators
  /* 30 */ {EnginePolicy::Spread,  0, false, false, false, true,  false, true,  false, true,  false, true,  true,  false, "spread-pod-operators", true},        // 25 + the same
};
inline constexpr uint32_t kEngineSettingMoreCount = (uint32_t)(sizeof(kEngineSettingsMore) / sizeof(kEngineSettingsMore[0]));

inline const EnginePolicy& engine_policy(uint32_t value) {
  if (value < kEngineSettingCount) return kEngineSettings[value];
  if (value >= kEngineSettingsMoreFirst && value - kEngineSettingsMoreFirst < kEngineSettingMoreCount) return kEngineSettingsMore[value - kEngineSettingsMoreFirst];
  return kEngineSettingPastTable;
}

// The value an option name stands for; 0 ("auto") for a name neither table holds. (A row without a name has none to match.)
inline uint32_t engine_value(const char* name) {
  for (uint32_t v = 0; v < kEngineSettingCount; ++v) if (kEngineSettings[v].name && !strcmp(kEngineSettings[v].name, name)) return v;
  for (uint32_t v = 0; v < kEngineSettingMoreCount; ++v) if (kEngineSettingsMore[v].name && !strcmp(kEngineSettingsMore[v].name, name)) return kEngineSettingsMoreFirst + v;
  return 0;
}

}  // namespace ksi
