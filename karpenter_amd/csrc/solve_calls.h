// solve_calls.h — ksolve_solve, ksolve_solve_batch and ksolve_solve_many: which engine runs a problem. Host-only; a part of
// ksolve_impl.h (included there, inside namespace ksi, behind everything it calls), compiled by the product library and by the host
// emulation alike. The ladder is: what is refused before any launch -> the spread engine -> the cursor engine, through its memory
// plans -> the general engine -> BIG. Its steps are written ONCE, as plain functions on a handle; the three drivers at the end walk
// them — solve() for one handle with its own launches, solve_batch_plain() with the batch's older and shorter rules (pinned cell by
// cell: tests/golden/engine_matrix*.json), solve_many_plain() as solve() would for every member at once. Where the drivers differ on
// purpose, the step says so ("Many problems per call", has the table).

// What a fast engine's kernel left behind: done = it solved the problem (or was stopped by a step limit / cancel flag) and its results
// stand; otherwise `reason` says why not (decline.h) — the kernel's own for status 3, DECLINE_CAPACITY for status 1, the handle's as
// it was after a device error — and `pops` how far a status-3 run got. The counters are downloaded for status 3 only.
struct FastOutcome { bool done; int status, n_claims; uint32_t reason; unsigned long long pops; };
static FastOutcome fast_outcome(ksolve_handle* h) {
  FastOutcome o{false, 0, 0, h->fast_reason, 0};
  be_d2h(h, &o.status, h->ws.status_out, 4);
  be_d2h(h, &o.n_claims, h->ws.n_claims_out, 4);
  be_sync(h);
  o.done = be_ok(h) && o.status != 3 && o.status != 1;
  if (be_ok(h) && o.status == 3) {
    ks::Counters ctr{};
    be_d2h(h, &ctr, h->ws.counters, sizeof(ctr));
    be_sync(h);
    o.reason = (uint32_t)ctr.decline;
    o.pops = ctr.queue_pops;
  } else if (be_ok(h) && o.status == 1) o.reason = ks::DECLINE_CAPACITY;
  return o;
}

// ---- the steps --------------------------------------------------------------------------------------------------------------------

// What solve() refuses before it launches anything, in its words (KSOLVE_OK: nothing): before solve_prepare ...
static ksolve_status refused_unprepared(ksolve_handle* h) {
  if (h->resident && h->has_topology) return fail(h, KSOLVE_ERR_INVALID, "a resident cluster with topology groups is solved through probes (ksolve_sweep / ksolve_probe_create): its counts include the bound pod rows");
  return KSOLVE_OK;
}
// ... and behind it, when the classes are counted: an engine-only handle outside its engine's shape, and more pod classes than the
// node stage keeps cursors for (under Auto that is the general engine's problem: nothing has run yet). solve() and SolveMany ask;
// SolveBatch never does, which is its recorded behaviour.
static ksolve_status refused_before_launch(ksolve_handle* h) {
  if (h->eng.spread_only() && !(h->tw.enabled && h->n_pods && h->n_classes))
    return h->eng.spread_operators && h->fast_reason ? declined(h, "spread") : outside_shape(h, EnginePolicy::Spread);
  if (h->eng.cursor_only() && !(h->fw.enabled && !h->pv.big && h->n_pods && h->n_classes))
    return h->eng.operators && h->fast_reason ? declined(h, "cursor") : outside_shape(h, EnginePolicy::Cursor);
  if (h->fw.enabled && h->fw.nodes && h->n_classes > (uint32_t)ks::kNodeStageMaxClasses) {
    h->fast_reason = ks::DECLINE_NODE_CLASSES;
    if (h->eng.refuses()) return declined(h, "cursor");
    h->fw.enabled = 0;
  }
  return KSOLVE_OK;
}

// May the batched cursor kernel (ksolve_pack_fast_batch: the LDS plan of ksolve_pack_fast_g0r*, a block per problem) take this handle?
// Not one that solve() would run on another kernel — a plan in HBM (an earlier solve moved it there, or engine = cursor-wide /
// cursor-hbm), the set-aside list (20 / 21: a kernel follows its loop), the pod operators, the two-wavefront kernel — or with kernels
// around the loop (node stage, limit stages): that one runs alone. Pod operators imply the set-aside list (create(): fw.podops only
// beside fw.unsched), so that test decides nothing; it is there for the reader. legacy_batch: SolveBatch leaves the two-wavefront
// test out, and runs a "cursor-pair" handle on the batched kernel (pinned).
static bool batched_cursor_takes(const ksolve_handle* h, bool legacy_batch) {
  const auto& fw = h->fw;
  return fw.plan.global_state == 0 && !fw.nodes && !fw.lim && !fw.unsched && !fw.podops && (legacy_batch || !fw.plan.helper);
}
// SolveBatch has no spread launch of its own. A spread handle runs alone through solve(), so that the batch runs the engine
// ksolve_solve would, if it is a DaemonSet problem, one with existing nodes (9 / 10), one over complement templates (18 / 19) or one
// that keeps unschedulable pods (22 / 23); every other spread-shaped handle runs the general engine with reason 0 (pinned).
static bool spread_takes_alone_in_batch(const ksolve_handle* h) {
  return h->tw.enabled && (h->daemon_groups || h->tw.nd.dom || h->spread_complement || h->fw.unsched) && h->n_classes;
}

// In front of a spread launch: the run-order rings (the first solve uploads them), and with existing nodes (9 / 10) the static
// (class, node) rows for this solve's classes — the kernel resets the nodes' remaining resources, pod counts and counters itself.
static void spread_before_launch(ksolve_handle* h) {
  alloc_run_order(h);
  if (h->tw.nd.dom) { node_static_rows(h); h->tw.nd.dead0 = h->nd_dead0; }
}

// What follows a fast engine's outcome. Done: its results stand (solve_finish next). Refused: an engine-only handle, declined — the
// text is on the handle, the status KSOLVE_ERR_UNSUPPORTED. HandBack: the general engine takes over after a solve_prepare(h, false),
// the reason stays on the handle. NextPlan (cursor): out of claim slots, and a larger memory plan is set.
enum class Settled { Done, Refused, HandBack, NextPlan };

static Settled spread_settle(ksolve_handle* h, const FastOutcome& o) {
  if (o.done) {
    h->engine_used = 3;
    h->fast_reason = 0; h->fast_attempts = 1;
    if (o.n_claims || h->tw.nd.dom) be_launch_fast_records(h, o.n_claims);   // (pods on existing nodes are scattered with the queue's results even when no claim was opened)
    if (h->fw.unsched) be_launch_fast_unsched(h);   // engines 22 / 23: the errors of the pods that ended on the set-aside list (none: nothing is written)
    return Settled::Done;
  }
  h->fast_reason = o.reason;   // status 3 = "not my shape / stopped before any result"
  if (h->eng.spread_only()) { declined(h, "spread"); return Settled::Refused; }
  if (h->fast_reason != ks::DECLINE_UNSCHEDULABLE_POD && h->fast_reason != ks::DECLINE_CAPACITY) h->tw.enabled = 0;   // not its shape: later solves of this handle go straight to the general engine
  return Settled::HandBack;
}

// Out of claim slots (DECLINE_CLAIM_SLOTS, reason 26) is no decline while a larger memory plan is left: the next plan is set (later
// solves of this handle start there) and true returned when it holds more claims. The attempt says how many pods its claims took:
// when the whole queue, at that rate and a quarter more, would not fit plan 1 either, it is plan 2 at once. (Under engines 20 / 21 the
// pops include the pods set aside, which took no claim: the rate is then an underestimate and the choice leans to plan 1; harmless —
// a plan 1 that runs out as well ends with 26 again and moves to plan 2.) plan1_only: SolveBatch's older rule — plan 1 whatever the
// attempt says; solve(), which then runs the handle, escalates further.
static bool next_plan_after_claim_slots(ksolve_handle* h, const FastOutcome& o, bool plan1_only) {
  if (h->fast_reason != ks::DECLINE_CLAIM_SLOTS || h->opts.lds_claim_cap) return false;
  if (plan1_only) { fast_plan_set(h, 1, h->fw.plan.rows); return true; }
  if (!be_ok(h) || h->fw.plan.global_state >= 2) return false;
  const int had = h->fw.plan.cap;
  int next = h->fw.plan.global_state + 1;
  if (next == 1) {
    fast_plan_set(h, 1, h->fw.plan.rows);
    const double placed = (double)(o.pops > 0 ? o.pops : 1);
    const bool holds_all = h->fw.plan.cap >= (int)((h->fast_mc + 63) & ~63u);   // plan 1 has a slot for every claim the problem may open
    if (!holds_all && (double)had * (double)h->n_pods / placed * 1.25 > (double)h->fw.plan.cap) next = 2;
  }
  fast_plan_set(h, next, h->fw.plan.rows);
  return h->fw.plan.cap > had;
}

// (h->fast_attempts, the runs of the cursor engine a solve took, is the drivers': solve() counts its loop, SolveMany counts the
// batched run as one, SolveBatch leaves the count alone — cells of both records show its 0.)
static Settled cursor_settle(ksolve_handle* h, const FastOutcome& o, bool plan1_only = false) {
  if (o.done) {
    h->engine_used = 2;
    h->fast_reason = 0;   // (a first attempt that ran out of LDS claim slots is not a fallback to the general engine)
    if (o.n_claims) be_launch_fast_records(h, o.n_claims);
    if (h->fw.unsched) be_launch_fast_unsched(h);   // the errors of the pods it set aside (none: nothing is written)
    return Settled::Done;
  }
  h->fast_reason = o.reason;   // (DECLINE_CAPACITY, 100 = more claims than max_claims: the general engine reports it, or moves to BIG)
  if (next_plan_after_claim_slots(h, o, plan1_only)) return Settled::NextPlan;
  if (h->eng.refuses()) { declined(h, "cursor"); return Settled::Refused; }
  h->fw.enabled = 0;   // later solves of this handle go straight to the general engine
  return Settled::HandBack;
}

static void be_results_drop(ksolve_results* r) { if (r && r->impl) { delete (ResultsImpl*)r->impl; r->impl = nullptr; } }

static ksolve_status solve(ksolve_handle* h, ksolve_results* out, bool fresh_context = true) {
  memset(out, 0, sizeof(*out));
  ksolve_status st = refused_unprepared(h);
  if (st != KSOLVE_OK) return st;
  if (h->base) { solve_probes(&h, 1, out, &st, fresh_context); return st; }
  st = solve_prepare(h, fresh_context);
  if (st == KSOLVE_OK) st = refused_before_launch(h);
  if (st != KSOLVE_OK) return st;
  if (h->tw.enabled && h->n_pods && h->n_classes) {
    alloc_run_order(h);   // (in front of the pack timer, which covers the static node rows)
    be_tic(h, T_PACK);
    spread_before_launch(h);
    if (h->tw.nd.dom) be_launch_pack_topo_nodes(h); else be_launch_pack_topo(h);
    be_toc(h, T_PACK);
    const Settled s = spread_settle(h, fast_outcome(h));
    if (s == Settled::Done) return solve_finish(h, out);
    if (s == Settled::Refused) return KSOLVE_ERR_UNSUPPORTED;
    st = solve_prepare(h, false);
    if (st != KSOLVE_OK) return st;
  }
  if (h->fw.enabled && !h->pv.big && h->n_pods && h->n_classes) {
    h->fast_attempts = 0;
    for (Settled s = Settled::NextPlan; s == Settled::NextPlan;) {
      h->fast_attempts++;
      be_tic(h, T_PACK);
      if (h->fw.nodes) fast_nodes_stage(h);   // existing nodes first (scheduler.go:594); the loop solves the pods they left
      be_launch_pack_fast(h);
      be_toc(h, T_PACK);
      s = cursor_settle(h, fast_outcome(h));
      if (s == Settled::Done) return solve_finish(h, out);
      if (s == Settled::Refused) return KSOLVE_ERR_UNSUPPORTED;
      st = solve_prepare(h, false);   // (NextPlan: once more with the claims' state in HBM; HandBack: for the general engine)
      if (st != KSOLVE_OK) return st;
    }
  }
  be_tic(h, T_PACK);
  if (h->n_pods) be_launch_pack(h);
  be_toc(h, T_PACK);
  if (!h->pv.big && h->big_capable) {
    int status = 0;
    be_d2h(h, &status, h->ws.status_out, 4);
    be_sync(h);
    if (status == 1) {
      // more in-flight claims than the LDS-resident order holds: this problem runs on the BIG engine from now on
      h->pv.big = 1; h->pv.lite = 0; h->pv.lds = h->lds_big;
      alloc_run_order(h);
      st = solve_prepare(h, false);
      if (st != KSOLVE_OK) return st;
      be_tic(h, T_PACK);
      be_launch_pack(h);
      be_toc(h, T_PACK);
    }
  }
  return solve_finish(h, out);
}

// ---- what the two calls over many handles share -------------------------------------------------------------------------------------

// The prepass (classes, queue order) and the result download of different problems are independent: a few host threads drive them on
// the problems' own streams so that the launches and copies of different problems overlap.
template <class Fn>
static void parallel_over(ksolve_handle** hs, uint32_t n, Fn&& fn) {
  const uint32_t n_threads = std::min<uint32_t>(n, std::max(1u, std::min(8u, std::thread::hardware_concurrency())));
  if (n_threads <= 1) { for (uint32_t i = 0; i < n; ++i) fn(i); return; }
  std::vector<std::thread> pool;
  for (uint32_t t = 0; t < n_threads; ++t) pool.emplace_back([&, t]() { be_thread_init(hs[0]); for (uint32_t i = t; i < n; i += n_threads) fn(i); });
  for (auto& th : pool) th.join();
}
// a member solved on its own through solve(): its results are complete
static ksolve_status solve_alone(ksolve_handle* h, ksolve_results* out) {
  be_results_drop(out);
  const ksolve_status st = solve(h, out, false);
  out->status = st;
  return st;
}
// handed back by a fast engine: prepared anew for the general engine's batched launch
static ksolve_status hand_back(ksolve_handle* h) {
  const ksolve_status st = solve_prepare(h, false);
  if (st == KSOLVE_OK) be_sync(h);
  return st;
}
static std::vector<ksolve_handle*> handles_of(ksolve_handle** hs, const std::vector<uint32_t>& idx) {
  std::vector<ksolve_handle*> g;
  for (uint32_t i : idx) g.push_back(hs[i]);
  return g;
}
// solve_finish for every member whose answer does not stand yet (done: refused, failed or solved alone)
static void finish_members(ksolve_handle** hs, uint32_t n, ksolve_results* outs, std::vector<ksolve_status>& st, const std::vector<char>& done) {
  parallel_over(hs, n, [&](uint32_t i) {
    if (done[i] || st[i] != KSOLVE_OK) { outs[i].status = st[i]; return; }
    st[i] = solve_finish(hs[i], &outs[i]);
    if (st[i] == KSOLVE_ERR_CAPACITY && hs[i]->big_capable && !hs[i]->pv.big) { be_results_drop(&outs[i]); st[i] = solve(hs[i], &outs[i], false); }   // re-run alone on the BIG engine
    outs[i].status = st[i];   // solve_finish zeroes `out` before it can fail: the per-problem status must survive that
  });
}
static ksolve_status worst_of(const std::vector<ksolve_status>& st) {
  ksolve_status worst = KSOLVE_OK;
  for (ksolve_status s : st) if (s != KSOLVE_OK && s != KSOLVE_ERR_CANCELLED) worst = s;
  return worst;
}

// Many independent problems, one launch: block b of the pack kernel is the wavefront of problem b. This is how
// consolidation sweeps (helpers.go:53-155: one Solve() per candidate set) and NodePool components fill the chip.
// Problems of the cursor engine's shape go to it (one block each); the ones it hands back (status 3), and all others, run on the
// general engine's batched launch.
static ksolve_status solve_batch_plain(ksolve_handle** hs, uint32_t n, ksolve_results* outs, ksolve_many_stats&) {
  for (uint32_t i = 0; i < n; ++i) memset(&outs[i], 0, sizeof(outs[i]));
  std::vector<ksolve_status> st(n, KSOLVE_OK);
  std::vector<char> done(n, 0);
  auto alone = [&](uint32_t i) { st[i] = solve_alone(hs[i], &outs[i]); done[i] = 1; };
  parallel_over(hs, n, [&](uint32_t i) { st[i] = solve_prepare(hs[i]); outs[i].status = st[i]; if (st[i] == KSOLVE_OK) be_sync(hs[i]); });
  std::vector<uint32_t> fast, run;
  for (uint32_t i = 0; i < n; ++i) {
    ksolve_handle* h = hs[i];
    if (st[i] != KSOLVE_OK || !h->n_pods) continue;
    if (spread_takes_alone_in_batch(h)) alone(i);
    else if (h->fw.enabled && !h->pv.big && h->n_classes) { if (batched_cursor_takes(h, /*legacy_batch=*/true)) fast.push_back(i); else alone(i); }
    else if (h->eng.refuses()) st[i] = fail(h, KSOLVE_ERR_UNSUPPORTED, "cursor engine requested for a problem outside its shape");   // (the batch path's short form; a spread-only handle gets the cursor wording too: a known wart)
    else run.push_back(i);
  }
  if (!fast.empty()) {
    std::vector<ksolve_handle*> g = handles_of(hs, fast);
    be_launch_pack_fast_batch(g.data(), (int)g.size());
    std::vector<Settled> how;   // every member's outcome and records first, then what the handed-back ones need
    for (ksolve_handle* h : g) how.push_back(cursor_settle(h, fast_outcome(h), /*plan1_only=*/true));
    for (size_t k = 0; k < fast.size(); ++k) {
      const uint32_t i = fast[k];
      if (how[k] == Settled::NextPlan) alone(i);   // more in-flight claims than the LDS plan holds: alone, on the plans that keep them in HBM
      else if (how[k] == Settled::Refused) st[i] = KSOLVE_ERR_UNSUPPORTED;
      else if (how[k] == Settled::HandBack && (st[i] = hand_back(hs[i])) == KSOLVE_OK) run.push_back(i);
    }
  }
  if (!run.empty()) { std::vector<ksolve_handle*> g = handles_of(hs, run); be_launch_pack_batch(g.data(), (int)g.size()); }
  finish_members(hs, n, outs, st, done);
  return worst_of(st);
}

// ---------------------------------------------------------------------------------------------------------------------------
// ksolve_solve_many: many problems in one call, each on the engine solve() would run — every member gets the result solve() would have
// given it on a fresh handle (outcome, error text, engine, fallback reason, memory plan, attempts, digest), and members of the spread
// engine's shape share launches: refusals -> the spread engine's many-problem launches (one per kernel flavour present) -> the cursor
// engine's batched launch (alone where solve() would run another kernel) -> the general engine's batched launch, with whatever the
// fast engines handed back.
// the many-problem form of the kernel be_launch_pack_topo would pick (pack_flavours.h); nullptr: there is none, the member runs alone
static const ks::PackTopoRow* topo_many_row(const ksolve_handle* h) { return ks::pack_topo_many_row(ks::topo_flavour(h->fw), h->tw.nd.dom != nullptr); }
// the order table of one launch: its members by pod count, largest first (ties in input order); tickets are handed out along it
static void topo_many_order(const std::vector<ksolve_handle*>& g, uint32_t* order) {
  for (size_t i = 0; i < g.size(); ++i) order[i] = (uint32_t)i;
  std::stable_sort(order, order + g.size(), [&](uint32_t a, uint32_t b) { return g[a]->n_pods > g[b]->n_pods; });
}

static ksolve_status solve_many_plain(ksolve_handle** hs, uint32_t n, ksolve_results* outs, ksolve_many_stats& S) {
  for (uint32_t i = 0; i < n; ++i) memset(&outs[i], 0, sizeof(outs[i]));
  std::vector<ksolve_status> st(n, KSOLVE_OK);
  std::vector<char> done(n, 0);   // the member's answer stands: refused, failed, or solved alone (results complete)
  auto refuse = [&](uint32_t i, ksolve_status s) { st[i] = s; done[i] = 1; };
  auto alone = [&](uint32_t i) { st[i] = solve_alone(hs[i], &outs[i]); done[i] = 1; S.alone_members++; };
  for (uint32_t i = 0; i < n; ++i) { const ksolve_status r = refused_unprepared(hs[i]); if (r != KSOLVE_OK) refuse(i, r); }
  parallel_over(hs, n, [&](uint32_t i) { if (done[i]) return; st[i] = solve_prepare(hs[i]); if (st[i] == KSOLVE_OK) be_sync(hs[i]); else done[i] = 1; });
  std::vector<uint32_t> spread, fast, run;
  for (uint32_t i = 0; i < n; ++i) {
    ksolve_handle* h = hs[i];
    if (done[i]) continue;
    const ksolve_status r = refused_before_launch(h);
    if (r != KSOLVE_OK) { refuse(i, r); continue; }
    if (!h->n_pods) continue;   // nothing to launch: solve_finish
    if (h->tw.enabled && h->n_classes) {
      // (engines 29 / 30: the kernels with the pod operators have no many-problem form — a launch of its own, as solve() makes it)
      if (topo_many_row(h)) spread.push_back(i); else alone(i);
    }
    else if (h->fw.enabled && !h->pv.big && h->n_classes) { if (batched_cursor_takes(h, /*legacy_batch=*/false)) fast.push_back(i); else alone(i); }
    else run.push_back(i);
  }
  auto to_general = [&](uint32_t i) {
    if ((st[i] = hand_back(hs[i])) != KSOLVE_OK) { done[i] = 1; return; }
    run.push_back(i); S.handed_back++;
  };
  if (!spread.empty()) {
    std::vector<ksolve_handle*> groups[ks::kTopoManyFlavours];
    for (uint32_t i : spread) { spread_before_launch(hs[i]); groups[topo_many_row(hs[i]) - ks::kPackTopoManyRows].push_back(hs[i]); }
    be_launch_pack_topo_many(groups);
    for (auto& g : groups) if (!g.empty()) S.spread_launches++;
    S.spread_members += (uint32_t)spread.size();
    for (uint32_t i : spread) {
      const Settled s = spread_settle(hs[i], fast_outcome(hs[i]));
      if (s == Settled::Refused) refuse(i, KSOLVE_ERR_UNSUPPORTED);
      else if (s == Settled::HandBack) to_general(i);
    }
  }
  if (!fast.empty()) {
    std::vector<ksolve_handle*> g = handles_of(hs, fast);
    be_launch_pack_fast_batch(g.data(), (int)g.size());
    S.cursor_members += (uint32_t)fast.size();
    for (uint32_t i : fast) {
      ksolve_handle* h = hs[i];
      h->fast_attempts = 1;   // the runs of the cursor engine this solve took, as solve() counts them: handed back or not
      const Settled s = cursor_settle(h, fast_outcome(h));
      if (s == Settled::NextPlan) {
        // alone on the plan solve() would move to after this attempt. solve() counts its own runs from zero and is not to be touched:
        // the batched run is added to what it reports, on the handle and in the results it filled. (The member is in cursor_members
        // and in alone_members: ksolve.h says so.)
        alone(i);
        h->fast_attempts++;
        if (outs[i].impl) outs[i].cursor_attempts++;
      }
      else if (s == Settled::Refused) refuse(i, KSOLVE_ERR_UNSUPPORTED);
      else if (s == Settled::HandBack) to_general(i);
    }
  }
  if (!run.empty()) {
    std::vector<ksolve_handle*> g = handles_of(hs, run);
    be_launch_pack_batch(g.data(), (int)g.size());
    S.general_members += (uint32_t)run.size();
  }
  finish_members(hs, n, outs, st, done);
  for (ksolve_status s : st) if (s == KSOLVE_ERR_UNSUPPORTED) S.refused++;
  return worst_of(st);
}

// ---- devices and probes: the same for both calls; `plain` is solve_batch_plain or solve_many_plain ------------------------------------

// one device: probes of a resident cluster run as one sweep per base handle, everything else through `plain`
template <class Plain>
static ksolve_status probes_then_plain(ksolve_handle** hs, uint32_t n, ksolve_results* outs, ksolve_many_stats& S, Plain plain) {
  std::vector<uint32_t> plain_idx;
  std::vector<ksolve_handle*> bases;
  for (uint32_t i = 0; i < n; ++i) {
    if (!hs[i]->base) { plain_idx.push_back(i); continue; }
    S.probe_members++;
    if (std::find(bases.begin(), bases.end(), hs[i]->base) == bases.end()) bases.push_back(hs[i]->base);
  }
  if (bases.empty()) return plain(hs, n, outs, S);
  ksolve_status worst = KSOLVE_OK;
  for (ksolve_handle* b : bases) {
    std::vector<uint32_t> idx;
    std::vector<ksolve_handle*> g;
    for (uint32_t i = 0; i < n; ++i) if (hs[i]->base == b) { idx.push_back(i); g.push_back(hs[i]); }
    std::vector<ksolve_results> ro(g.size());
    std::vector<ksolve_status> st(g.size(), KSOLVE_OK);
    solve_probes(g.data(), (uint32_t)g.size(), ro.data(), st.data(), true);
    for (size_t k = 0; k < g.size(); ++k) outs[idx[k]] = ro[k];
    const ksolve_status rc = worst_of(st);
    if (rc != KSOLVE_OK) worst = rc;
  }
  if (!plain_idx.empty()) {
    std::vector<ksolve_handle*> g = handles_of(hs, plain_idx);
    std::vector<ksolve_results> ro(g.size());
    const ksolve_status rc = plain(g.data(), (uint32_t)g.size(), ro.data(), S);
    for (size_t k = 0; k < g.size(); ++k) outs[plain_idx[k]] = ro[k];
    if (rc != KSOLVE_OK) worst = rc;
  }
  return worst;
}

// the handles' devices side by side (one host thread each), one probes_then_plain per device; the counters summed into `stats` if given
template <class Plain>
static ksolve_status by_device(ksolve_handle** hs, uint32_t n, ksolve_results* outs, ksolve_many_stats* stats, Plain plain) {
  std::vector<int> devices;
  for (uint32_t i = 0; i < n; ++i) { const int dv = be_device_of(hs[i]); if (std::find(devices.begin(), devices.end(), dv) == devices.end()) devices.push_back(dv); }
  ksolve_many_stats sum{};
  ksolve_status worst = KSOLVE_OK;
  if (devices.size() <= 1) worst = probes_then_plain(hs, n, outs, sum, plain);
  else {
    std::vector<ksolve_many_stats> part(devices.size(), ksolve_many_stats{});
    std::vector<ksolve_status> rc(devices.size(), KSOLVE_OK);
    std::vector<std::thread> pool;
    for (size_t g = 0; g < devices.size(); ++g) pool.emplace_back([&, g]() {
      std::vector<uint32_t> idx;
      std::vector<ksolve_handle*> grp;
      for (uint32_t i = 0; i < n; ++i) if (be_device_of(hs[i]) == devices[g]) { idx.push_back(i); grp.push_back(hs[i]); }
      be_thread_init(grp[0]);
      std::vector<ksolve_results> ro(grp.size());
      rc[g] = probes_then_plain(grp.data(), (uint32_t)grp.size(), ro.data(), part[g], plain);
      for (size_t k = 0; k < grp.size(); ++k) outs[idx[k]] = ro[k];
    });
    for (auto& th : pool) th.join();
    for (auto r : rc) if (r != KSOLVE_OK) worst = r;
    for (const ksolve_many_stats& p : part) {
      sum.spread_launches += p.spread_launches; sum.spread_members += p.spread_members; sum.cursor_members += p.cursor_members;
      sum.general_members += p.general_members; sum.handed_back += p.handed_back; sum.alone_members += p.alone_members;
      sum.probe_members += p.probe_members; sum.refused += p.refused;
    }
  }
  if (stats) *stats = sum;
  return worst;
}
static ksolve_status solve_batch(ksolve_handle** hs, uint32_t n, ksolve_results* outs) { return by_device(hs, n, outs, nullptr, solve_batch_plain); }   // (SolveBatch reports no counters)
static ksolve_status solve_many(ksolve_handle** hs, uint32_t n, ksolve_results* outs, ksolve_many_stats* stats) { return by_device(hs, n, outs, stats, solve_many_plain); }
