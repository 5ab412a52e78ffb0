"""The one statement of how a fast engine's opt-in setting is tested (TEST INFRASTRUCTURE, importable like parity): a pair of
`ksolve_options.engine` values — "auto-X" and the engine-only "cursor-X" / "spread-X", rows 7-27 of csrc/engine_setting.h — is
described by a Switch, and Switch.check / Switch.declined hold one problem against the oracle under the pair and under the settings
one step below it. The case modules (tests/*_cases.py) declare their Switch; the test files call solve / same / where / refusal here."""
from typing import NamedTuple, Optional, Tuple

import parity
from karpenter_amd.scheduling import NewScheduler, Unsupported

# how same() compares the instance-type lists of a NodeClaim
STRICT = "strict"                # in order, always
SETS_UNDER_DAEMONSETS = "ds"     # in order, except in a problem with DaemonSets (same() is given the problem)
SETS = "sets"                    # as sets, always (test bodies that hold a result of a DaemonSet problem without the problem)
FAST = ("cursor", "spread")


def solve(prob, engine, lib):
    s = NewScheduler(dict(prob, options=dict(prob.get("options", {}), engine=engine)), solver_lib=lib)
    try:
        return s.Solve()
    finally:
        s.close()


def where(res):
    return res["counters"]["engine"], res["counters"]["engineFallbackReason"]


def refusal(prob, engine, lib):
    """The text of the Unsupported that `engine` answers the problem with."""
    try:
        solve(prob, engine, lib)
    except Unsupported as e:
        return str(e)
    raise AssertionError(f"{engine} solved a problem it must refuse")


def refusal_says(text, kind, reason, by_host=False):
    """The rule for a refusal's text. The engine — or the host on its behalf, once the handle exists — declined: "declined the problem
    (reason N)". Reason 0, or by_host — the host found the batch outside the engine's shape when it created the handle and never
    asked the engine —: "requested for a problem outside its shape", with the reason where the host left one."""
    if reason == 0 or by_host:
        assert f"{kind} engine requested for a problem outside its shape" in text and (reason == 0 or text.endswith(f"(reason {reason})")), (reason, text)
    else:
        assert f"{kind} engine declined the problem (reason {reason})" in text, (reason, text)


def sorted_its(res):
    """Daemon-overhead groups are visited in Go map order by the reference (scheduler.go:1001), so the order of
    InstanceTypeOptions across groups is not defined: compare them as sets. IN PLACE: take a digest before."""
    for c in res["newNodeClaims"]:
        c["instanceTypes"] = sorted(c["instanceTypes"])
    return res


def same(got, want, prob=None, mode=SETS_UNDER_DAEMONSETS):
    """Claims and their order, pod assignment, requirements, existing nodes, pod errors with their flags (parity), the
    reference-equivalent evaluation count (V) and the packing cost. Without `prob` the default mode is the strict one."""
    if mode == SETS or (mode == SETS_UNDER_DAEMONSETS and prob is not None and prob.get("daemonSetPods")):
        sorted_its(got), sorted_its(want)
    parity.assert_same_results(got, want)
    assert got["counters"]["referenceBinEvaluations"] == want["counters"]["binEvaluations"]
    assert abs(got["packingCost"] - want["packingCost"]) < 1e-9 * max(1.0, want["packingCost"])


def same_pops(got, want, what=None):
    assert got["counters"]["pops"] == want["counters"]["pops"], (what, got["counters"]["pops"], want["counters"]["pops"])


def digests_of_repeated_solves(lib, prob, engine, n, kind):
    """n solves on one handle, each on the `kind` engine with reason 0 -> (the set of digests, the last result)."""
    s = NewScheduler(dict(prob, options=dict(prob.get("options", {}), engine=engine)), solver_lib=lib)
    try:
        out = set()
        for _ in range(n):
            r = s.Solve()
            assert where(r) == (kind, 0), r["counters"]
            out.add(parity.results_digest(r)[0])
        return out, r
    finally:
        s.close()


class Switch(NamedTuple):
    """One opt-in pair and what stands one step below it."""
    kind: str                                   # the fast engine: "cursor" or "spread"
    only: str                                   # the engine-only setting with the switch: solves on `kind` or refuses
    auto: str                                   # the "auto-" setting with the switch: falls back to the general engine
    base: str = "auto"                          # the "auto-" setting below the switch: falls back with a base reason
    base_only: Optional[str] = None             # the engine-only setting below the switch: refuses (None: no such leg)
    reasons: Optional[Tuple[int, ...]] = None   # the base reasons (None: given per call)
    base_only_declines: Optional[Tuple[int, ...]] = None   # the base reasons `base_only` declines with; any other the host finds first (None: all)
    errors: Optional[bool] = None               # the oracle's result must (True), must not (False) or may (None) carry pod errors
    pops: bool = False                          # queue pops are compared with the oracle's
    mode: str = SETS_UNDER_DAEMONSETS           # how instance-type lists are compared (same())
    base_first: bool = False                    # declined() shows first that `base` stops earlier, with a base reason

    def same(self, got, want, prob):
        same(got, want, prob, self.mode)

    def check(self, oracle, lib, prob, *, reason=None, base=None, base_only=None, want=None):
        """One problem five ways. The oracle once (`want`: computed before). `base` hands the problem to the general engine with a
        base reason and equals the oracle; `base_only` refuses and names that reason. `only` solves it on the fast engine — no
        fallback, reason 0 — and equals the oracle; `auto` gives the same digest on the same engine and equals the oracle too.
        Returns (the result under `only`, the oracle's)."""
        reasons = self.reasons if reason is None else (reason,)
        base_only = base_only or self.base_only
        want = want or oracle.solve(prob)
        if self.errors is not None:
            assert bool(want["podErrors"]) == self.errors, ("the oracle schedules every pod of this problem" if self.errors else want["podErrors"])
        plain = solve(prob, base or self.base, lib)
        assert plain["counters"]["engine"] == "general" and plain["counters"]["engineFallbackReason"] in reasons, plain["counters"]
        self.same(plain, want, prob)
        if base_only is not None:
            (r,) = reasons   # (a pair with an engine-only setting below it has ONE base reason)
            refusal_says(refusal(prob, base_only, lib), self.kind, r, by_host=self.base_only_declines is not None and r not in self.base_only_declines)
        out = []
        for engine in (self.only, self.auto):
            got = solve(prob, engine, lib)
            assert where(got) == (self.kind, 0), (engine, got["counters"])
            out.append((got, parity.results_digest(got)[0]))   # (the digest before same(), which may sort the instance-type lists in place)
            self.same(got, want, prob)
            if self.pops:
                same_pops(got, want, engine)
        assert out[0][1] == out[1][1]
        return out[0][0], want

    def declined(self, oracle, lib, prob, reason, *, base_reasons=None):
        """A problem the fast engine still hands back with the switch: `only` refuses and names `reason`, `auto` equals the oracle on
        the general engine with that reason. Returns the result under `auto`."""
        if self.base_first:
            plain = solve(prob, self.base, lib)
            assert plain["counters"]["engine"] == "general" and plain["counters"]["engineFallbackReason"] in (base_reasons or self.reasons), plain["counters"]
        refusal_says(refusal(prob, self.only, lib), self.kind, reason)
        auto = solve(prob, self.auto, lib)
        assert where(auto) == ("general", reason), auto["counters"]
        self.same(auto, oracle.solve(prob), prob)
        return auto


def three_ways(oracle, lib, prob, engine, auto="auto", plans=(), kind=None, mode=SETS_UNDER_DAEMONSETS):
    """The form without a switch: `engine` must solve the problem on the `kind` engine (its own name by default) — no fallback,
    reason 0 — and equal the oracle; so must `auto` (which has to pick the same engine), the general engine, and every further
    setting of `plans`. Returns (the result under `engine`, the oracle's)."""
    kind = kind or engine
    want = oracle.solve(prob)
    first = None
    for setting in (engine, auto, "general") + tuple(plans):
        got = solve(prob, setting, lib)
        assert where(got) == (kind, 0) if setting != "general" else got["counters"]["engine"] == "general", (setting, got["counters"])
        same(got, want, prob, mode)
        first = first or got
    return first, want


def fuzz_cases(oracle, lib, problems, engine, *, pops, mode=SETS_UNDER_DAEMONSETS):
    """Over (seed, problem): whatever `engine` runs equals the oracle (and, if asked, in queue pops); a fast engine ends with reason 0,
    anything else is the general engine. Yields (seed, problem, the oracle's result, the result, the engine that ran, its reason)."""
    for seed, prob in problems:
        want = oracle.solve(prob)
        got = solve(prob, engine, lib)
        same(got, want, prob, mode)
        if pops:
            same_pops(got, want, seed)
        ran, reason = where(got)
        assert reason == 0 if ran in FAST else ran == "general", (seed, got["counters"])
        yield seed, prob, want, got, ran, reason
