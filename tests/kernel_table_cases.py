"""Which pack kernel a handle launches (csrc/pack_flavours.h: the flavours, the kernel matrix and its lookups) — the cases that
tests/test_kernel_table.py runs through the host emulation and tests/test_gpu_kernel_table.py on the device's test build. Both export
ksolve_test_last_pack_kernel / ksolve_test_previous_pack_kernel (test builds only): the fast engines' pack kernel launched for a handle
last and the one before it, asked here of the solver library itself, on the session's handle (ksched_solver_handle). The emulation
names the kernel the device backend would launch, from the same lookup. A handle launched on a kernel of a later flavour would pass every
parity test and be slower: the names are written here, beside the problems."""
import ctypes

import engine_checks as ec
import existing_node_cases as en
import pod_operator_cases as pc
import solve_many_cases as mc
import spread_pod_operator_cases as sp
import unschedulable_cases as uc
from karpenter_amd import fixtures as fx
from karpenter_amd.scheduling import NewScheduler

# solve_many_cases.flavour_members() in its order: the kernel of the member solved alone, and as a member of one SolveMany
# ("": no fast engine's pack kernel ran — the general engine's member, and the member without pods)
FLAVOUR_KERNELS = [("ksolve_pack_topo", "ksolve_pack_topo_many"),
                   ("ksolve_pack_topo_nodes", "ksolve_pack_topo_nodes_many"),
                   ("ksolve_pack_topo_u", "ksolve_pack_topo_many_u"),
                   ("ksolve_pack_topo_nodes_u", "ksolve_pack_topo_nodes_many_u"),
                   ("ksolve_pack_topo_f", "ksolve_pack_topo_many_f"),
                   ("ksolve_pack_topo_nodes_f", "ksolve_pack_topo_nodes_many_f"),
                   ("ksolve_pack_topo", "ksolve_pack_topo_many"),           # complement templates: the plain kernel
                   ("ksolve_pack_topo", "ksolve_pack_topo_many"),           # ... with DaemonSets
                   ("ksolve_pack_fast_g0r1", "ksolve_pack_fast_batch"),     # the cursor engine: alone on the LDS plan, batched in the call
                   ("", ""),
                   ("", "")]


def config1_slice():
    return fx.config1(pods=300, n_types=144, seed=7)


def sixteen_nodepools():
    """test_loop_events.sixteen_nodepools: more than 64 pod classes live at once."""
    return fx.config4(pods=8000, n_types=200, n_pools=16, seed=42)


def positive_problem_with_nodes():
    """With existing nodes the spread engine's pod operators take positive pods only: the first of
    spread_pod_operator_cases.positive_problems() that has nodes. The setting picks the kernel, not the batch."""
    return next(p for p in sp.positive_problems() if p.get("stateNodes"))


# (name, problem, setting, engine, the pack kernel before the last one, the last one).
# The unschedulable batch is the one without the 10,000-cpu pod: that pod alone lifts the library's lower bound of the NodeClaims the
# batch needs (total requests over the largest allocatable) past the few the batch's LDS plan is cut to, and the handle starts on a
# later plan; two pods of an absent zone leave the batch on the LDS plan.
def lone_cases():
    return [("cursor-pod-operators", pc.zone_notin_problem, "cursor-pod-operators", "cursor", "", "ksolve_pack_fast_p_g0r1"),
            ("spread-pod-operators", sp.own_notin_problem, "spread-pod-operators", "spread", "", "ksolve_pack_topo_p"),
            ("spread-pod-operators-nodes", positive_problem_with_nodes, "spread-pod-operators", "spread", "", "ksolve_pack_topo_nodes_p"),
            ("cursor-unschedulable", lambda: uc.plain_batch(0, 2), "cursor-unschedulable", "cursor", "", "ksolve_pack_fast_u_g0r1"),
            ("cursor", config1_slice, "cursor", "cursor", "", "ksolve_pack_fast_g0r1"),
            ("cursor-wide", config1_slice, "cursor-wide", "cursor", "", "ksolve_pack_fast_g1r1"),
            ("cursor-hbm", config1_slice, "cursor-hbm", "cursor", "", "ksolve_pack_fast_g2r1"),
            ("cursor-pair", config1_slice, "cursor-pair", "cursor", "", "ksolve_pack_fast2"),
            ("four-rows", sixteen_nodepools, "cursor", "cursor", "", "ksolve_pack_fast_g0r4"),
            ("cursor-nodes", lambda: en.block_edge_problem(63), "cursor-nodes", "cursor", "ksolve_pack_nodes_lds", "ksolve_pack_fast_g0r1")]


def kernels_of(sched):
    """(the pack kernel before the last one, the last one) of an open scheduler's handle; "" for none."""
    lib = ctypes.CDLL(sched._solver_lib)
    sched._lib.ksched_solver_handle.restype = ctypes.c_void_p
    sched._lib.ksched_solver_handle.argtypes = [ctypes.c_void_p]
    handle = sched._lib.ksched_solver_handle(sched._session)
    assert handle
    names = []
    for fn in (lib.ksolve_test_previous_pack_kernel, lib.ksolve_test_last_pack_kernel):
        fn.restype, fn.argtypes = ctypes.c_char_p, [ctypes.c_void_p]
        names.append((fn(handle) or b"").decode())
    return tuple(names)


def solve(prob, setting, lib):
    """engine_checks.solve, with the handle's kernel names read before the scheduler is closed -> (Results, names)."""
    s = NewScheduler(mc.with_engine(prob, setting), solver_lib=lib)
    try:
        res = s.Solve()
        return res, kernels_of(s)
    finally:
        s.close()


def check_lone(oracle, lib, case):
    """One case: the engine, the kernels' names, and the result against the oracle."""
    _, make, setting, engine, before, last = case
    prob = make()
    got, names = solve(prob, setting, lib)
    assert ec.where(got) == (engine, 0), ec.where(got)
    assert names == (before, last)
    ec.same(got, oracle.solve(prob), prob)


def check_flavour_members_alone(oracle, lib):
    """Every member of flavour_members() solved alone under its setting."""
    for i, ((prob, setting), (alone, _), engine) in enumerate(zip(mc.flavour_members(), FLAVOUR_KERNELS, mc.FLAVOUR_ENGINES)):
        got, names = solve(prob, setting, lib)
        assert got["counters"]["engine"] == engine, (i, ec.where(got))
        assert names[1] == alone, (i, names)
        ec.same(got, oracle.solve(prob), prob)


def check_flavour_members_many(oracle, lib):
    """... and through one SolveMany: the six many-problem kernels, the batched cursor kernel."""
    members = mc.flavour_members()
    scheds = mc.open_members(members, lib)
    try:
        results, stats = mc.many(scheds)
        names = [kernels_of(s)[1] for s in scheds]
    finally:
        mc.close_all(scheds)
    assert stats["spread_launches"] == 6 and stats["spread_members"] == 8, stats
    assert [r["counters"]["engine"] for r in results] == mc.FLAVOUR_ENGINES
    assert names == [many for _, many in FLAVOUR_KERNELS]
    mc.same_as_oracle(oracle, members, results)
