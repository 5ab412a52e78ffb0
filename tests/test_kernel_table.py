"""csrc/pack_flavours.h — the flavours of the fast engines' pack kernels, the kernel matrix and its lookups — held against a literal
table (CPU): every list row and every lookup over the full ranges, printed by a g++ program that includes the header; the compile
jobs of the build against the same table; and, on the host emulation, which kernel a handle launches (tests/kernel_table_cases.py;
tests/test_gpu_kernel_table.py on the device). The table below was written from the declarations of csrc/pack_kernels.h and the
ladders of ksolve.hip at the commit before the header existed, not from the header."""
import os
import subprocess

import pytest

import kernel_table_cases as kc
from test_device_algorithm import emu  # noqa: F401  (fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# family kernel flavour (0 plain, 1 + set-aside list, 2 + [spread: node filters, 3 +] pod operators) then plan rows | nodes
ROWS = """\
fast ksolve_pack_fast_g0r1 0 0 1
fast ksolve_pack_fast_g1r1 0 1 1
fast ksolve_pack_fast_g2r1 0 2 1
fast ksolve_pack_fast_g0r4 0 0 4
fast ksolve_pack_fast_g1r4 0 1 4
fast ksolve_pack_fast_g2r4 0 2 4
fast ksolve_pack_fast_u_g0r1 1 0 1
fast ksolve_pack_fast_u_g1r1 1 1 1
fast ksolve_pack_fast_u_g2r1 1 2 1
fast ksolve_pack_fast_u_g0r4 1 0 4
fast ksolve_pack_fast_u_g1r4 1 1 4
fast ksolve_pack_fast_u_g2r4 1 2 4
fast ksolve_pack_fast_p_g0r1 2 0 1
fast ksolve_pack_fast_p_g1r1 2 1 1
fast ksolve_pack_fast_p_g2r1 2 2 1
fast ksolve_pack_fast_p_g0r4 2 0 4
fast ksolve_pack_fast_p_g1r4 2 1 4
fast ksolve_pack_fast_p_g2r4 2 2 4
topo ksolve_pack_topo 0 0
topo ksolve_pack_topo_nodes 0 1
topo ksolve_pack_topo_u 1 0
topo ksolve_pack_topo_nodes_u 1 1
topo ksolve_pack_topo_f 2 0
topo ksolve_pack_topo_nodes_f 2 1
topo ksolve_pack_topo_p 3 0
topo ksolve_pack_topo_nodes_p 3 1
many ksolve_pack_topo_many 0 0
many ksolve_pack_topo_nodes_many 0 1
many ksolve_pack_topo_many_u 1 0
many ksolve_pack_topo_nodes_many_u 1 1
many ksolve_pack_topo_many_f 2 0
many ksolve_pack_topo_nodes_many_f 2 1
cold ksolve_test_fast_cold_g0r1 0 0 1
cold ksolve_test_fast_cold_g0r4 0 0 4
cold ksolve_test_fast_cold_u_g0r1 1 0 1
cold ksolve_test_fast_cold_u_g0r4 1 0 4
cold ksolve_test_fast_cold_p_g0r1 2 0 1
cold ksolve_test_fast_cold_p_g0r4 2 0 4
cold ksolve_test_fast_cold_g1r1 0 1 1
cold ksolve_test_fast_cold_u_g2r4 1 2 4
"""
# the template bools of every flavour (US PO | US FS PO), the number of many-problem kernels, then every lookup: "-" where no kernel exists
TRAITS_AND_LOOKUPS = """\
fast-traits 0 0 0
fast-traits 1 1 0
fast-traits 2 1 1
topo-traits 0 0 0 0
topo-traits 1 1 0 0
topo-traits 2 1 1 0
topo-traits 3 1 1 1
many-flavours 6
fast? 0 0 1 ksolve_pack_fast_g0r1
fast? 0 0 4 ksolve_pack_fast_g0r4
fast? 0 1 1 ksolve_pack_fast_g1r1
fast? 0 1 4 ksolve_pack_fast_g1r4
fast? 0 2 1 ksolve_pack_fast_g2r1
fast? 0 2 4 ksolve_pack_fast_g2r4
fast? 1 0 1 ksolve_pack_fast_u_g0r1
fast? 1 0 4 ksolve_pack_fast_u_g0r4
fast? 1 1 1 ksolve_pack_fast_u_g1r1
fast? 1 1 4 ksolve_pack_fast_u_g1r4
fast? 1 2 1 ksolve_pack_fast_u_g2r1
fast? 1 2 4 ksolve_pack_fast_u_g2r4
fast? 2 0 1 ksolve_pack_fast_p_g0r1
fast? 2 0 4 ksolve_pack_fast_p_g0r4
fast? 2 1 1 ksolve_pack_fast_p_g1r1
fast? 2 1 4 ksolve_pack_fast_p_g1r4
fast? 2 2 1 ksolve_pack_fast_p_g2r1
fast? 2 2 4 ksolve_pack_fast_p_g2r4
topo? 0 0 ksolve_pack_topo
topo? 0 1 ksolve_pack_topo_nodes
topo? 1 0 ksolve_pack_topo_u
topo? 1 1 ksolve_pack_topo_nodes_u
topo? 2 0 ksolve_pack_topo_f
topo? 2 1 ksolve_pack_topo_nodes_f
topo? 3 0 ksolve_pack_topo_p
topo? 3 1 ksolve_pack_topo_nodes_p
many? 0 0 ksolve_pack_topo_many
many? 0 1 ksolve_pack_topo_nodes_many
many? 1 0 ksolve_pack_topo_many_u
many? 1 1 ksolve_pack_topo_nodes_many_u
many? 2 0 ksolve_pack_topo_many_f
many? 2 1 ksolve_pack_topo_nodes_many_f
many? 3 0 -
many? 3 1 -
cold? 0 0 1 ksolve_test_fast_cold_g0r1
cold? 0 0 4 ksolve_test_fast_cold_g0r4
cold? 0 1 1 ksolve_test_fast_cold_g1r1
cold? 0 1 4 -
cold? 0 2 1 -
cold? 0 2 4 -
cold? 1 0 1 ksolve_test_fast_cold_u_g0r1
cold? 1 0 4 ksolve_test_fast_cold_u_g0r4
cold? 1 1 1 -
cold? 1 1 4 -
cold? 1 2 1 -
cold? 1 2 4 ksolve_test_fast_cold_u_g2r4
cold? 2 0 1 ksolve_test_fast_cold_p_g0r1
cold? 2 0 4 ksolve_test_fast_cold_p_g0r4
cold? 2 1 1 -
cold? 2 1 4 -
cold? 2 2 1 -
cold? 2 2 4 -
"""

PROGRAM = r"""
#include <cstdio>
#include "pack_flavours.h"
using namespace ks;
static const char* name(const PackFastRow* r) { return r ? r->kernel : "-"; }
static const char* name(const PackTopoRow* r) { return r ? r->kernel : "-"; }
int main() {
  for (const PackFastRow& r : kPackFastRows) printf("fast %s %d %d %d\n", r.kernel, (int)r.flavour, r.plan, r.rows);
  for (const PackTopoRow& r : kPackTopoRows) printf("topo %s %d %d\n", r.kernel, (int)r.flavour, (int)r.nodes);
  for (const PackTopoRow& r : kPackTopoManyRows) printf("many %s %d %d\n", r.kernel, (int)r.flavour, (int)r.nodes);
  for (const PackFastRow& r : kFastColdRows) printf("cold %s %d %d %d\n", r.kernel, (int)r.flavour, r.plan, r.rows);
  for (int f = 0; f < kFastFlavours; ++f) printf("fast-traits %d %d %d\n", f, (int)flavour_us((FastFlavour)f), (int)flavour_po((FastFlavour)f));
  for (int f = 0; f < kTopoFlavours; ++f) printf("topo-traits %d %d %d %d\n", f, (int)flavour_us((TopoFlavour)f), (int)flavour_fs((TopoFlavour)f), (int)flavour_po((TopoFlavour)f));
  printf("many-flavours %d\n", kTopoManyFlavours);
  const int rows[2] = {1, 4};
  for (int f = 0; f < kFastFlavours; ++f) for (int p = 0; p < 3; ++p) for (int r : rows) printf("fast? %d %d %d %s\n", f, p, r, name(pack_fast_row((FastFlavour)f, p, r)));
  for (int f = 0; f < kTopoFlavours; ++f) for (int n = 0; n < 2; ++n) printf("topo? %d %d %s\n", f, n, name(pack_topo_row((TopoFlavour)f, n != 0)));
  for (int f = 0; f < kTopoFlavours; ++f) for (int n = 0; n < 2; ++n) printf("many? %d %d %s\n", f, n, name(pack_topo_many_row((TopoFlavour)f, n != 0)));
  for (int f = 0; f < kFastFlavours; ++f) for (int p = 0; p < 3; ++p) for (int r : rows) printf("cold? %d %d %d %s\n", f, p, r, name(fast_cold_row((FastFlavour)f, p, r)));
  // the flavour a work record asks for: each switch implies the ones before it
  struct Work { int unsched; const void* filt; const void* podops; };
  const int one = 1;
  const Work works[4] = {{0, nullptr, nullptr}, {1, nullptr, nullptr}, {1, &one, nullptr}, {1, &one, &one}};
  for (const Work& w : works) printf("work %d %d\n", (int)fast_flavour(w), (int)topo_flavour(w));
}
"""
WORKS = ["work 0 0", "work 1 1", "work 1 2", "work 2 3"]   # (the cursor engine has no node filters: a spread handle's `filt` leaves it at its flavour)


def test_rows_and_lookups_of_the_kernel_table(tmp_path):
    """Plain C++ that g++ compiles without HIP, as engine_setting.h is."""
    src, exe = tmp_path / "table.cpp", tmp_path / "table"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "karpenter_amd", "csrc"), "-o", str(exe), str(src)])
    assert subprocess.check_output([str(exe)], text=True).splitlines() == (ROWS + TRAITS_AND_LOOKUPS).splitlines() + WORKS


SOURCES = {"ksolve_pack_fast.hip": "fast", "ksolve_pack_topo.hip": "topo", "ksolve_pack_topo_many.hip": "many"}


def rows_of_job(source, defines):
    """The table's rows a compile job defines: those of its family and -DKS_PACK_FLAVOUR, of one nodes selector under -DKS_PACK_NODES."""
    d = dict(x.removeprefix("-D").split("=") for x in defines)
    assert set(d) <= {"KS_PACK_FLAVOUR", "KS_PACK_NODES"} and "KS_PACK_FLAVOUR" in d, (source, defines)
    rows = [r.split() for r in ROWS.splitlines() if r.split()[0] == SOURCES[source] and r.split()[2] == d["KS_PACK_FLAVOUR"]]
    return [r[1] for r in rows if "KS_PACK_NODES" not in d or r[3] == d["KS_PACK_NODES"]]


def test_compile_jobs_cover_the_table_once():
    import __graft_entry__ as ge
    product = ge.compile_jobs(ge.KSOLVE_UNITS)
    test_build = ge.compile_jobs(ge.KSOLVE_UNITS + ge.TEST_HOOK_UNITS)
    assert len({name for _, _, name, _ in test_build}) == len(test_build)            # an object per (source, defines)
    defined = []
    for source, defines, _, codegen in product:
        if source in SOURCES:
            got = rows_of_job(source, defines)
            assert got, (source, defines)
            defined += got
            assert codegen[-2:] == ["-mllvm", "-amdgpu-sched-strategy=max-ilp"], (source, codegen)   # (without it: a measured 1 % on these kernels)
        else:
            assert not defines, (source, defines)
    want = [r.split()[1] for r in ROWS.splitlines() if r.split()[0] != "cold"]
    assert sorted(defined) == sorted(want) and len(set(defined)) == len(defined)
    # today's partition of kernels into objects: the plain single-problem spread kernels an object each, two kernels in every other one
    assert sorted(len(rows_of_job(s, d)) for s, d, _, _ in product if s == "ksolve_pack_topo.hip") == [1, 1, 2, 2, 2]
    # the test hooks' unit, which defines the "cold" rows, is in the test build alone
    assert [s for s, _, _, _ in test_build if s not in [p[0] for p in product]] == ["ksolve_test_fast_cold.hip"]
    assert all(os.path.exists(os.path.join(ROOT, "karpenter_amd", "csrc", s)) for s, _, _, _ in test_build)


# ---- which kernel a handle launches, on the emulation: the name the device backend would launch, from the same lookup ----

@pytest.mark.parametrize("case", kc.lone_cases(), ids=lambda c: c[0])
def test_kernel_of_a_lone_solve(oracle, emu, case):
    kc.check_lone(oracle, emu, case)


def test_kernels_of_the_flavour_members_alone(oracle, emu):
    kc.check_flavour_members_alone(oracle, emu)


def test_kernels_of_the_flavour_members_in_one_call(oracle, emu):
    kc.check_flavour_members_many(oracle, emu)
