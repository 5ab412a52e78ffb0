#!/usr/bin/env python3
"""Records the member names of the reference's scheduling types that go/ksolve_*.go select on, as a JSON list of names
(tests/golden/reference_members.json), so that tests/test_abi.py::test_go_binding_uses_only_members_the_reference_declares
runs without a checkout of the reference.

    python tests/golden/make_reference_members.py <karpenter checkout>

Sources (under the checkout):
  pkg/controllers/provisioning/scheduling/*.go   struct fields, embedded types and methods of the types below
  pkg/scheduling/*.go                            HostPortUsage / VolumeUsage: the fields and methods the binding's accessors meet
The Go source is only read as data (regex over `type T struct {...}` blocks and `func (r *T) Name(` lines); no reference code is
copied into the repository.
"""
import glob
import json
import os
import re
import sys

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_members.json")
CONTROLLER_TYPES = ("Scheduler", "Topology", "PodData", "ExistingNode", "NodeClaim", "TopologyGroup")
PKG_TYPES = ("HostPortUsage", "VolumeUsage")


def sources(directory):
    return [open(f).read() for f in sorted(glob.glob(os.path.join(directory, "*.go"))) if not f.endswith("_test.go")]


def struct_fields(srcs, type_name):
    """Field names and embedded type names of `type <type_name> struct {...}`."""
    out = set()
    for t in srcs:
        m = re.search(r"type %s struct \{(.*?)\n\}" % type_name, t, re.S)
        if m:
            for line in m.group(1).split("\n"):
                mm = re.match(r"\t(\*?[\w.]+)(\s|$)", line)
                if mm and not line.strip().startswith("//"):
                    out.add(mm.group(1).lstrip("*").split(".")[-1])
    return out


def methods(srcs, type_name):
    return {name for t in srcs for name in re.findall(r"func \(\w+ \*?%s\) (\w+)\(" % type_name, t)}


def main(ref):
    ctrl = sources(os.path.join(ref, "pkg", "controllers", "provisioning", "scheduling"))
    pkg = sources(os.path.join(ref, "pkg", "scheduling"))
    doc = {"source": "kubernetes-sigs/karpenter: pkg/controllers/provisioning/scheduling and pkg/scheduling (non-test .go files)",
           "members": {t: sorted(struct_fields(ctrl, t) | methods(ctrl, t)) for t in CONTROLLER_TYPES},
           "pkg_scheduling": {t: {"fields": sorted(struct_fields(pkg, t)), "methods": sorted(methods(pkg, t))} for t in PKG_TYPES}}
    for t, names in doc["members"].items():
        if not names:
            raise SystemExit(f"no members found for {t} under {ref}")
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(OUT)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
