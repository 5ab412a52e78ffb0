"""Code length / SGPRs / VGPRs / scratch of every device FUNCTION of one translation unit, two builds side by side: the functions
whose figures differ, and whether any loop function (fast_hot_run / fast_slow_run) is among them. scripts/kernel_resources.sh gives
the per-KERNEL figures, which are maxima over a kernel's call graph; this says which function moved them.

The inputs are the device assembly of the unit, with the flags __graft_entry__.py compiles it with, from either commit:
  hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -mllvm -amdgpu-sched-strategy=max-ilp --cuda-device-only -S \
        karpenter_amd/csrc/ksolve_pack_fast.hip -o branch.s
usage: python scripts/function_resources.py parent.s branch.s"""
import re
import subprocess
import sys

FIELDS = (("code", r"; codeLenInByte = (\d+)"), ("sgpr", r"; TotalNumSgprs: (\d+)"), ("vgpr", r"; NumVgprs: (\d+)"), ("scratch", r"; ScratchSize: (\d+)"))


def functions(path):
    """{mangled name: {code, sgpr, vgpr, scratch}} from the comment block the AMDGPU backend writes behind every function."""
    out, name = {}, None
    for line in open(path, errors="replace"):
        m = re.match(r"\s*\.type\s+([\w.$]+),@function", line)
        if m:
            name = m.group(1)
            continue
        if name is None:
            continue
        for key, pat in FIELDS:
            m = re.match(pat, line)
            if m:
                out.setdefault(name, {})[key] = int(m.group(1))
    return out


def demangle(names):
    for tool in ("/opt/rocm/lib/llvm/bin/llvm-cxxfilt", "llvm-cxxfilt", "c++filt"):
        try:
            txt = subprocess.run([tool], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout
            return dict(zip(names, txt.splitlines()))
        except (OSError, subprocess.CalledProcessError):
            continue
    return {n: n for n in names}


def main():
    parent, branch = functions(sys.argv[1]), functions(sys.argv[2])
    names = sorted(set(parent) | set(branch))
    plain = demangle(names)
    short = lambda n: re.sub(r"\bks::", "", plain[n])[:110]
    differ = [n for n in names if parent.get(n) != branch.get(n)]
    loops = [n for n in names if re.search(r"fast_(hot|slow)_run", plain[n])]
    print(f"{len(names)} functions, {len(differ)} differ; loop functions (fast_hot_run / fast_slow_run): {len(loops)}, "
          f"of which differ: {len([n for n in loops if n in differ])}")
    for n in sorted(differ, key=short):
        print(short(n))
        print("    parent", parent.get(n))
        print("    branch", branch.get(n))


if __name__ == "__main__":
    main()
