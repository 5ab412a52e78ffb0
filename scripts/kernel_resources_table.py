"""Every kernel of one or two built device libraries, from the code objects' notes, symbol tables and .text sections: bytes of the
kernel function | VGPRs | SGPRs | VGPR spills | SGPR spills | scratch bytes | static LDS bytes | sha1 of the function's bytes (12 digits).
With two libraries (parent, this commit) the rows stand side by side with a verdict. scripts/kernel_resources.sh gives the register
columns alone.
usage: python3 scripts/kernel_resources_table.py PARENT.so [THIS.so]"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
NOTE_KEYS = (".vgpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def kernels_of(so):
    """{kernel: "bytes vgpr sgpr vspill sspill scratch lds sha1"} over every offload bundle of the library (one per translation unit)."""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, "fat.bin")
        run(f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", so, os.path.join(tmp, "copy.so"))
        data = open(fat, "rb").read()
        magic = b"__CLANG_OFFLOAD_BUNDLE__"
        starts = [m.start() for m in re.finditer(re.escape(magic), data)]
        for n, a in enumerate(starts):
            bundle, co, text = (os.path.join(tmp, f"b{n}.{e}") for e in ("bin", "co", "text"))
            open(bundle, "wb").write(data[a:starts[n + 1] if n + 1 < len(starts) else len(data)])
            subprocess.run([f"{LLVM}/clang-offload-bundler", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={bundle}", f"--output={co}", "--unbundle"],
                           check=True, capture_output=True)
            if not os.path.exists(co) or not os.path.getsize(co):
                continue
            notes = {}
            for block in run(f"{LLVM}/llvm-readelf", "--notes", co).split("- .agpr_count")[1:]:
                name = re.search(r"\.name:\s+(\S+)", block).group(1)
                notes[name] = [int(re.search(re.escape(k) + r":\s+(\d+)", block).group(1)) for k in NOTE_KEYS]
            sec = re.search(r"\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)", run(f"{LLVM}/llvm-readelf", "-S", co))
            text_addr = int(sec.group(1), 16)
            run(f"{LLVM}/llvm-objcopy", f"--dump-section=.text={text}", co, os.path.join(tmp, "copy.co"))
            code = open(text, "rb").read()
            for line in run(f"{LLVM}/llvm-readelf", "-sW", co).splitlines():
                f = line.split()
                if len(f) == 8 and f[3] == "FUNC" and f[7] in notes:
                    addr, size = int(f[1], 16), int(f[2])
                    sha = hashlib.sha1(code[addr - text_addr:addr - text_addr + size]).hexdigest()[:12]
                    out[f[7]] = " ".join(map(str, [size] + notes[f[7]] + [sha]))
    return out


def short(name):
    """ksolve_pack_topo for _Z16ksolve_pack_topoPKN2ks8TopoArgsE; a template's kernel keeps its mangled name, a library's (rocprim's,
    kilobytes of it) the head of it and a digest of the whole."""
    m = re.match(r"_Z(\d+)", name)
    if m and not name[m.end() + int(m.group(1)):].startswith("I"):
        return name[m.end():m.end() + int(m.group(1))]
    return name if len(name) <= 80 else name[:60] + "~" + hashlib.sha1(name.encode()).hexdigest()[:8]


def main():
    tables = [kernels_of(p) for p in sys.argv[1:3]]
    names = sorted(set().union(*tables), key=lambda n: (len(n), n))
    if len(tables) == 1:
        for n in names:
            print(f"{short(n)} | {tables[0][n]}")
        return
    print("kernel | parent | this commit | same")
    for n in names:
        a, b = tables[0].get(n, "-"), tables[1].get(n, "-")
        same = "yes" if a == b else "new" if a == "-" else "gone" if b == "-" else "registers" if a.split()[1:7] == b.split()[1:7] else "NO"
        print(f"{short(n)} | {a} | {b} | {same}")


if __name__ == "__main__":
    main()
