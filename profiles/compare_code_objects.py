"""Are the kernels of two builds the same instructions?  Compares, symbol by symbol, the gfx950 code objects of two trees:

    python profiles/compare_code_objects.py OLD_TREE NEW_TREE [WORKDIR]

For each tree and each arm (tinsel_hip.hip under the parity flags, tinsel_fast.hip under the tolerance flags of tinsel_amd/build.py) it
compiles the device side alone (hipcc --cuda-device-only), unbundles the gfx950 ELF, and compares every function of OLD with its namesake
in NEW: first the symbol's bytes, then -- where they differ -- the disassembly with the literals of `s_add_u32 / s_addc_u32` that follow an
`s_getpc_b64` masked (the pc-relative address of a constant table, which moves when code is added in front of it).  Prints per arm:
functions in OLD, byte-identical, identical but for such literals, changed otherwise (listed), removed (listed), added (listed).
"""
import hashlib
import os
import re
import subprocess
import sys

LLVM = "/opt/rocm/llvm/bin"
COMMON = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-slp-vectorize", "-Wno-unused-function", "-Wno-unused-variable", "--cuda-device-only"]
ARMS = {"parity": ("tinsel_hip.hip", ["-ffp-contract=off", "-fno-fast-math"]),
        "fast": ("tinsel_fast.hip", ["-DTN_FAST=1", "-ffp-contract=fast", "-fno-hip-fp32-correctly-rounded-divide-sqrt", "-freciprocal-math",
                                     "-fgpu-flush-denormals-to-zero"])}


def build(tree, arm, work, tag):
    src, flags = ARMS[arm]
    co, elf = os.path.join(work, "%s_%s.co" % (tag, arm)), os.path.join(work, "%s_%s.elf" % (tag, arm))
    subprocess.run(["hipcc"] + COMMON + flags + ["-c", os.path.join(tree, "tinsel_amd", "csrc", src), "-o", co], check=True)
    subprocess.run([LLVM + "/clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + co,
                    "--output=" + elf], check=True)
    return elf


def symbol_bytes(elf):
    secs = subprocess.run([LLVM + "/llvm-readelf", "-SW", elf], capture_output=True, text=True, check=True).stdout
    index = None
    for line in secs.splitlines():
        p = line.replace("[", " ").replace("]", " ").split()
        if len(p) > 5 and p[1] == ".text":
            index, addr, off = p[0], int(p[3], 16), int(p[4], 16)
    if index is None:
        raise RuntimeError("%s: no .text section (not a gfx950 code object?)" % elf)
    data = open(elf, "rb").read()
    out = {}
    for line in subprocess.run([LLVM + "/llvm-readelf", "-sW", elf], capture_output=True, text=True, check=True).stdout.splitlines():
        p = line.split()
        if len(p) >= 8 and p[3] == "FUNC" and p[6] == index:
            a, size = int(p[1], 16), int(p[2])
            out[p[7]] = hashlib.sha256(data[a - addr + off:a - addr + off + size]).hexdigest()
    return out


def disassembly(elf):
    text = subprocess.run([LLVM + "/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", elf], capture_output=True, text=True, check=True).stdout
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]* ?<(.+)>:$", line.strip())
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line.strip():
            cur.append(re.sub(r"\s*//.*$", "", line.strip()))
    return out


def only_pc_literals(a, b):
    if len(a) != len(b):
        return False
    mask = lambda s: re.sub(r"0x[0-9a-f]+$|-?\d+$", "L", s)
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y and not (x.split()[0] == y.split()[0] and x.split()[0] in ("s_add_u32", "s_addc_u32") and mask(x) == mask(y) and
                           any("s_getpc_b64" in p for p in a[max(0, i - 3):i])):
            return False
    return True


def main(argv):
    old, new = argv[1], argv[2]
    work = argv[3] if len(argv) > 3 else "."
    for arm in ARMS:
        eo, en = build(old, arm, work, "old"), build(new, arm, work, "new")
        so, sn = symbol_bytes(eo), symbol_bytes(en)
        differ = [k for k in so if k in sn and so[k] != sn[k]]
        do, dn = disassembly(eo), disassembly(en)
        other = [k for k in differ if not only_pc_literals(do.get(k, []), dn.get(k, [None]))]
        print("%s arm: %d functions in OLD, %d byte-identical in NEW, %d identical but for pc-relative literals, %d changed otherwise, %d removed, %d added" % (
            arm, len(so), len(so) - len(differ) - len(set(so) - set(sn)), len(differ) - len(other), len(other), len(set(so) - set(sn)), len(set(sn) - set(so))))
        for k in other:
            print("  CHANGED", k)
        for k in sorted(set(so) - set(sn)):
            print("  REMOVED", k)
        for k in sorted(set(sn) - set(so)):
            print("  added  ", k)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
