#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds of the library: tools/cmp_device_code.py A.so B.so

For a change that touches host code only.  From each library the .hip_fatbin section is taken and its gfx950 code
object unbundled; then, keyed by symbol name, the disassembly of every function and, keyed by kernel name, every entry of
the AMDGPU metadata note (registers, LDS, scratch, arguments) are compared.  The code objects as files may differ: where
a template is first instantiated orders .text, so PC-relative literals are compared by the symbol they reach and the
alignment padding behind a function's last instruction is left out.  Needs no GPU.  Exit status 0: same names, every body and entry equal.
"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def run(*cmd):
    return subprocess.run(cmd, check=True, stdout=subprocess.PIPE, universal_newlines=True).stdout


def code_object(lib, tmp):
    fat, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, os.path.basename(lib) + ".co")
    run(os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, fat)
    run(os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + fat, "--output=" + co)
    return co


def symbols(co):
    """(sorted [(address, name)] of the functions and objects, {address of a GOT slot: name})"""
    syms, got = [], {}
    for line in run(os.path.join(LLVM, "llvm-objdump"), "-t", co).splitlines():
        f = line.split()
        if len(f) >= 5 and f[-3] in (".text", ".rodata", ".bss", ".data") and ("F" in f[1:4] or "O" in f[1:4]):
            syms.append((int(f[0], 16), f[-1]))
    for line in run(os.path.join(LLVM, "llvm-readelf"), "-r", co).splitlines():
        f = line.split()
        if len(f) >= 5 and f[2].startswith("R_AMDGPU_"):
            got[int(f[0], 16)] = f[4]
    return sorted(syms), got


def functions(co):
    """{symbol: [instruction, ...]}; the literal of a PC-relative address (s_getpc_b64, then s_add_u32 with a 32-bit literal)
    is replaced by the symbol it reaches: the functions of two builds may lie in another order."""
    syms, got = symbols(co)

    def resolve(addr):
        if addr in got:
            return "got:" + got[addr]
        below = [(a, n) for a, n in syms if a <= addr]
        return "%s+0x%x" % (below[-1][1], addr - below[-1][0]) if below else "0x%x" % addr

    out, name, pc = {}, None, None
    for line in run(os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co).splitlines():
        m = re.match(r"^<(.+)>:$", line.strip())
        if m:
            name, pc = m.group(1), None
            out[name] = []
            continue
        if not name or not line.strip():
            continue
        ins, _, tail = line.partition("//")
        ins = ins.strip()
        m = re.match(r"^s_add_u32 (\S+), (\S+), 0x([0-9a-f]+)$", ins)
        if pc is not None and m:
            lit = int(m.group(3), 16)
            ins = "s_add_u32 %s, %s, <%s>" % (m.group(1), m.group(2), resolve(pc + 4 + (lit - (1 << 32) if lit >> 31 else lit)))
        pc = int(tail.split(":")[0], 16) if ins.startswith("s_getpc_b64") else None
        out[name].append(ins)
    padded = 0
    for body in out.values():                          # the padding behind a function's last instruction up to the next
        n = len(body)                                  # function's alignment: layout, not code
        while body and body[-1] in ("s_nop 0", "..."):
            body.pop()
        padded += len(body) < n
    print("    %s: trailing padding (s_nop 0 / ...) left out of %d of %d bodies" % (os.path.basename(co), padded, len(out)))
    return out


def kernels(co):
    out, name, cur = {}, None, []
    for line in run(os.path.join(LLVM, "llvm-readelf"), "--notes", co).splitlines():
        if re.match(r"^\s*- \.agpr_count:|^\s*- \.args:", line) and cur:          # a new entry of amdhsa.kernels
            if name:
                out[name] = cur
            name, cur = None, []
        m = re.match(r"^\s*\.name:\s+(\S+)$", line)
        if m and line.startswith("    .name"):
            name = m.group(1)
        cur.append(line.rstrip())
        if line.startswith("amdhsa.target"):
            break
    if name:
        out[name] = cur
    return out


def compare(what, a, b):
    bad = sorted(set(a) ^ set(b)) + sorted(k for k in set(a) & set(b) if a[k] != b[k])
    print("%s: %d / %d, %d differ" % (what, len(a), len(b), len(bad)))
    for k in bad[:20]:
        print("   ", k, "(only in one)" if (k in a) != (k in b) else "(differs)")
    return not bad


def main():
    with tempfile.TemporaryDirectory() as tmp:
        ca, cb = code_object(sys.argv[1], tmp), code_object(sys.argv[2], tmp)
        fa, fb = functions(ca), functions(cb)
        ok = compare("symbols", fa, fb)
        ok = compare("kernel metadata entries", kernels(ca), kernels(cb)) and ok
        for k in ("ndt_align_kernel", "fitness_points_kernel", "fitness_far_kernel", "fitness_reduce_kernel", "ndt_eval_kernel", "ndt_order_kernel"):
            print("    %-24s %d / %d instances" % (k, sum(k in n and not n.endswith(".kd") for n in fa), sum(k in n and not n.endswith(".kd") for n in fb)))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
