"""Kernel-by-kernel diff of the gfx950 instruction streams of two builds of the library: the check that a refactor of the kernel sources
left the machine code alone (and, where it did not, by how much).  Extracts the gfx950 code object of each library
(kernel_resources.code_object), disassembles both with llvm-objdump and prints per kernel name either `identical` or `differs` with the
instruction counts of both sides, whether the two multisets of mnemonics are equal (a pure re-ordering / re-allocation), the number of
differing lines of a plain line diff of the instructions and of the same diff over the mnemonics alone (what is left when registers are
renamed), split at the kernel's first MFMA into set-up and the rest; then the resource tuple (vgpr+agpr, agpr, sgpr, lds, scratch) of each
side.  A plain diff: it looks for no particular instruction.  The one thing it normalises is the literal of the s_add_u32 behind an
s_getpc_b64 -- the distance to a global, which moves with the size of everything in front of it.
usage: python tools/kernel_streams.py <a.so> <b.so> [substring of the kernel name]"""
import difflib
import re
import subprocess
import sys
import tempfile
from collections import Counter

from kernel_resources import code_object, resources

LLVM = "/opt/rocm/lib/llvm/bin/"


def streams(lib):
    """({kernel name: [instruction text, ...]}, resources) of a library's gfx950 code object"""
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(code_object(lib))
        f.flush()
        txt = subprocess.run([LLVM + "llvm-objdump", "-d", "--mcpu=gfx950", "--no-show-raw-insn", f.name], capture_output=True, text=True, check=True).stdout
        res = resources(f.name)
    heads, bodies = [], []
    for blk in re.split(r"\n(?=[0-9a-f]{16} <)", txt):
        m = re.match(r"[0-9a-f]{16} <(\S+)>:", blk)
        if not m:
            continue
        heads.append(m.group(1))
        # an instruction line without its address comment; branch targets stay as the relative offsets objdump prints
        ins = [ln.split("//")[0].strip() for ln in blk.split("\n")[1:] if ln.split("//")[0].strip()]
        for i in range(1, len(ins)):
            if ins[i - 1].startswith("s_getpc_b64") and ins[i].startswith("s_add_u32"):
                ins[i] = ins[i].rsplit(",", 1)[0] + ", <pc-relative>"
        bodies.append(ins)
    names = subprocess.run(["c++filt"], input="\n".join(heads), capture_output=True, text=True).stdout.split("\n")  # (as kernel_resources names them)
    return {names[i]: bodies[i] for i in range(len(heads))}, res


def ndiff(a, b):
    return sum(1 for d in difflib.unified_diff(a, b, lineterm="", n=0) if d[:1] in "+-" and d[:3] not in ("+++", "---"))


def main():
    a, b = sys.argv[1], sys.argv[2]
    pat = sys.argv[3] if len(sys.argv) > 3 else ""
    (sa, ra), (sb, rb) = streams(a), streams(b)
    same = diff = 0
    for name in sorted(set(sa) | set(sb)):
        if pat not in name or name not in ra and name not in rb:  # (kernels only: the code object's other symbols have no resource note)
            continue
        if name not in sa or name not in sb:
            print(f"only in {'a' if name in sa else 'b'}: {name}\n    resources (vgpr+agpr, agpr, sgpr, lds, scratch): {(ra if name in sa else rb).get(name)}")
            diff += 1
            continue
        ia, ib = sa[name], sb[name]
        if ia == ib:
            verdict = "identical"
            same += 1
        else:
            ma, mb = [i.split()[0] for i in ia], [i.split()[0] for i in ib]
            fa = next((i for i, m in enumerate(ma) if m.startswith("v_mfma")), len(ma))
            fb = next((i for i, m in enumerate(mb) if m.startswith("v_mfma")), len(mb))
            verdict = (f"differs: instructions {len(ia)} -> {len(ib)}, mnemonic multiset {'equal' if Counter(ma) == Counter(mb) else 'NOT equal'}, "
                       f"{ndiff(ia, ib)} differing lines; mnemonics alone: {ndiff(ma[:fa], mb[:fb])} in the set-up ({fa} -> {fb} instructions in front of the "
                       f"first MFMA), {ndiff(ma[fa:], mb[fb:])} behind it")
            diff += 1
        print(f"{name}\n    {verdict}\n    resources (vgpr+agpr, agpr, sgpr, lds, scratch): {ra.get(name)} -> {rb.get(name)}")
    print(f"{same} kernels identical, {diff} differ")


if __name__ == "__main__":
    main()
