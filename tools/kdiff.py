#!/usr/bin/env python3
"""Which kernels of two builds of the library differ: tools/kdiff.py OLD.so NEW.so [name-substring]
Disassembles the gfx950 code objects of both (as tools/kres.py finds them), compares every kernel's instruction
stream (mnemonics and operands; addresses, pc-relative literals and s_nop dropped) and prints, for the kernels whose code changed, the opcode counts
that moved.  The last line counts the kernels whose device code is identical."""
import collections
import os
import re
import subprocess
import sys
import tempfile

from kres import code_objects

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


def kernels(lib):
    out = {}
    for co in code_objects(lib):
        with tempfile.NamedTemporaryFile(suffix=".co", delete=False) as f:
            f.write(co)
        txt = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", f.name], capture_output=True, text=True).stdout
        os.unlink(f.name)
        name = None
        for line in txt.splitlines():
            m = re.match(r"^[0-9a-f]+ <(\w+)>:", line)
            if m:
                name = m.group(1)
                out[name] = []
                continue
            t = line.split("//")[0].strip()
            if name and t and t != "..." and not t.startswith("s_nop") and not t.startswith("s_code_end"):    # "...": elided padding
                t = re.sub(r"\s+", " ", t)
                if t.startswith(("s_add_u32", "s_addc_u32")):    # pc-relative offsets of constant tables move with the object
                    t = re.sub(r"0x[0-9a-f]+$", "PCREL", t)
                out[name].append(t)
    return out


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    pat = sys.argv[3] if len(sys.argv) > 3 else ""
    same = 0
    for k in sorted(set(old) | set(new)):
        dem = subprocess.run(["c++filt", k], capture_output=True, text=True).stdout.strip()
        dem = re.sub(r"^void \(anonymous namespace\)::", "", dem).split("(")[0]
        if pat not in dem:
            continue
        if old.get(k) == new.get(k):
            same += 1
            continue
        a = collections.Counter(i.split()[0] for i in old.get(k, []))
        b = collections.Counter(i.split()[0] for i in new.get(k, []))
        valu = lambda c: sum(n for o, n in c.items() if o.startswith("v_"))
        lds = lambda c: sum(n for o, n in c.items() if o.startswith("ds_"))
        d = sorted(((b[o] - a[o], o) for o in set(a) | set(b) if b[o] != a[o]), key=lambda t: -abs(t[0]))[:8]
        print("%-52s VALU %5d -> %5d (%+d)  LDS %4d -> %4d | %s" % (dem, valu(a), valu(b), valu(b) - valu(a), lds(a), lds(b),
                                                                   ", ".join("%s %+d" % (o, n) for n, o in d)))
    print("%d kernels identical" % same)


if __name__ == "__main__":
    main()
