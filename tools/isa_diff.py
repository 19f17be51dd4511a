#!/usr/bin/env python3
"""Kernel-by-kernel comparison of the gfx950 device code of two .o / .so files: for every kernel whose demangled name matches the regex,
whether the instruction text (addresses and encodings stripped) is identical in both, plus the counts a loop change is judged by -
MFMAs, VALU instructions between the first and the last MFMA, s_waitcnt, LDS reads / writes, v_exp.

    python tools/isa_diff.py parent/sepr_attention.o sepreformer_amd/_native/sepr_attention.o 'relattn_x3p?_kernel'
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

OBJDUMP = os.environ.get("LLVM_OBJDUMP") or shutil.which("llvm-objdump") or "/opt/rocm/lib/llvm/bin/llvm-objdump"


def kernels(path, pattern):
    """{demangled name: [instruction text]} of the kernels in `path` that match `pattern`."""
    pat, out = re.compile(pattern), {}
    with tempfile.TemporaryDirectory() as tmp:
        base = os.path.join(tmp, os.path.basename(path))
        shutil.copy(path, base)
        subprocess.run([OBJDUMP, "--offloading", base], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=False)
        for o in sorted(f for f in (os.path.join(tmp, n) for n in os.listdir(tmp)) if f.startswith(base + ".") and "amdgcn" in f):
            dis = subprocess.run([OBJDUMP, "-d", "--demangle", o], stdout=subprocess.PIPE, text=True, check=True).stdout
            cur = None
            for line in dis.splitlines():
                if line.endswith(">:"):
                    name = line.split("<", 1)[1][:-2]
                    cur = out.setdefault(name, []) if pat.search(name) else None
                elif cur is not None and line.startswith("\t"):
                    if line.strip() == "...":       # objdump's elision of the zero padding behind a kernel: layout, not an instruction
                        continue
                    cur.append(line.split("//")[0].strip())
    return out


def stats(ins):
    mf = [k for k, t in enumerate(ins) if t.startswith("v_mfma")]
    inner = ins[mf[0]:mf[-1] + 1] if mf else []
    n = lambda seq, pre: sum(1 for t in seq if t.startswith(pre))   # noqa: E731
    return {"instr": len(ins), "mfma": len(mf), "valu_in_loop": n(inner, "v_") - n(inner, "v_mfma"), "v_exp": n(ins, "v_exp"),
            "s_waitcnt": n(ins, "s_waitcnt"), "lgkmcnt_waits": sum(1 for t in ins if t.startswith("s_waitcnt") and "lgkmcnt" in t),
            "ds_read": n(ins, "ds_read"), "ds_write": n(ins, "ds_write")}


def main(argv):
    a, b = kernels(argv[0], argv[2]), kernels(argv[1], argv[2])
    differ = 0
    for name in sorted(set(a) | set(b)):
        if name in a and name in b:
            same = a[name] == b[name]
            differ += not same
            print(f"{'IDENTICAL' if same else 'DIFFERENT'}  {name}")
        else:
            print(f"{'only in ' + os.path.basename(argv[0 if name in a else 1]) + ' (' + ('first' if name in a else 'second') + ')'}  {name}")
        for tag, k in (("first ", a), ("second", b)):
            if name in k:
                print(f"    {tag} " + " ".join(f"{key} {val}" for key, val in stats(k[name]).items()))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
