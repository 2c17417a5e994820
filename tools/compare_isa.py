#!/usr/bin/env python3
"""Compare the gfx950 device code of the convolution sources between a git revision and the working tree (no GPU needed).

    python tools/compare_isa.py [BASE_REV] [file ...]         # default: HEAD, the seven convolution files

Each file is compiled to assembly at both states with the flags of build_native.py plus `--cuda-device-only -S`; lines that
contain `__hip_cuid_` (a hash of the source text) are dropped.  Prints per file `identical`, or the kernels whose text differs.
A one-off check for refactors that must not change the machine code; not a test.
"""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = ["conv_split", "conv1x1_split", "wgrad_split", "wgrad1x1_split", "conv_strided", "conv_mfma", "conv_wgrad"]


def asm(root, name, out):
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics", "-I", os.path.join(root, "include"),
           "-I", os.path.join(root, "consistent_depth_amd", "csrc"), "--cuda-device-only", "-S", "-o", out,
           os.path.join(root, "consistent_depth_amd", "csrc", name + ".hip")]
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
    with open(out) as f:
        return [l for l in f if "__hip_cuid_" not in l]


def functions(lines):
    """{symbol: text} of every function body; the rest (metadata, data) under the key ''."""
    out, cur = {"": []}, ""
    for l in lines:
        m = re.match(r"^(\w+):\s+; @\1", l)
        if m:
            cur = m.group(1)
            out[cur] = []
        out[cur].append(l)
        if cur and l.startswith(".Lfunc_end"):
            cur = ""
    return out


def main():
    args = sys.argv[1:]
    base = args[0] if args else "HEAD"
    files = args[1:] or FILES
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(["git", "-C", REPO, "archive", base, "include", "consistent_depth_amd/csrc"], check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
        with ThreadPoolExecutor(8) as ex:
            jobs = {f: (ex.submit(asm, tmp, f, os.path.join(tmp, f + ".base.s")), ex.submit(asm, REPO, f, os.path.join(tmp, f + ".new.s"))) for f in files}
            for f in files:
                a, b = (functions(j.result()) for j in jobs[f])
                diff = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
                if not diff:
                    print(f"{f}.hip: identical ({len(a) - 1} functions)")
                    continue
                funcs = [k for k in diff if k]
                names = subprocess.run(["c++filt"] + funcs, capture_output=True, text=True).stdout.split("\n") if funcs else []
                print(f"{f}.hip: DIFFERS in {len(funcs)} of {len(a) - 1} functions" + (" and in the metadata / data sections" if "" in diff else ""))
                for n in names:
                    if n:
                        print("    " + re.sub(r"\(.*", "", n).replace("void ", ""))


if __name__ == "__main__":
    main()
