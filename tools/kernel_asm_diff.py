"""Which kernels of a .hip file compile to other device code than at a git revision (no GPU needed):
python tools/kernel_asm_diff.py REV query.hip [marshal.hip ...] [-DSJ_DEBUG_BOUNDS]

Both trees -- the working tree and `git archive REV` in a temporary directory -- are compiled with hipcc -S --cuda-device-only for
gfx950, and the body of every kernel (its label up to s_endpgm) is compared line by line.  Prints one line per kernel that
differs, with the number of assembly lines and of v_writelane (scalar state kept in vector lanes) on either side, and the count of
identical ones.  A kernel that is identical here runs the revision's instructions: its speed needs no new measurement."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CS = os.path.join("simdjson-go_amd", "csrc")


def kernels(tree, src, flags, out):
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S",
                    "--cuda-device-only", *flags, "-o", out, os.path.join(tree, CS, src)], check=True, stderr=subprocess.DEVNULL)
    text = open(out).read()
    return {m.group(1): m.group(2) for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\s*s_endpgm", text, re.S | re.M)}


def main():
    rev, args = sys.argv[1], sys.argv[2:]
    flags = [a for a in args if a.startswith("-")]
    with tempfile.TemporaryDirectory() as tmp:
        old = os.path.join(tmp, "old")
        os.mkdir(old)
        tar = subprocess.run(["git", "-C", ROOT, "archive", rev, "simdjson-go_amd/csrc", "include"], check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", old], input=tar, check=True)
        for src in (a for a in args if not a.startswith("-")):
            a = kernels(old, src, flags, os.path.join(tmp, "a.s"))
            b = kernels(ROOT, src, flags, os.path.join(tmp, "b.s"))
            names = sorted(set(a) | set(b))
            same = [k for k in names if a.get(k) == b.get(k)]
            print(f"{src}: {len(same)} of {len(names)} kernels identical to {rev}")
            for k in names:
                if k in same:
                    continue
                x, y = a.get(k, ""), b.get(k, "")
                name = subprocess.run(["c++filt", k], capture_output=True, text=True).stdout.strip().replace("(anonymous namespace)::", "")
                print(f"  differs  {name[:90]:<90s} lines {len(x.splitlines())} -> {len(y.splitlines())}, "
                      f"v_writelane {x.count('v_writelane')} -> {y.count('v_writelane')}")


if __name__ == "__main__":
    main()
