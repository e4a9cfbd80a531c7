"""Which kernels of a .hip file compile to other device code than at a git revision (no GPU needed):
python tools/kernel_asm_diff.py REV query.hip [marshal.hip ...] [-DSJ_DEBUG_BOUNDS] ['OLD=NEW' ...]

Both trees -- the working tree and `git archive REV` in a temporary directory -- are compiled with hipcc -S --cuda-device-only for
gfx950, and the body of every kernel (its label up to s_endpgm) is compared line by line.  Prints one line per kernel that
differs, with the number of assembly lines and of v_writelane (scalar state kept in vector lanes) on either side, and the count of
identical ones.  A kernel that is identical here runs the revision's instructions: its speed needs no new measurement.

OLD=NEW: the revision's kernel OLD is compared with the working tree's kernel NEW -- a renamed kernel, or the instantiation of a
template that replaces it -- instead of being listed as removed and added.  Both are the demangled names without namespaces and
arguments, e.g. 'k_q_order_hist=k_q_sort_hist<unsigned long>'; every pair is printed with its verdict.  Comments, the numbers of the
basic block labels (they count the functions in front) and a kernel's own mangled name inside its body are not compared, so the
line counts are those of instructions, labels and directives."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CS = os.path.join("simdjson-go_amd", "csrc")


def short(mangled):
    """the demangled name without `void`, namespaces and the argument list"""
    name = subprocess.run(["c++filt", mangled], capture_output=True, text=True).stdout.strip()
    name = name.replace("(anonymous namespace)::", "").replace("sj::", "").replace("void ", "")
    depth = 0
    for i, ch in enumerate(name):
        depth += (ch == "<") - (ch == ">")
        if ch == "(" and depth == 0:
            return name[:i]
    return name


def kernels(tree, src, flags, out):
    """{short name: body} of the kernels of one file"""
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S",
                    "--cuda-device-only", *flags, "-o", out, os.path.join(tree, CS, src)], check=True, stderr=subprocess.DEVNULL)
    text = open(out).read()
    found = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\s*s_endpgm", text, re.S | re.M):
        name = short(m.group(1))
        assert name not in found, name
        body = re.sub(r"[ \t]*;[^\n]*", "", m.group(2).replace(m.group(1), "SELF"))
        found[name] = "\n".join(line for line in re.sub(r"\.LBB\d+_", ".LBB_", body).splitlines() if line.strip())
    return found


def main():
    rev, args = sys.argv[1], sys.argv[2:]
    flags = [a for a in args if a.startswith("-")]
    pairs = dict(a.split("=", 1) for a in args if "=" in a and not a.startswith("-"))
    with tempfile.TemporaryDirectory() as tmp:
        old = os.path.join(tmp, "old")
        os.mkdir(old)
        tar = subprocess.run(["git", "-C", ROOT, "archive", rev, "simdjson-go_amd/csrc", "include"], check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", old], input=tar, check=True)
        for src in (a for a in args if not a.startswith("-") and "=" not in a):
            a = kernels(old, src, flags, os.path.join(tmp, "a.s"))
            b = kernels(ROOT, src, flags, os.path.join(tmp, "b.s"))
            renamed = {o: n for o, n in pairs.items() if o in a and n in b}
            names = sorted((set(a) | set(b)) - set(renamed) - set(renamed.values()))
            same = [k for k in names if a.get(k) == b.get(k)]
            print(f"{src}{' ' + ' '.join(flags) if flags else ''}: {len(same)} of {len(names)} kernels of one name identical to {rev}")

            def differs(label, x, y):
                print(f"  differs    {label[:100]:<100s} lines {len(x.splitlines())} -> {len(y.splitlines())}, "
                      f"v_writelane {x.count('v_writelane')} -> {y.count('v_writelane')}")
            for k in names:
                if k not in same:
                    differs(k + ("" if k in a and k in b else "  (removed)" if k in a else "  (added)"), a.get(k, ""), b.get(k, ""))
            for o, n in sorted(renamed.items()):
                if a[o] == b[n]:
                    print(f"  identical  {o} -> {n}")
                else:
                    differs(f"{o} -> {n}", a[o], b[n])


if __name__ == "__main__":
    main()
