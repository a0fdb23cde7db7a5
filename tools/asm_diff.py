#!/usr/bin/env python3
"""Are the device functions of this tree's kernels the machine code another revision generates?  Compiles each side's kernel units
(KERNEL_SOURCES of its own voxel_rt2_amd/build.py; a revision from before there was such a list: its SOURCES without vrt_api.hip) for the
device alone (hipcc -S, this tree's flags, a process per unit) from this tree and from REV's csrc/, include/ and build.py (git archive
into a temporary folder), cuts the listings into functions and compares every function both sides have, whichever unit holds it,
instruction for instruction: comments dropped, block labels renumbered in order of appearance (a function's labels carry its number in
the file, which moves when functions are added).  A function that two units of one side define is an error (exit status 2).

    python tools/asm_diff.py [REV] [--rename REGEX=REPL ...] [-DNAME[=VALUE] ...] [name-substring ...]         REV: default HEAD~1

-D...: both sides are compiled with these definitions too (-DVRT_DEV_KNOBS: the development build's kernels, libvrt_dev.so).

--rename: a kernel of this tree whose name changed (a template parameter added with a default, say) is paired with REV's by rewriting this
tree's demangled names with re.sub(REGEX, REPL, name) first, e.g. --rename '(k_render_pool<[^>]*), false>=\1>'.

Prints one line per function that differs or that only one side has, then the counts; exit status 1 if a function both have differs.
A function that holds the same multiset of instruction lines in another order (the scheduler swapping independent instructions) is
reported apart from one whose instructions differ; both count for the exit status."""
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from voxel_rt2_amd import build as B  # noqa: E402

CSRC = os.path.join("voxel_rt2_amd", "csrc")
MAX_PROCS = 8   # compiler processes at a time


DEFINES = []


def kernel_sources(root):
    """The units of `root` that hold device code, by root's own build.py."""
    spec = importlib.util.spec_from_file_location("_asm_diff_build", os.path.join(root, "voxel_rt2_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return list(getattr(mod, "KERNEL_SOURCES", None) or [s for s in mod.SOURCES if s != "vrt_api.hip"])


def listing(root, src, out):
    flags = [f for f in B.FLAGS if f not in ("-shared", "-fPIC")] + DEFINES
    subprocess.run([B._hipcc()] + flags + ["--offload-device-only", "-S", os.path.join(root, CSRC, src), "-o", out], check=True, capture_output=True)
    return open(out).read()


def side(root, tmp, tag, what):
    """{demangled name: [instruction lines]} over all kernel units of `root`, compiled side by side."""
    srcs = kernel_sources(root)
    with ThreadPoolExecutor(max_workers=min(len(srcs), MAX_PROCS)) as pool:
        texts = list(pool.map(lambda s: listing(root, s, os.path.join(tmp, f"{tag}_{s}.s")), srcs))
    out, home = {}, {}
    for src, text in zip(srcs, texts):
        for n, body in functions(text).items():
            if n in out:
                print(f"error: {what} defines {n[:150]} in two units, {home[n]} and {src}", file=sys.stderr)
                sys.exit(2)
            out[n], home[n] = body, src
    return out


def functions(text):
    """{demangled name: [instruction lines]} of a device listing."""
    out, cur, body = {}, None, None
    for line in text.splitlines():
        m = re.match(r"^([A-Za-z_][\w$.]*):\s*(;.*)?$", line)
        if m and cur is None and not m.group(1).startswith("."):
            cur, body = m.group(1), []
            continue
        if cur is None:
            continue
        if re.match(r"^\.Lfunc_end\d+:", line):
            out[cur] = body
            cur = None
            continue
        line = line.split(";")[0].strip()
        if line and not line.startswith((".p2align", ".loc", ".file", ".cfi", ".section", ".text")):
            body.append(line)
    names = list(out)
    nice = subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.splitlines() if names else []
    return {n: out[k] for k, n in zip(names, nice)}


def normal(body):
    seen = {}

    def label(m):
        return seen.setdefault(m.group(0), f".L{len(seen)}")
    # (the kernel descriptor's directive repeats the function's own symbol: dropped, so that a renamed kernel can compare equal)
    return [re.sub(r"\.L[A-Za-z_]*\d+(_\d+)?", label, re.sub(r"^\.amdhsa_kernel \S+", ".amdhsa_kernel", ln)) for ln in body]


def main():
    args = sys.argv[1:]
    DEFINES[:] = [a for a in args if a.startswith("-D")]
    args = [a for a in args if not a.startswith("-D")]
    renames = []
    while "--rename" in args:
        i = args.index("--rename")
        renames.append(args[i + 1].split("=", 1))
        del args[i:i + 2]
    rev = args.pop(0) if args and not subprocess.run(["git", "-C", ROOT, "rev-parse", "--verify", "-q", args[0] + "^{commit}"], capture_output=True).returncode else "HEAD~1"
    with tempfile.TemporaryDirectory() as tmp:
        old = os.path.join(tmp, "rev")
        os.makedirs(old)
        tar = subprocess.run(["git", "-C", ROOT, "archive", rev, "voxel_rt2_amd/csrc", "voxel_rt2_amd/build.py", "include"], check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", old], input=tar, check=True)
        a, b = side(old, tmp, "a", rev), side(ROOT, tmp, "b", "this tree")
    for pat, repl in renames:
        b = {re.sub(pat, repl, n): body for n, body in b.items()}
    pick = lambda n: not args or any(s in n for s in args)
    same = reordered = differ = 0
    for n in sorted(set(a) | set(b)):
        if not pick(n):
            continue
        if n not in a or n not in b:
            print(f"only in {'this tree' if n in b else rev}: {n[:150]}")
        elif normal(a[n]) == normal(b[n]):
            same += 1
        elif sorted(normal(a[n])) == sorted(normal(b[n])):   # (labels are numbered in order of appearance: a moved BLOCK is not this)
            reordered += 1
            print(f"SAME INSTRUCTIONS, DIFFERENT ORDER ({len(a[n])} instructions): {n[:150]}")
        else:
            differ += 1
            print(f"DIFFERS ({len(a[n])} -> {len(b[n])} instructions): {n[:150]}")
    print(f"{same} functions identical to {rev}'s, {reordered} hold the same instructions in another order, {differ} differ")
    return 1 if differ or reordered else 0


if __name__ == "__main__":
    sys.exit(main())
