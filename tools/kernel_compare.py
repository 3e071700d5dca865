#!/usr/bin/env python3
"""Are the kernels of two source trees the same machine code?  For a refactor of host code.

    python tools/kernel_compare.py PARENT_TREE BRANCH_TREE [file.hip ...] [-j N] [--rename REGEX=REPL ...] [--new-ok]

Every .hip file named (default: every one of luciddreamer_amd/build.py's SOURCES that differs between the trees, or includes a
header under csrc/ that does) is compiled in both trees with `hipcc -S --cuda-device-only` and that file's flags from the BRANCH
tree's build.py, once without and once with -DLR_DIAGNOSTICS.  The kernels (.amdhsa_kernel symbols) of the two assemblies must be
the same set, and for each kernel the text from its label to .end_amdhsa_kernel -- code and descriptor: registers, LDS, scratch
-- must be equal once comments are dropped and the numbers of local labels (.LBB<n>_, .Lfunc_end<n>, ...) are replaced.  Kernels
are matched by name, so the order in which they are emitted does not matter.  Text is compared, nothing is searched for.

A branch that adds a template argument to a kernel changes its symbol and nothing else: --rename REGEX=REPL (repeatable) is
applied to the BRANCH's assembly before it is cut into kernels, so that such a kernel meets its parent under the parent's name
(for a trailing bool that is true in the old instantiations: --rename '(k_render_fwd\w*I(?:Lb[01]E)+)Lb1EE=\1E').  --new-ok:
kernels that only the branch has (after renaming) are listed and not counted as a difference.

Prints one line per file and build, "<file> [diagnostics]: N kernels, 0 differ", and exits non-zero if any kernel differs or is
missing on one side.  Needs hipcc; no GPU."""
import argparse
import concurrent.futures
import filecmp
import importlib.util
import os
import re
import subprocess
import sys
import tempfile

REL_CSRC = os.path.join("luciddreamer_amd", "csrc")
_LABEL = re.compile(r"\.L(BB|func_end|func_begin|tmp|JTI)\d+(_\d+)?")


def load_build(tree):
    spec = importlib.util.spec_from_file_location("lr_build_of_tree", os.path.join(tree, "luciddreamer_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def kernels(asm_text):
    """{kernel name: normalised text from its label to .end_amdhsa_kernel}."""
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm_text, flags=re.M))
    out, name, buf = {}, None, []
    for line in asm_text.splitlines():
        m = re.match(r"^(\S+):", line)
        if name is None and m and m.group(1) in names and m.group(1) not in out:
            name, buf = m.group(1), []
        if name is None:
            continue
        line = _LABEL.sub(lambda mm: ".L" + mm.group(1) + "N", re.sub(r"\s*;.*$", "", line.rstrip()))
        if line.strip():
            buf.append(line)
        if re.match(r"^\s*\.end_amdhsa_kernel", line):
            out[name] = "\n".join(buf)
            name = None
    return out


def assemble(build, tree, src, diagnostics, outdir, renames=()):
    inc = os.path.join(outdir, "inc")
    os.makedirs(inc, exist_ok=True)
    with open(os.path.join(inc, "lr_src_hash.h"), "w") as f:           # api.hip's generated header; the hash is host data
        f.write('#define LR_SRC_HASH "kernel_compare"\n')
    out = os.path.join(outdir, src.replace(".hip", ".s"))
    flags = [f for f in build.COMMON_FLAGS if f != build.INCLUDE and f not in ("-I", "-fPIC")]
    cmd = [build.hipcc(), "-S", "--cuda-device-only", os.path.join(tree, REL_CSRC, src), "-o", out] + flags + \
          ["-I", os.path.join(tree, "include"), "-I", inc] + build.SOURCES[src] + (["-DLR_DIAGNOSTICS"] if diagnostics else [])
    subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    with open(out) as f:
        text = f.read()
    for pattern, repl in renames:
        text = re.sub(pattern, repl, text)
    return kernels(text)


def touched(build, parent, branch):
    a, b = os.path.join(parent, REL_CSRC), os.path.join(branch, REL_CSRC)
    differs = lambda f: not (os.path.exists(os.path.join(a, f)) and os.path.exists(os.path.join(b, f)) and
                             filecmp.cmp(os.path.join(a, f), os.path.join(b, f), shallow=False))
    headers = {f for f in set(os.listdir(a)) | set(os.listdir(b)) if f.endswith(".h") and differs(f)}
    # a changed header reaches a file directly or through common.h; when in doubt the file is compared
    via_common = bool(headers)
    picked = []
    for src in build.SOURCES:
        text = open(os.path.join(b, src)).read()
        includes = set(re.findall(r'#include "([^"]+)"', text))
        if differs(src) or includes & headers or (via_common and "common.h" in includes):
            picked.append(src)
    return picked


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("parent")
    ap.add_argument("branch")
    ap.add_argument("files", nargs="*")
    ap.add_argument("-j", type=int, default=8)
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=REPL")
    ap.add_argument("--new-ok", action="store_true")
    args = ap.parse_args()
    renames = [tuple(r.split("=", 1)) for r in args.rename]
    parent, branch = os.path.abspath(args.parent), os.path.abspath(args.branch)
    build = load_build(branch)
    files = args.files or touched(build, parent, branch)
    if not files:
        print("no .hip file differs between the trees")
        return 0
    bad = 0
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(max(1, args.j)) as pool:
        jobs = {}
        for src in files:
            for diag in (False, True):
                for side, tree in (("parent", parent), ("branch", branch)):
                    d = os.path.join(tmp, side + ("_diag" if diag else ""))
                    jobs[(src, diag, side)] = pool.submit(assemble, build, tree, src, diag, d, renames if side == "branch" else ())
        for src in files:
            for diag in (False, True):
                try:
                    a, b = jobs[(src, diag, "parent")].result(), jobs[(src, diag, "branch")].result()
                except subprocess.CalledProcessError as e:
                    print(f"{src}{' [diagnostics]' if diag else ''}: hipcc failed\n{e.stdout}")
                    bad += 1
                    continue
                only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
                differ = sorted(k for k in set(a) & set(b) if a[k] != b[k])
                print(f"{src}{' [diagnostics]' if diag else ''}: {len(b)} kernels, {len(differ)} differ" +
                      (f", {len(only_a)} only in the parent, {len(only_b)} only in the branch" if only_a or only_b else ""))
                for k in (differ + only_a + only_b)[:10]:
                    print("    " + k)
                bad += len(differ) + len(only_a) + (0 if args.new_ok else len(only_b))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
