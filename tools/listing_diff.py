#!/usr/bin/env python3
"""Kernel-by-kernel comparison of two device listings: does a source change leave a kernel's instructions what they were?

    python tools/listing_diff.py OLD_TREE NEW_TREE [--map FILE] [--files k_kmpc.hip,k_stmpc.hip]
    python tools/listing_diff.py old.s new.s [--map FILE]

A tree is a checkout of this repository: the named files of its csrc/ are compiled to gfx950 assembly (`-S --cuda-device-only`) with the
flags of that tree's csrc/Makefile, per-file flags included.  A listing is the output of such a compile.  Per kernel of OLD the tool prints
"identical" or the number of differing lines, after normalising what a rename or a move changes and the instructions do not: basic-block
label numbers, mangled symbol names, comments and the section line (a template instantiation sits in a comdat section of its own).  The
kernel descriptor (.amdhsa_*: registers, scratch, LDS) is compared with the instructions.

--map FILE: lines `old_name new_name`, demangled, without namespace and arguments, e.g.
    k_kmpc_plan_gen_idx k_kmpc_plan_gen_t<KmpcIdxArgs>
A kernel not in the map is looked up under its own name, then as `name<>` (it became a template whose plain instantiation takes no arguments).  Exit status 1 when a kernel differs or is missing.  CPU only.
"""
import difflib
import os
import re
import shutil
import subprocess
import sys
import tempfile

CXXFILT = shutil.which("llvm-cxxfilt", path="/opt/rocm/lib/llvm/bin" + os.pathsep + os.environ.get("PATH", "")) or "c++filt"


def demangle(names):
    out = subprocess.run([CXXFILT], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return [re.sub(r"^void ", "", re.sub(r"\(.*$", "", o)).replace("f1p::", "") for o in out[:len(names)]]


def kernels(path):
    """{demangled name: normalised lines} of every .amdhsa_kernel of a listing"""
    bodies, cur, name = {}, None, None
    for ln in open(path, errors="replace"):
        m = re.match(r"^(_Z\w+):", ln)
        if m:                                                       # (a label before the last one's descriptor: that was a device function)
            name, cur = m.group(1), []
            continue
        if cur is None:
            continue
        ln = ln.split(";")[0].rstrip()
        if ln.strip() == ".end_amdhsa_kernel":
            bodies[name], cur = cur, None
        elif ln.strip() and not re.match(r"\s*\.(section|size|p2align|type|globl|protected|weak)\b", ln):
            cur.append(re.sub(r"_Z\w+", "SYM", re.sub(r"\.L(BB|func_end|tmp)\d+(_?)", r".L\1\2", ln)))
    names = list(bodies)
    return dict(zip(demangle(names), (bodies[n] for n in names)))


def listing(tree, src, out):
    csrc = os.path.join(tree, "f1tenth_planning_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS \?= (.*)$", mk, re.M).group(1).split()
    obj = re.escape(src[:-len(".hip")]) + r"\.o"
    for m in re.finditer(r"^(.*):\s*override EXTRA \+= (\S+)", mk, re.M):      # per-file flags: by object name, or by a $(foreach m,$(LIST),...)
        lst = re.search(r"\$\(foreach \w+,\$\((\w+)\)", m.group(1))
        members = re.search(rf"^{lst.group(1)} = (.*)$", mk, re.M).group(1).split() if lst else []
        if re.search(obj, m.group(1)) or src[:-len(".hip")] in members:
            flags.append(m.group(2))
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", *flags, "-S", "--cuda-device-only", src, "-o", out], cwd=csrc, check=True)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    opt = {a: sys.argv[sys.argv.index(a) + 1] for a in ("--map", "--files") if a in sys.argv}
    args = [a for a in args if a not in opt.values()]
    if len(args) != 2:
        raise SystemExit(__doc__)
    names = dict(ln.strip().split(None, 1) for ln in open(opt["--map"]) if ln.strip() and not ln.startswith("#")) if "--map" in opt else {}
    pairs = []
    if os.path.isdir(args[0]):
        tmp = tempfile.mkdtemp(prefix="listing_diff_")
        for src in opt.get("--files", "k_kmpc.hip,k_stmpc.hip").split(","):
            outs = [os.path.join(tmp, f"{side}_{src[:-4]}.s") for side in ("old", "new")]
            for tree, out in zip(args, outs):
                listing(tree, src, out)
            pairs.append((src, *outs))
    else:
        pairs.append((os.path.basename(args[0]), args[0], args[1]))
    bad = 0
    for label, old, new in pairs:
        a, b = kernels(old), kernels(new)
        print(f"{label}: {len(a)} kernels")
        for k in sorted(a):
            kb = names.get(k, k)
            if kb not in b and kb + "<>" in b:                      # a kernel that became the empty instantiation of a variadic template
                kb += "<>"
            if kb not in b:
                print(f"  {k:<44} MISSING ({kb})")
                bad += 1
                continue
            if a[k] == b[kb]:
                print(f"  {k:<44} identical ({len(a[k])} lines)")
                continue
            ops = difflib.SequenceMatcher(None, a[k], b[kb], autojunk=False).get_opcodes()
            nd = sum(max(i2 - i1, j2 - j1) for t, i1, i2, j1, j2 in ops if t != "equal")
            print(f"  {k:<44} {nd} lines differ ({len(a[k])} -> {len(b[kb])})")
            bad += 1
    raise SystemExit(1 if bad else 0)


if __name__ == "__main__":
    main()
