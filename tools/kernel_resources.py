#!/usr/bin/env python3
"""Per-kernel register / spill / scratch table of every .hip translation unit in csrc/ ("check with
-Rpass-analysis=kernel-resource-usage ... and fail on VGPR spills per instantiation").

    python tools/kernel_resources.py            # table
    python tools/kernel_resources.py --check    # exit 1 when a kernel carries more scratch than its budget (BUDGET; default 0)
    python tools/kernel_resources.py --objdir build_x    # another object directory of csrc/ (variant builds)

Reads the compiler's own remarks of the REAL build (csrc/Makefile keeps them next to every object, <obj>.res: same flags as the shipped
object, per-file flags such as k_stmpc.o's -fno-slp-vectorize included); `make libf1p.so` is run first so they are current.  Nothing is
compiled here, nothing is written outside the build directory.  CPU only (hipcc cross-compiles gfx950).
"""
import glob
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "f1tenth_planning_amd", "csrc")
# scratch bytes per lane a kernel may carry (mangled-name substring -> budget).  Everything else must have none.
#   ILb1E...            the materialising variants (all_traj requested): HBM-write-bound, not VALU-bound.  Round 6: 160 -> 56 -- the clothoid + footprint
#                       instantiation is spill-free at two waves per SIMD (was 104 B); what is left is cubic + footprint's 52 B (12 VGPRs; two waves measured 4 % slower)
#   k_kmpc_*            spills sit in the once-per-workgroup setup blocks and the rarely taken serial fp64 fallback, not in the
#                       filter loop (tools/isa_loops.py); a lower register cap was measured slower (LABNOTES.md 5b)
#   k_lattice / g1      the out-of-line fp64 fit's 8-byte frame; the branch-and-bound instantiation of a TRACK plan (k_lattice<.., PRUNE, .., TRK>) 24 B:
#                       two VGPRs spilled around the per-ego track look-up -- a fall-back shape (f1p_lattice_set_mode(0), candidate slices), the
#                       track plans' default schedule is the mixed one
#   k_lattice_filter3<CR, true, ..>   the instantiations with the test hooks compiled in.  They ARE what launch_lattice_mixed launches for host-supplied
#                       goals (<CR, true, true>), cubic + footprint and footprint + host goals -- production plan shapes of the add_sample_function
#                       path -- so those shapes carry this budget (8-24 B of scratch); the spill-free claim holds for the device-goal shapes
#                       (<CR, false, false, GEN, FOOT = false>: 0 scratch, asserted below by the default budget of 0)
#   k_kmpc_plan_gen_t<> / <KmpcIdxArgs>   (IJEE / IJNS_11KmpcIdxArgsEEE) the planning kernel and its instantiation with the ego indirection of
#                       f1p_stmpc_plan_batch's kinematic branch: 7 / 14 VGPRs (32 / 52 B) spilled in the same once-per-workgroup blocks, none in
#                       the three filter loops (tools/isa_loops.py).  The two instantiations with the occupancy test carry none; the keys are
#                       whole template argument lists, so they match nothing else
#   k_stmpc_shoot_t<StCtlGen>   (INS_8StCtlGenEJEE: k_stmpc_shoot_gen, not its _col form) the PLAIN-fp64 evaluation of f1p_stmpc_plan_* (f1p_stmpc_set_mode(0): the parity mode, not the default schedule): 36 B of
#                       SGPR spill slots around the all-fp64 rollout loop's set-up.  The default schedule's kernels (k_stmpc_filter_gen,
#                       _refine_gen, _refine_tp_gen, _decide_gen) carry none
#   k_kmpc_plan_gen_t<KmpcIdxArgs, KmpcObs>   the kinematic branch of f1p_stmpc_plan_batch with f1p_stmpc_set_obstacles' discs: 4 VGPRs (12 B), reloaded in the
#                       fp64 tails (the refinement's time-parallel disc test and the serial fp64 fallback), none in the three f32 filter loops; the
#                       same kernel without the indirection (k_kmpc_plan_gen_obs) carries none
#   k_lattice<.., cubic, .., LatObs>   the all-fp64 kernel's cubic instantiations WITH the moving discs' argument (f1p_lattice_set_obstacles): 2 VGPRs (12 B) in
#                       the point-footprint ones, 28 (60 B) in materialised + footprint, whose instantiation without discs carries 52 B.  While discs are set
#                       cubic plans run here; the clothoid ones stay inside the budgets of their instantiations without discs
BUDGET = {"9k_latticeILb0ELi1ELb0ELb0ELb0EJNS_6LatObs": 12, "9k_latticeILb0ELi1ELb0ELb0ELb1EJNS_6LatObs": 12,
          "9k_latticeILb1ELi1ELb0ELb1ELb0EJNS_6LatObs": 60, "9k_latticeILb1ELi1ELb0ELb1ELb1EJNS_6LatObs": 60,
          "ILb1E": 56, "k_kmpc_plan_gen_tIJEE": 32, "k_kmpc_plan_gen_tIJNS_11KmpcIdxArgsEEE": 52, "k_kmpc_plan_gen_tIJNS_11KmpcIdxArgsENS_7KmpcObsEEE": 12, "k_stmpc_shoot_tINS_8StCtlGenEJEE": 36, "k_kmpc_shoot_mixed": 0, "k_rivals": 0, "k_course_arc": 0, "k_rivals_frenet": 0, "k_rivals_predict": 0, "k_clothoid_g1": 8, "9k_latticeILb0E": 8,
          "k_lattice_filter3ILi1ELb1E": 24, "k_lattice_filter3ILi2ELb1E": 24,
          "k_lattice_filter3ILi1ELb0ELb0ELi0ELb1E": 8, "k_lattice_filter3ILi2ELb0ELb0ELi0ELb1E": 8,
          "9k_latticeILb0ELi0ELb1ELb0ELb1E": 24}   # (the instantiations WITH test hooks -- incl. the host-goal shapes; device goals, point footprint: 0)
# The headline kernels (k_lattice_prologue, k_lattice_filter3<CR, false, false, GEN, false>) carry NO scratch and no VGPR spills;
# `make resources` is part of __graft_entry__.build().


def demangle(names):
    try:
        out = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-cxxfilt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
        return [re.sub(r"\(.*$", "", o).replace("f1p::", "") for o in out[:len(names)]]
    except OSError:
        return names


def resources(res_file):
    rows, cur = [], None
    for ln in open(res_file, errors="replace").read().splitlines():
        m = re.search(r"remark:\s+(Function Name|TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill|LDS Size \[bytes/block\]):\s*(\S+)", ln)
        if not m:
            continue
        k, v = m.groups()
        if k == "Function Name":
            cur = {"name": v}
            rows.append(cur)
        elif cur is not None:
            cur[k.split(" [")[0]] = v
    return rows


def main():
    check = "--check" in sys.argv
    quiet = "--quiet" in sys.argv
    bad = []
    out = sys.stdout
    if quiet:
        sys.stdout = open(os.devnull, "w")
    print(f"{'kernel':<58} {'SGPR':>5} {'VGPR':>5} {'AGPR':>5} {'sgpr-spill':>10} {'vgpr-spill':>10} {'scratch':>8} {'occ':>4} {'LDS':>7}")
    objdir = sys.argv[sys.argv.index("--objdir") + 1] if "--objdir" in sys.argv else "build"
    if objdir == "build":                                   # the default build: bring it (and its remarks) up to date first
        r = subprocess.run(["make", "-C", CSRC, "-j4", "libf1p.so"], capture_output=True, text=True)
        if r.returncode:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(r.returncode)
    srcs = sorted(glob.glob(os.path.join(CSRC, "k_*.hip"))) + sorted(glob.glob(os.path.join(CSRC, "f1p_*.hip")))   # the kernel files, then the host API units
    res = [os.path.join(CSRC, objdir, os.path.basename(p)[:-len(".hip")] + ".o.res") for p in srcs]
    missing = [p for p in res if not os.path.exists(p)]
    if missing:
        raise SystemExit(f"kernel_resources: {objdir}/ holds remarks for {len(res) - len(missing)} of {len(srcs)} source files "
                         f"({os.path.basename(missing[0])} missing) -- rebuild (make clean; make)")
    for rf in res:
        rows = resources(rf)
        names = demangle([r["name"] for r in rows])
        for r, nm in zip(rows, names):
            print(f"{nm[:58]:<58} {r.get('TotalSGPRs', '?'):>5} {r.get('VGPRs', '?'):>5} {r.get('AGPRs', '?'):>5} {r.get('SGPRs Spill', '?'):>10} "
                  f"{r.get('VGPRs Spill', '?'):>10} {r.get('ScratchSize', '?'):>8} {r.get('Occupancy', '?'):>4} {r.get('LDS Size', '?'):>7}")
            budget = max([v for k, v in BUDGET.items() if k in r["name"]] + [0])
            if int(r.get("ScratchSize", 0)) > budget:
                bad.append(f"{nm} ({r.get('ScratchSize')} B > {budget})")
    sys.stdout = out
    if check and bad:
        print("scratch over budget:", ", ".join(bad))
        raise SystemExit(1)


if __name__ == "__main__":
    main()
