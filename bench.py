#!/usr/bin/env python3
"""bench.py -- candidate-trajectory-steps/sec of the batched lattice planner on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

`python bench.py --gpus N` without a launcher starts the N ranks itself (torch.distributed.run as a child process, before
this process touches the GPU) and passes their output and exit code through.

One "step" = one batched LatticePlanner.plan() over a batch of synthetic egos (BASELINE.json configs[2]:
4096 egos x 256 candidates x 50 stations) through the C-ABI, inputs already resident in HBM when the timed
region starts.  Egos are independent, so with N ranks every rank plans its own 4096 egos on its own GPU with no
data-path collective (weak scaling; N = 8 is BASELINE configs[3]); the ranks only meet in the barrier around the timed
region and in the max-over-ranks of the elapsed time (gloo, CPU tensors -- torch never touches the GPU in this process).

Rank 0 prints ONE JSON line with the driver's contract fields plus
  roofline            -- the dominant kernel (k_lattice) against the HBM roofline: algorithmic bytes per launch / the
                         kernel's average duration from HIP events on the ctx stream; the kernel is fp64-VALU bound by
                         construction (0.14 B per candidate-step), so the fp64 VALU fraction is reported next to it, from the
                         newest committed PMC profile (profiles/*_pmc.json, parsed here)
  cpu_baseline        -- the CPU oracle (C port of the reference's algorithm, OpenMP) on a bounded sample of the workload
  cpu_baseline_numpy  -- the numpy-vectorised restatement on ONE core (north_star's "same-box CPU numpy baseline")
  candidate_sharded   -- ONE ego batch with its candidate set split over the N ranks: slice evaluation, the RCCL
                         all-reduce(min) exchange (f1p_comm_argmin_dev) and the winner re-emission, checked bit for bit
                         against the unsharded plan; `rccl_ranks` is what the communicator itself reports
  kmpc_c4             -- BASELINE configs[4]: 1024 egos x 512 rollouts x 30 steps in total, 1024 / N egos per GPU.
`--shard candidates` makes the candidate-sharded pipeline the timed step (strong scaling over the candidate set).
"""
import argparse
import glob
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8 TB/s spec
# VALU issue peaks, T lane-instructions/s at 2.4 GHz (1024 SIMDs x 64 lanes x 2.4e9 / cycles per wave64 instruction):
#   F32_GUIDE   78.6  MI355X_MICROARCH.md: SIMD-32, a wave64 v_fma_f32 per 2 cycles (157.3 TFLOP/s of FMA).  `valu.frac` is
#                     quoted against THIS figure for the f32 filter kernels (VERDICT r2 #1a).
#   F32_MEASURED 62.9 what the chip actually issues for the cheapest class -- v_add / v_mul / v_fmac / v_fma with VGPR or literal
#                     operands, v_and / v_or / v_lshrrev / v_add_u32: 2.5 cycles per instruction at any occupancy >= 2 waves
#                     per SIMD (tools/microbench/issue_cycles.hip, profiles/r03_valu_issue_cycles.txt)
#   SLOW_CLASS  36.5  4.3 cycles: v_max / v_min / v_floor / v_cvt / v_bfe / v_cmp / v_cndmask / DPP / integer multiplies, every fp64
#                     instruction, packed f32 (two results per instruction), anything with an SGPR operand -- the fp64 kernels'
#                     reference (round 2 quoted 39.3 = 4 cycles)
#   TRANS       18.9  8.3 cycles: v_sin / v_cos / v_rcp / v_sqrt / v_exp
VALU_PEAK_F32_GUIDE = 78.6
VALU_PEAK_F32_MEASURED = 62.9
VALU_PEAK_SLOW_CLASS = 36.5
VALU_CYC = {"fast": 2.5, "slow": 4.3, "trans": 8.3}
VALU_ISSUE_PEAK_TLANES = VALU_PEAK_SLOW_CLASS      # fp64 kernels (kmpc / all-fp64 lattice lines)



# ---------------------------------------------------------------------------------------------------------------------------------
# The record.  The driver parses the LAST stdout line and keeps about 8 KB of tail: round 5's 27 KB line did not parse.
# The line is now a compact object (< 4 KB: contract fields, roofline, cpu_baseline, parity, a bounded set of flat scalars); the full
# record -- every nested leg -- goes to bench_full.json beside this script (and into gpurun_out/ when that directory exists).
COMPACT_MAX_BYTES = 4096
FULL_RECORD_PATH = None          # --full-record
COMPACT_CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data")
COMPACT_CONFIG = ("workload", "egos_per_gpu", "candidates", "stations", "generator", "state", "rollouts", "horizon", "parallelism")
COMPACT_ROOFLINE = ("bound", "achieved", "peak", "unit", "frac", "traffic", "traffic_source", "kernel", "kernel_ms", "dominant_kernel_ms",
                    "algorithmic_bytes_per_launch", "shader_clock_mhz")
COMPACT_CPU = ("value", "unit", "cores", "kind", "sample")
COMPACT_PARITY = ("egos_checked", "best_idx_mismatches", "max_abs_dsteer", "near_idx_mismatches", "max_abs_steer_diff", "max_abs_dspeed")
# flat scalars, in the order they are dropped LAST-first should the line ever outgrow COMPACT_MAX_BYTES
COMPACT_SCALARS = (
    "per_gpu_value", "rccl_ranks", "exchange_us_p50", "candidate_sharded_ranks", "candidate_sharded_bit_identical", "exchange_selftest_ok",
    "hsa_ipc_env_zero_on_every_rank", "audit_mismatching_egos", "other_schedules_bit_identical",
    "host_boundary_p50_ms", "host_boundary_d2h_ms", "host_boundary_no_traj_p50_ms", "closed_loop_step_p50_ms",
    "kernel_ms_prologue", "kernel_ms_filter3", "kernel_ms_refine", "kernel_ms_select",
    "valu_instr_per_candidate", "traffic_over_algorithmic_bytes",
    "scene_sweep_worst_vs_centred", "scene_sweep_all_bit_identical", "scene_sweep_oracle_mismatches",
    "kmpc_c4_streamed_ms", "kmpc_c4_generated_ms", "kmpc_c4_cache_stream_frac", "kmpc_c4_generated_roofline_frac",
    "kmpc_stream8192_ms", "kmpc_stream8192_hbm_frac", "kmpc_stream8192_shader_mhz",
    "pursuit_65536_ms", "pursuit_plans_per_s", "pursuit_valu_issue_frac", "pursuit_near_idx_mismatches",
    "all_fp64_ms", "every_station_ms", "first_plan_ms_per_plan", "two_plans_in_flight_ms_per_plan",
    "host_goals_ms_per_plan", "cubic_ms_per_plan", "footprint_ms_per_plan", "materialised_hbm_frac", "blocked_egos",
)


def _compact_value(v, text=160):
    """numbers to 6 significant digits, non-finite floats to null (strict JSON), long strings cut"""
    if isinstance(v, bool) or v is None or isinstance(v, int):
        return v
    if isinstance(v, float):
        if v != v or v in (float("inf"), float("-inf")):
            return None
        return float("%.6g" % v)
    if isinstance(v, str):
        return v if len(v) <= text else v[:text - 1] + "~"
    if isinstance(v, (list, tuple)):
        return [_compact_value(x, text) for x in v[:8]]
    if hasattr(v, "item"):                       # numpy scalar
        return _compact_value(v.item(), text)
    return None


def _pick(d, keys, text=160):
    if not isinstance(d, dict):
        return None
    return {k: _compact_value(d[k], text) for k in keys if k in d and not isinstance(d[k], dict)}


def compact_record(full, max_bytes=COMPACT_MAX_BYTES):
    """The one line the driver parses: the contract's fields + roofline + cpu_baseline (+ parity, per-rank times, flat scalars) of `full`."""
    rec = {k: _compact_value(full.get(k)) for k in COMPACT_CONTRACT}
    rec["config"] = _pick(full.get("config"), COMPACT_CONFIG, text=200) or {"workload": None}
    roof = _pick(full.get("roofline"), COMPACT_ROOFLINE, text=96)
    if roof is not None:
        if isinstance(roof.get("kernel"), str) and "dominant kernel is " in full["roofline"]["kernel"]:
            roof["kernel"] = full["roofline"]["kernel"].split("dominant kernel is ")[1].rstrip(")")
        for k in ("traffic", ):
            roof.setdefault(k, None)
    rec["roofline"] = roof
    rec["cpu_baseline"] = _pick(full.get("cpu_baseline"), COMPACT_CPU, text=200)
    if isinstance(full.get("cpu_baseline_numpy"), dict):
        rec["cpu_baseline_numpy"] = _pick(full["cpu_baseline_numpy"], ("value", "cores"))
    rec["parity"] = _pick(full.get("parity"), COMPACT_PARITY)
    prk = full.get("per_rank_ms_per_step")
    if isinstance(prk, dict):
        rec["per_rank_ms_per_step"] = _pick(prk, ("min", "max", "ranks"))
    for k in COMPACT_SCALARS:
        if full.get(k) is not None and not isinstance(full[k], (dict, list)):
            rec[k] = _compact_value(full[k])
    rec["full_record"] = os.path.basename(FULL_RECORD_PATH or "bench_full.json")
    keys = [k for k in reversed(COMPACT_SCALARS) if k in rec]
    line = json.dumps(rec, separators=(",", ":"), allow_nan=False)
    while len(line) > max_bytes and keys:
        rec.pop(keys.pop(0))
        line = json.dumps(rec, separators=(",", ":"), allow_nan=False)
    return rec, line


def _strict(o):
    """non-finite floats -> None all the way down, so the side file is strict JSON too"""
    if isinstance(o, dict):
        return {str(k): _strict(v) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return [_strict(v) for v in o]
    if hasattr(o, "item") and not isinstance(o, (str, bytes)):
        o = o.item()
    if isinstance(o, float) and (o != o or o in (float("inf"), float("-inf"))):
        return None
    return o


def emit(full, stream=None, rk=None):
    """rank 0: full record -> bench_full.json (stderr names it), compact record -> the LAST stdout line"""
    if rk is not None and "per_rank_ms_per_step" not in full and getattr(rk, "last_per_rank_s", None) and full.get("steps"):
        prs = list(rk.last_per_rank_s)                       # every workload's line carries every rank's own time (a straggler is visible)
        full["per_rank_ms_per_step"] = {"min": min(prs) / full["steps"] * 1e3, "max": max(prs) / full["steps"] * 1e3, "ranks": len(prs)}
    full = _strict(full)
    _, line = compact_record(full)
    written = []
    targets = [FULL_RECORD_PATH or os.path.join(ROOT, "bench_full.json")]
    if FULL_RECORD_PATH is None and os.path.isdir(os.path.join(ROOT, "gpurun_out")):
        targets.append(os.path.join(ROOT, "gpurun_out", "bench_full.json"))
    for path in targets:
        try:
            with open(path, "w") as f:
                json.dump(full, f, allow_nan=False)
                f.write("\n")
            written.append(path)
        except OSError:
            pass
    print("bench.py: full record (%d bytes as one line) -> %s" % (len(json.dumps(full)), ", ".join(written) or "nowhere writable"), file=sys.stderr, flush=True)
    sys.stderr.flush()
    print(line, file=stream or sys.stdout, flush=True)
    return line


DUMP_MAX_BYTES = 64 * 10**6      # --dump-outputs: every .npy file together, headers included
DUMP_COSTS = ("best_cost", "all_cost")   # +inf by contract for a candidate in collision (f1p.h check_collision): always carry a _nonfinite file


def dump_outputs(path, arrays, max_bytes=DUMP_MAX_BYTES):
    """--dump-outputs: name -> array (one row per ego along axis 0) -> path/<name>.npy.  Integer columns are written as float64 (exact), float32
    stays float32.  Every file is finite: a non-finite entry is written as 0 and <name>_nonfinite.npy holds, at the same index, +1 for +inf,
    -1 for -inf, 2 for NaN and 0 for a finite value (written for the DUMP_COSTS arrays always, for any other array when it has such an entry).
    When the set would exceed max_bytes, every array keeps the same rows: a sorted sample of egos drawn with a fixed seed, whose indices go
    to ego_rows.npy."""
    import numpy as np
    arrays = {k: np.ascontiguousarray(v if v.dtype in (np.float32, np.float64) else v.astype(np.float64)) for k, v in arrays.items()}
    for name in list(arrays):
        v = arrays[name]
        bad = ~np.isfinite(v)
        if name in DUMP_COSTS or bad.any():
            code = np.zeros(v.shape)
            code[v == np.inf], code[v == -np.inf], code[np.isnan(v)] = 1.0, -1.0, 2.0
            arrays[name + "_nonfinite"] = code
            arrays[name] = np.where(bad, v.dtype.type(0), v)
    n = len(next(iter(arrays.values())))
    header = 256                                           # an .npy header is 128 bytes for these shapes; twice that to be safe
    budget = max_bytes - header * (len(arrays) + 1)
    row_bytes = sum(v[:1].nbytes for v in arrays.values())
    if n * row_bytes > budget:
        k = budget // (row_bytes + 8)
        rows = np.sort(np.random.default_rng(0).choice(n, k, replace=False))
        arrays = {name: v[rows] for name, v in arrays.items()}
        arrays["ego_rows"] = rows.astype(np.float64)
    os.makedirs(path, exist_ok=True)
    for name, v in arrays.items():
        np.save(os.path.join(path, name + ".npy"), v)
    print("bench.py: outputs of the last timed step (%s) -> %s" % (", ".join("%s %s" % (k, list(v.shape)) for k, v in arrays.items()), path),
          file=sys.stderr, flush=True)


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--egos", type=int, default=4096)
    ap.add_argument("--cands", type=int, default=256)
    ap.add_argument("--stations", type=int, default=50)
    ap.add_argument("--cpu-egos", type=int, default=0, help="egos in the CPU-baseline sample (0 = auto, ~10-20 s)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--full-record", default=None, help="where rank 0 writes the full record (default: bench_full.json beside this script, and gpurun_out/ "
                                                        "when it exists); stdout's last line is the compact record either way")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, rank 0 writes what the last timed step computed (the arrays a caller of that path receives) as "
                         "DIR/<name>.npy, float64 (float32 stays float32), at most 64 MB in all: a fixed, seeded sample of egos when larger; "
                         "every file is finite, +-inf / NaN entries (a blocked ego's +inf best_cost) are flagged in <name>_nonfinite.npy")
    ap.add_argument("--no-secondary", action="store_true", help="skip the candidate-sharded and kmpc legs of the default run")
    ap.add_argument("--only-timed", action="store_true",
                    help="profiling runs (tools/profile_gpu.sh): nothing but the warm-up and the timed steady-state region touches the GPU, so that "
                         "every dispatch of a kernel in the trace is a steady-state one")
    ap.add_argument("--latency-iters", type=int, default=200, help="host-boundary plan() calls for p50/p95 (0 = skip)")
    ap.add_argument("--workload", choices=["lattice", "lattice-materialised", "kmpc", "stmpc", "pursuit"], default="lattice",
                    help="lattice = the headline (BASELINE configs[2]); the others are secondary lines for DESIGN.md")
    ap.add_argument("--shard", choices=["egos", "candidates"], default="egos",
                    help="lattice, N ranks: egos = every rank plans its own egos (no collective, the headline); candidates = ONE ego "
                         "batch, every rank evaluates a slice of the candidates, RCCL all-reduce(min), every rank re-emits the winner")
    ap.add_argument("--generator", choices=["clothoid", "cubic"], default="clothoid",
                    help="candidate generator: clothoid = the reference's (headline); cubic = cubic Hermite spline (secondary line)")
    ap.add_argument("--kmpc-f64", action="store_true", help="kmpc: plain fp64 evaluation instead of the f32 filter + fp64 refinement")
    ap.add_argument("--kmpc-cost", action="store_true", help="kmpc: also request best_cost (forces an fp64 re-evaluation of every winner)")
    ap.add_argument("--kmpc-stream", action="store_true", help="kmpc: controls streamed from an HBM buffer instead of generated in registers")
    ap.add_argument("--all-fp64", action="store_true", help="lattice: time the all-fp64 kernel (f1p_lattice_set_mode 0) instead of the default f32-filter / fp64-decision schedule")
    ap.add_argument("--prune", action="store_true", help="lattice: time the branch-and-bound kernel as the step (default: exhaustive; the default run reports branch and bound beside it)")
    ap.add_argument("--rollouts", type=int, default=512)
    ap.add_argument("--horizon", type=int, default=30)
    return ap.parse_args(argv)


# ---------------------------------------------------------------------------------------------------------------------
# self-launch: `python bench.py --gpus N` with no launcher.  Runs BEFORE anything GPU-related is imported: this parent
# never creates a HIP context and never re-execs; the ranks are ordinary child processes.
# ---------------------------------------------------------------------------------------------------------------------
def visible_gpus():
    """GPU nodes in the KFD topology (a file read: does not initialise the GPU).  None when the topology is unreadable."""
    nodes = glob.glob("/sys/class/kfd/kfd/topology/nodes/*/properties")
    if not nodes:
        return None
    n = 0
    for p in nodes:
        try:
            props = dict(line.split()[:2] for line in open(p) if len(line.split()) >= 2)
        except OSError:
            return None
        if int(props.get("simd_count", "0")) > 0:
            n += 1
    return n


def self_launch(args, argv):
    have = visible_gpus()
    if have is not None and have < args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} requested but only {have} GPU(s) are visible on this node")
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")       # dmabuf IPC: RCCL across processes needs it on this pool
    env.setdefault("OMP_NUM_THREADS", "1")
    return subprocess.call(cmd, env=env)


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    args = parse_args(argv)
    global FULL_RECORD_PATH
    FULL_RECORD_PATH = os.path.abspath(args.full_record) if args.full_record else None
    # every rank, however it was launched (self-launch above, or the driver's own torchrun): dmabuf IPC before anything loads
    # HIP -- RCCL across processes fails with `hipIpcGetMemHandle: invalid argument` on this pool without it
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.environ.setdefault("OMP_WAIT_POLICY", "passive")     # the CPU-baseline oracle's idle OpenMP workers sleep instead of spinning beside the GPU legs
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        raise SystemExit(self_launch(args, argv))
    sys.path.insert(0, ROOT)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if args.workload == "kmpc":
        return main_kmpc(args)
    if args.workload == "pursuit":
        return main_pursuit(args)
    if args.workload == "stmpc":
        return main_stmpc(args)
    return main_lattice(args)


# ---------------------------------------------------------------------------------------------------------------------
# shared plumbing
# ---------------------------------------------------------------------------------------------------------------------
class Ranks:
    """rank bookkeeping + the gloo group used for the barrier and the max-over-ranks of the elapsed time"""

    def __init__(self):
        self.rccl_ok, self.rccl_hung, self.rccl_note = True, False, None
        self.last_per_rank_s = None
        self.rank = int(os.environ.get("RANK", "0"))
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        self.local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        self.dist = None
        self.oversubscribed = False

    def open_context(self):
        """One rank per GPU; fails loudly when the node has fewer devices than local ranks."""
        from f1tenth_planning_amd import _abi
        from f1tenth_planning_amd.runtime import Context   # loads libf1p.so before torch is imported
        n = _abi.load_library().f1p_device_count()
        local_world = int(os.environ.get("LOCAL_WORLD_SIZE", str(self.world)))
        # F1P_BENCH_OVERSUBSCRIBE=1 (tests only): several ranks share the devices there are, to exercise the N-rank control flow
        # (barriers, max over ranks, rank-0 line) on a 1-GPU box; RCCL refuses two ranks on one device, so those legs are skipped
        self.oversubscribed = os.environ.get("F1P_BENCH_OVERSUBSCRIBE") == "1" and n >= 1 and n < local_world
        if n < 1 or (self.world > 1 and n < local_world and not self.oversubscribed):
            raise SystemExit(f"bench.py: {local_world} ranks on this node but f1p_device_count() = {n}")
        return Context(self.local_rank % n if self.oversubscribed else self.local_rank)

    def init(self):
        if self.world > 1:
            import torch.distributed as dist_mod   # CPU-only use: gloo barrier + max
            self.dist = dist_mod
            self.dist.init_process_group(backend="gloo", rank=self.rank, world_size=self.world)

    def barrier(self):
        if self.dist:
            self.dist.barrier()

    def max(self, x):
        if not self.dist:
            return float(x)
        import torch
        t = torch.tensor([float(x)], dtype=torch.float64)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        return float(t.item())

    def gather(self, x):
        """every rank's value of x, in rank order (a list of floats on every rank)"""
        if not self.dist:
            return [float(x)]
        import torch
        out = [torch.zeros(1, dtype=torch.float64) for _ in range(self.world)]
        self.dist.all_gather(out, torch.tensor([float(x)], dtype=torch.float64))
        return [float(t.item()) for t in out]

    def all_equal_int(self, v):
        """True when every rank holds the same integer"""
        if not self.dist:
            return True
        import torch
        lo = torch.tensor([int(v)], dtype=torch.int64); hi = lo.clone()
        self.dist.all_reduce(lo, op=self.dist.ReduceOp.MIN); self.dist.all_reduce(hi, op=self.dist.ReduceOp.MAX)
        return bool(lo.item() == hi.item())

    def exchange(self, ctx, d_cost, d_idx, E):
        """the cross-rank argmin of the candidate-sharded mode: RCCL on the ctx stream; with ranks sharing a GPU (test hook) the same
        rule on the host through gloo (f1tenth_planning_amd.dist.argmin_allreduce), so that everything around the collective runs"""
        if not self.oversubscribed:
            ctx.comm_argmin_dev(d_cost, d_idx, E)
            return
        import numpy as np
        from f1tenth_planning_amd.dist import argmin_allreduce
        c, i = argmin_allreduce(d_cost.download(np.float64, (E,)), d_idx.download(np.int32, (E,)))
        d_cost.upload(c); d_idx.upload(i)

    def comm_info(self, ctx):
        """(ranks, rank) of the RCCL communicator itself; (None, rank) under the test hook that shares one GPU between ranks -- no
        communicator exists there, the exchange is the gloo stand-in"""
        return (None, self.rank) if self.oversubscribed else ctx.comm_info()

    def init_rccl(self, ctx, fatal=False):
        """ncclCommInitRank off the critical path.  The communicator only serves the candidate-sharded / exchange legs -- the headline
        (ego-sharded, no collective) never needs it -- so it is brought up in a daemon thread with a deadline (30 s at one rank, 120 s
        with several; F1P_RCCL_INIT_TIMEOUT_S overrides) and the ranks agree on the outcome through the gloo group: if ANY rank's
        communicator did not come up, EVERY rank skips the legs that need it, the line says why (`rccl_init`), and the processes leave
        through os._exit after printing (a thread may still sit inside the bootstrap).  Seen this round: ncclCommInitRank with ONE
        rank never returned on one box.  fatal = True (`--shard candidates`: the run IS the collective): the rank prints why and exits 3
        -- a wedged bootstrap fails the run instead of hanging it.  Never a re-exec."""
        if self.oversubscribed:
            return
        import threading
        t_lim = float(os.environ.get("F1P_RCCL_INIT_TIMEOUT_S", 120.0 if self.dist else 30.0))
        box = {}

        def bring_up():
            try:
                if self.dist:
                    from f1tenth_planning_amd.dist import init_rccl
                    init_rccl(ctx, self.rank, self.world)
                else:
                    ctx.comm_init(ctx.comm_unique_id(), 1, 0)
                box["ok"] = True
            except Exception as exc:   # noqa: BLE001 -- reported, not raised: the headline does not depend on it
                box["err"] = str(exc)
        th = threading.Thread(target=bring_up, daemon=True)
        th.start()
        th.join(t_lim)
        mine = (not th.is_alive()) and box.get("ok", False)
        everyone = self.all_equal_int(1 if mine else 0) and mine
        if everyone:
            return
        self.rccl_ok = False
        self.rccl_hung = th.is_alive()
        why = (f"ncclCommInitRank did not return within {t_lim:.0f} s" if th.is_alive() else
               ("communicator init failed: " + box["err"]) if "err" in box else "another rank's communicator did not come up")
        self.rccl_note = (f"rank {self.rank}/{self.world}: {why} (HSA_ENABLE_IPC_MODE_LEGACY={os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY')}, "
                          f"MASTER_ADDR={os.environ.get('MASTER_ADDR')}): candidate-sharded and exchange legs skipped")
        sys.stderr.write("bench.py: " + self.rccl_note + "\n")
        sys.stderr.flush()
        if fatal:
            os._exit(3)

    def env_ok(self):
        """HSA_ENABLE_IPC_MODE_LEGACY=0 on EVERY rank (set by main() when the launcher did not)"""
        return self.all_equal_int(1 if os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY") == "0" else 0) and os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY") == "0"

    def close(self):
        if self.dist:
            self.dist.barrier()
            self.dist.destroy_process_group()


def timed_region(rk, ctx, step, warmup, steps):
    """W untimed steps, barrier + sync, EXACTLY K timed steps, sync + barrier; returns (max-over-ranks seconds, HIP-event ms)"""
    for _ in range(warmup):
        step()
    ctx.sync()
    rk.barrier()
    ctx.timer_begin()                                       # HIP events on the stream the kernels run on
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    kernel_ms_total = ctx.timer_end()                       # synchronises the stream
    ctx.sync()
    elapsed = time.perf_counter() - t0
    rk.last_per_rank_s = rk.gather(elapsed)                 # launch skew is the only thing ego sharding can lose: min / max over the ranks go into the line
    elapsed = rk.max(elapsed)
    rk.barrier()
    return elapsed, kernel_ms_total


def load_pmc(config):
    """Newest committed PMC profile of the headline kernel for this workload configuration (profiles/rNN_*_pmc.json, written
    by tools/prof_summary.py --json from the separate rocprofv3 --pmc passes of this same command).  Parsed at run time so
    the roofline never carries a number pasted into this file."""
    best = None
    for p in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc.json"))):
        try:
            d = json.load(open(p))
        except (OSError, ValueError):
            continue
        if d.get("config") != config:
            continue
        for k in d.get("kernels", []):
            if k.get("headline"):
                best = dict(k, source=os.path.relpath(p, ROOT), all_kernels=d.get("kernels", []))
    return best


def algorithmic_bytes_lattice(E, C, S, n_wp, grid_w, grid_h, device_goals=True):
    """SURVEY.md 8(d), fp64 payloads: poses in, (goals in), waypoints + bit-packed grid once, scalars + best_traj out."""
    b = E * 32                                   # poses [E][4] f64
    if not device_goals:
        b += E * C * 24                          # goals [E][C][3] f64
    b += n_wp * 32                               # waypoints x, y, v, psi f64 (read once, then cache-resident)
    b += ((grid_w + 31) // 32) * 4 * grid_h      # bit-packed occupancy (read once)
    b += E * (8 + 8 + 4 + 8 + 4 + 4)             # steer, speed, best_idx, best_cost, status, near_idx
    b += E * S * 32                              # best_traj [E][S][4] f64
    return b


# ---------------------------------------------------------------------------------------------------------------------
# secondary legs of the default run (every rank takes part)
# ---------------------------------------------------------------------------------------------------------------------
def leg_candidate_sharded(rk, ctx, rl, steps, E=4096, C=512, S=50, timed=True):
    """ONE batch of E egos (the same poses on every rank), C candidates split over the ranks (BASELINE configs[1]'s candidate
    set / configs[3]'s candidate-sharded mode): slice evaluation -> RCCL all-reduce(min) exchange -> winner re-emission on every
    rank.  Checked bit for bit against the unsharded plan of the same GPU."""
    import numpy as np
    from f1tenth_planning_amd import synth
    from f1tenth_planning_amd.dist import candidate_shard_cfg
    cfg = synth.bench_lattice_cfg(n_cand=C, n_stations=S)
    poses = synth.make_egos(rl, E, seed=101)
    sh = candidate_shard_cfg(cfg, rk.rank, rk.world)
    d_poses = ctx.to_device(poses)
    d_cost, d_idx = ctx.alloc(8 * E), ctx.alloc(4 * E)
    d_steer, d_speed, d_status, d_near, d_traj = ctx.alloc(8 * E), ctx.alloc(8 * E), ctx.alloc(4 * E), ctx.alloc(4 * E), ctx.alloc(8 * E * S * 4)
    r_steer, r_speed, r_idx, r_cost, r_status, r_near, r_traj = (ctx.alloc(8 * E), ctx.alloc(8 * E), ctx.alloc(4 * E), ctx.alloc(8 * E),
                                                                  ctx.alloc(4 * E), ctx.alloc(4 * E), ctx.alloc(8 * E * S * 4))
    # the similarity term is live here too: a first plan's winners are the previous path of the sharded plan AND of its unsharded truth
    ctx.lattice_set_closed_loop(False)
    ctx.lattice_plan_dev(d_poses, E, cfg, r_steer, r_speed, r_idx, r_cost, r_status, r_near, r_traj)
    d_prev = ctx.to_device(np.ascontiguousarray(r_traj.download(np.float64, (E, S, 4))[:, :, 2]))
    ctx.lattice_plan_dev(d_poses, E, cfg, r_steer, r_speed, r_idx, r_cost, r_status, r_near, r_traj, d_prev_theta=d_prev)   # the unsharded truth
    nranks, myrank = rk.comm_info(ctx)

    def step():
        ctx.lattice_plan_dev(d_poses, E, sh, None, None, d_idx, d_cost, d_prev_theta=d_prev)             # this rank's candidate slice
        rk.exchange(ctx, d_cost, d_idx, E)                                                               # RCCL, same stream
        ctx.lattice_emit_dev(d_poses, E, cfg, d_idx, d_cost, d_steer, d_speed, d_status, d_near, d_traj)
    step.outputs = lambda: {"steer": d_steer.download(np.float64, (E,)), "speed": d_speed.download(np.float64, (E,)),   # --dump-outputs
                            "best_idx": d_idx.download(np.int32, (E,)), "best_cost": d_cost.download(np.float64, (E,)),
                            "status": d_status.download(np.int32, (E,)), "near_idx": d_near.download(np.int32, (E,)),
                            "best_traj": d_traj.download(np.float64, (E, S, 4))}

    step(); ctx.sync()
    same = all(np.array_equal(a.download(t, s), b.download(t, s), equal_nan=(t == np.float64)) for a, b, t, s in
               ((d_steer, r_steer, np.float64, (E,)), (d_speed, r_speed, np.float64, (E,)), (d_idx, r_idx, np.int32, (E,)),
                (d_cost, r_cost, np.float64, (E,)), (d_status, r_status, np.int32, (E,)), (d_near, r_near, np.int32, (E,)),
                (d_traj, r_traj, np.float64, (E, S, 4))))
    same_everywhere = rk.all_equal_int(1 if same else 0) and same
    out = {"egos": E, "candidates": C, "stations": S, "candidates_per_rank": int(sh.cand_count), "ranks": rk.world, "rccl_ranks": None if nranks is None else int(nranks),
           "rccl_rank_of_reporter": int(myrank), "bit_identical_to_unsharded_plan_on_every_rank": bool(same_everywhere),
           "similarity_term": "live (previous path = a first plan's winners, device-resident)"}
    def exchange_only(n):
        """the exchange alone: evaluate, drain the stream, then time only the two collectives + the two key kernels"""
        def timed_exchange():
            ex = []
            for _ in range(n):
                ctx.lattice_plan_dev(d_poses, E, sh, None, None, d_idx, d_cost, d_prev_theta=d_prev)
                ctx.sync(); rk.barrier()
                ctx.timer_begin(); rk.exchange(ctx, d_cost, d_idx, E); ex.append(ctx.timer_end() * 1e3)
            return ex
        ex = timed_exchange()
        out.update({"exchange_us_p50": float(np.percentile(ex, 50)), "exchange_us_min": float(np.min(ex)), "exchange_bytes_per_rank": E * 12,
                    "exchange": ("host stand-in through gloo (ranks share one GPU: test hook)" if rk.oversubscribed else
                                 "all-reduce(min, u64 cost key) + all-reduce(min, i32 index among the holders), RCCL on the ctx stream")})
        if not rk.oversubscribed:                                  # the single-collective form, same results (checked by the self-test)
            ctx.comm_set_exchange(1)
            ex1 = timed_exchange()
            ctx.comm_set_exchange(0)
            out["exchange_allgather"] = {"us_p50": float(np.percentile(ex1, 50)), "us_min": float(np.min(ex1)), "bytes_gathered_per_rank": E * 16 * rk.world,
                                         "form": "f1p_comm_set_exchange(1): ONE all-gather of (key, index) records + a local minimum on every rank"}
    if timed:
        elapsed, ms_total = timed_region(rk, ctx, step, 3, steps)
        out.update({"ms_per_plan": elapsed / steps * 1e3, "candidate_steps_per_s": float(E) * C * S * steps / elapsed})
        exchange_only(min(steps, 50))
    return out, step, exchange_only


def leg_exchange_selftest(rk, ctx, E=1024):
    """The exchange on synthetic (cost, index) pairs with NaN / +-inf / signed zeros / cross-rank ties against np.argmin over the
    concatenation of all ranks' candidates (every rank can build every rank's arrays from the common seed)."""
    import numpy as np
    rng = np.random.default_rng(4242)
    W = rk.world
    cost = rng.normal(0, 1, (W, E))
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, 1.0, -1.0])
    pick = rng.integers(0, len(special) * 3, (W, E))
    cost = np.where(pick < len(special), special[np.minimum(pick, len(special) - 1)], cost)
    idx = (np.arange(W)[:, None] * 64 + rng.integers(0, 64, (W, E))).astype(np.int32)      # rank r holds indices [64 r, 64 r + 64)
    d_c, d_i = ctx.to_device(cost[rk.rank]), ctx.to_device(idx[rk.rank])
    rk.exchange(ctx, d_c, d_i, E)
    got_c, got_i = d_c.download(np.float64, (E,)), d_i.download(np.int32, (E,))
    same_ag = None
    if not rk.oversubscribed:                                      # the all-gather form must return the same bits
        d_c2, d_i2 = ctx.to_device(cost[rk.rank]), ctx.to_device(idx[rk.rank])
        ctx.comm_set_exchange(1); rk.exchange(ctx, d_c2, d_i2, E); ctx.comm_set_exchange(0)
        same_ag = bool(np.array_equal(d_i2.download(np.int32, (E,)), got_i) and np.array_equal(d_c2.download(np.float64, (E,)), got_c, equal_nan=True))
    # np.argmin over all ranks' candidates ordered by global index: first NaN, else first minimum
    want_i = np.empty(E, np.int32); want_c = np.empty(E)
    for e in range(E):
        order = np.argsort(idx[:, e], kind="stable")
        j = order[int(np.argmin(cost[order, e]))]
        want_i[e] = idx[j, e]; want_c[e] = cost[j, e]
    ok = bool(np.array_equal(got_i, want_i) and np.array_equal(got_c, want_c, equal_nan=True))
    return {"pairs": E, "nan_costs": int(np.isnan(cost).sum()), "matches_np_argmin_on_every_rank": rk.all_equal_int(1 if ok else 0) and ok,
            "allgather_form_identical_on_every_rank": None if same_ag is None else (rk.all_equal_int(1 if same_ag else 0) and same_ag)}


def kmpc_setup(rk, args, E, T, R, ctx=None):
    import numpy as np
    from f1tenth_planning_amd import _abi, synth
    cfg = _abi.kmpc_cfg(horizon=T, n_rollouts=R)
    cl = synth.make_centerline(seed=2)
    rng = np.random.default_rng(10 + rk.rank)
    k = rng.integers(0, len(cl) - 1, E)
    states = np.column_stack([cl[k, 1] + rng.normal(0, 0.1, E), cl[k, 2] + rng.normal(0, 0.1, E), rng.uniform(0.5, 5.5, E),
                              cl[k, 3] + rng.normal(0, 0.1, E)])
    own = ctx is None
    if own:
        ctx = rk.open_context()
    ctx.set_waypoints(cl, cols=(1, 2, 5, 3))
    ref = ctx.kmpc_ref(states, T)
    return ctx, cfg, states, ref, own


def leg_two_plans_in_flight(rk, rl, img, res, origin, poses, cfg, E, C, S, steps):
    """Two contexts (two HIP streams, two sets of scratch and output buffers) on this rank's GPU, independent plans of the SAME
    workload issued to them alternately: the latency-bound fp64 tail of one plan (refinement + selection: a third of a plan, few
    waves) overlaps with the next plan's filter.  What a caller gets by double-buffering consecutive batches; reported beside
    `value`, which stays the one-plan-at-a-time figure.  Outputs of both contexts are checked against each other."""
    import numpy as np
    ctxs = [rk.open_context(), rk.open_context()]
    bufs = []
    for c in ctxs:
        c.set_waypoints(rl); c.set_grid(img, res, origin, 206)
        c.lattice_set_closed_loop(True)                             # steady state: every plan's previous path is its context's last plan
        d_p = c.to_device(poses)
        bufs.append((d_p, (c.alloc(8 * E), c.alloc(8 * E), c.alloc(4 * E), c.alloc(8 * E), c.alloc(4 * E), c.alloc(4 * E), c.alloc(8 * E * S * 4))))
    for c, (d_p, b) in zip(ctxs, bufs):
        for _ in range(5):
            c.lattice_plan_dev(d_p, E, cfg, *b)
        c.sync()
    # (wall clock over two streams fed by ONE host thread: a host that is busy elsewhere starves both streams -- seen once as 0.21 ms per plan
    # against 0.050 on the next box -- so the region is timed three times and the fastest pass is the figure; every pass is in the record)
    passes = []
    for _ in range(3):
        rk.barrier()
        t0 = time.perf_counter()
        for k in range(steps):
            c, (d_p, b) = ctxs[k & 1], bufs[k & 1]
            c.lattice_plan_dev(d_p, E, cfg, *b)
        for c in ctxs:
            c.sync()
        passes.append(rk.max(time.perf_counter() - t0))
    elapsed = min(passes)
    rk.barrier()
    same = bool(np.array_equal(bufs[0][1][2].download(np.int32, (E,)), bufs[1][1][2].download(np.int32, (E,))) and
                np.array_equal(bufs[0][1][0].download(np.float64, (E,)), bufs[1][1][0].download(np.float64, (E,))))
    for c in ctxs:
        c.close()
    return {"plans": steps, "ms_per_plan": elapsed / steps * 1e3, "candidate_steps_per_s": float(E) * C * S * steps * rk.world / elapsed,
            "both_contexts_agree": same, "passes_ms_per_plan": [p / steps * 1e3 for p in passes],
            "note": "two contexts on one GPU, plans issued alternately (fastest of three timed passes): one plan's fp64 refinement / selection overlaps the next plan's f32 filter"}


def kmpc_valu_roofline(pmc, kernel_ms, E, R, T):
    """roofline.valu of k_kmpc_plan_gen from the newest committed PMC profile of this configuration (instructions per launch are a property
    of the code, the duration is the one measured in this run)"""
    if not (pmc and pmc.get("SQ_INSTS_VALU")):
        return None
    tl = pmc["SQ_INSTS_VALU"] * 64.0 / (kernel_ms * 1e-3) / 1e12
    v = {"kernel": pmc["kernel"], "achieved": tl, "peak": VALU_PEAK_F32_GUIDE, "unit": "T lane-instr/s", "frac": tl / VALU_PEAK_F32_GUIDE,
         "peak_definition": "MI355X_MICROARCH.md: one wave64 f32 VALU instruction per 2 cycles at 2.4 GHz; measured on this chip "
                            "(profiles/r03_valu_issue_cycles.txt): 2.5 cycles for plain VGPR-operand f32, 4.3 for packed f32 / integer multiplies / "
                            "conversions (most of this kernel: Philox + v_pk_fma), 8.3 for transcendentals",
         "frac_of_slow_class_issue_peak": tl / VALU_PEAK_SLOW_CLASS,
         "valu_instr_per_rollout_step": pmc["SQ_INSTS_VALU"] * 64.0 / (E * R * T), "source": pmc["source"]}
    if pmc.get("SQ_ACTIVE_INST_VALU") and pmc.get("GRBM_GUI_ACTIVE"):
        v["busy_frac_profiled"] = pmc["SQ_ACTIVE_INST_VALU"] * 4.0 / (1024.0 * pmc["GRBM_GUI_ACTIVE"] / 8.0)
    return v


def pursuit_valu_roofline(kernel_ms, E):
    """roofline of the batched pure pursuit from the newest committed PMC profile of this configuration (profiles/r*_pursuit_pmc.json): fp64 code, so the
    reference is the one-pass issue rate of an fp64 / VOP3 instruction (4.3 cycles per wave64 instruction per SIMD, profiles/r03_valu_issue_cycles.txt)"""
    pmc = load_pmc({"egos": E, "workload": "pursuit"})
    if not (pmc and pmc.get("SQ_INSTS_VALU")):
        return None
    tl = pmc["SQ_INSTS_VALU"] * 64.0 / (kernel_ms * 1e-3) / 1e12
    traffic = None
    if pmc.get("FETCH_SIZE_KiB") is not None and pmc.get("WRITE_SIZE_KiB") is not None:
        traffic = int((pmc["FETCH_SIZE_KiB"] * 2 + pmc["WRITE_SIZE_KiB"]) * 1024)      # gfx950 wide-read correction x2 (MI355X_MICROARCH.md)
    return {"bound": "valu", "achieved": tl, "peak": VALU_PEAK_SLOW_CLASS, "unit": "T lane-instr/s", "frac": tl / VALU_PEAK_SLOW_CLASS,
            "kernel": pmc["kernel"].split("(")[0].replace("void ", "").replace("f1p::", ""),
            "kernel_ms": kernel_ms, "valu_instr_per_ego": pmc["SQ_INSTS_VALU"] / float(E), "traffic": traffic, "algorithmic_bytes_per_launch": 52 * E,
            "traffic_source": pmc["source"],
            "peak_definition": "fp64 / VOP3 issue rate measured on this chip: one wave64 instruction per 4.3 cycles per SIMD at 2.4 GHz; 52 B per ego of HBM traffic is 1 % of the 8 TB/s roof"}


def leg_kmpc_c4(rk, args, steps):
    """BASELINE configs[4]: kinematic-MPC random shooting, 1024 egos x 512 rollouts x 30 steps IN TOTAL, 1024 / N egos per GPU.  Two
    variants: controls streamed from HBM (8 B per rollout-step) and -- the planner's own path, KMPCPlanner.plan -- controls generated in the
    kernel around the device-resident warm start.  Carries its own roofline, cpu_baseline (rank 0, N = 1) and parity gate."""
    import numpy as np
    from f1tenth_planning_amd.dist import shard_range
    T, R, E_total = 30, 512, 1024
    lo, hi = shard_range(E_total, rk.rank, rk.world)
    E = hi - lo
    ctx, cfg, states, ref, _ = kmpc_setup(rk, args, E, T, R)
    d_x0, d_ref = ctx.to_device(states), ctx.to_device(ref)
    d_ctrl = ctx.alloc(4 * E * T * 2 * R)
    ctx.kmpc_sample_controls_dev(d_ctrl, E, cfg, seed=2 + rk.rank)
    d_steer, d_speed, d_bi = ctx.alloc(8 * E), ctx.alloc(8 * E), ctx.alloc(4 * E)

    def step():
        ctx.kmpc_shoot_dev(d_x0, d_ref, d_ctrl, E, cfg, d_steer, d_speed, d_bi, None)
    elapsed, ms_total = timed_region(rk, ctx, step, 5, steps)
    kernel_ms = ms_total / steps
    abytes = E * R * T * 8 + E * (T + 1) * 32 + E * 32 + E * 28
    gbs = abytes / (kernel_ms * 1e-3) / 1e9
    out = {"workload": f"kmpc shooting: {E_total} egos x {R} rollouts x {T} steps over {rk.world} GPU(s) (BASELINE configs[4]), {E} egos per GPU",
           "rollout_steps_per_s": float(E_total) * R * T * steps / elapsed, "ms_per_plan": elapsed / steps * 1e3, "kernel_ms": kernel_ms,
           "control_stream_GBps_per_gpu": gbs,
           "roofline": {"bound": "hbm", "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS, "traffic": None,
                        "kernel": "k_kmpc_shoot_mixed", "algorithmic_bytes_per_launch": abytes, "bytes_per_rollout_step": abytes / (E * R * T),
                        "note": "126 MB of controls per 1024 egos are Infinity-Cache resident across launches below ~2048 egos per GPU: a cache-stream "
                                "rate, NOT an HBM fraction (profiles/r04_kmpc8192_* is the HBM-resident evidence)"},
           "note": "controls streamed from HBM as f32 [E][T][2][R]"}
    # parity + CPU baseline of the streamed plan (rank 0; the CPU figure is an N = 1 one)
    if rk.rank == 0 and not args.no_cpu_baseline:
        from oracle import oracle
        nthr = oracle.max_threads()
        n_cpu = min(E, max(nthr, 128))
        ctrl = d_ctrl.download(np.float32, (E, T, 2, R))[:n_cpu]
        t1 = time.perf_counter()
        want = oracle.kmpc_shoot_batch(states[:n_cpu], ref[:n_cpu], ctrl, cfg, nthreads=nthr)
        cpu_s = time.perf_counter() - t1
        got = d_bi.download(np.int32, (E,))[:n_cpu]
        out["parity"] = {"egos_checked": int(n_cpu), "best_idx_mismatches": int((want["best_idx"] != got).sum()),
                         "max_abs_dsteer": float(np.abs(want["steer"] - d_steer.download(np.float64, (E,))[:n_cpu]).max())}
        if rk.world == 1:
            out["cpu_baseline"] = {"value": n_cpu * R * T / cpu_s, "unit": "rollout-steps/s", "cores": nthr, "kind": "port",
                                   "sample": f"first {n_cpu} egos x {R} rollouts x {T} steps, oracle/f1p_oracle.c orc_kmpc_shoot_batch, {nthr} threads, {cpu_s:.2f} s"}
    # the same plan with the controls generated in the kernel around the device-resident warm start (no control buffer at all)
    from f1tenth_planning_amd import _abi
    calls = [0]

    def gstep():
        smp = _abi.kmpc_sampler(seed=2 + rk.rank, call=calls[0]); calls[0] += 1
        ctx.kmpc_plan_dev(d_x0, d_ref, E, cfg, smp, d_steer, d_speed, d_bi, None)
    g_elapsed, g_ms = timed_region(rk, ctx, gstep, 5, steps)
    ts = []
    for _ in range(30):                                   # host boundary: x0 up, reference extraction, plan, winners down
        smp = _abi.kmpc_sampler(seed=2 + rk.rank, call=calls[0]); calls[0] += 1
        t1 = time.perf_counter(); ctx.kmpc_plan(states, cfg, smp, want_seq=False, want_cost=False); ts.append((time.perf_counter() - t1) * 1e3)
    gen = {"rollout_steps_per_s": float(E_total) * R * T * steps / g_elapsed, "ms_per_plan": g_elapsed / steps * 1e3,
           "kernel_ms": g_ms / steps, "host_boundary_p50_ms": float(np.percentile(ts, 50)),
           "note": "f1p_kmpc_plan_*: Philox4x32-10 controls in registers around the ctx's warm start; VALU-bound, no HBM stream; "
                   "one workgroup per ego at every batch size (f1p_kmpc_set_groups can split an ego's rollouts; measured slower)"}
    if rk.rank == 0:
        g_bytes = E * (T + 1) * 32 + E * 32 + E * 28 + E * T * 16
        valu = kmpc_valu_roofline(load_pmc({"workload": "kmpc", "egos": E, "rollouts": R, "horizon": T, "controls": "generated"}), g_ms / steps, E, R, T)
        gen["roofline"] = {"bound": "valu" if valu else "hbm", "achieved": valu["achieved"] if valu else g_bytes / (g_ms / steps * 1e-3) / 1e9,
                           "peak": valu["peak"] if valu else HBM_PEAK_GBS, "unit": valu["unit"] if valu else "GB/s",
                           "frac": valu["frac"] if valu else g_bytes / (g_ms / steps * 1e-3) / 1e9 / HBM_PEAK_GBS, "traffic": None,
                           "kernel": "k_kmpc_plan_gen", "valu": valu,
                           "hbm": {"achieved": g_bytes / (g_ms / steps * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                   "algorithmic_bytes_per_launch": g_bytes, "bytes_per_rollout_step": g_bytes / (E * R * T)}}
        if not args.no_cpu_baseline:                      # parity of the generated plan: its controls materialised for the oracle
            from oracle import oracle
            nthr = oracle.max_threads()
            n_cpu = min(E, max(nthr, 128))
            ctx.kmpc_warm_reset()
            smp = _abi.kmpc_sampler(seed=2 + rk.rank, call=54321, use_warm=False)
            ctx.kmpc_plan_dev(d_x0, d_ref, E, cfg, smp, d_steer, d_speed, d_bi, None)
            ctx.kmpc_gen_controls_dev(d_ctrl, E, cfg, smp)
            ctrl = d_ctrl.download(np.float32, (E, T, 2, R))[:n_cpu]
            want = oracle.kmpc_shoot_batch(states[:n_cpu], ref[:n_cpu], ctrl, cfg, nthreads=nthr)
            gen["parity"] = {"egos_checked": int(n_cpu), "best_idx_mismatches": int((want["best_idx"] != d_bi.download(np.int32, (E,))[:n_cpu]).sum())}
    out["generated_in_kernel"] = gen
    ctx.close()
    return out


def read_sclk_mhz():
    """the shader clock level the driver marks active right now (sysfs pp_dpm_sclk; None when unreadable)"""
    import re
    best = None
    for pth in glob.glob("/sys/class/drm/card*/device/pp_dpm_sclk"):
        try:
            for line in open(pth):
                if "*" in line:
                    m = re.search(r"(\d+)\s*[Mm][Hh]z", line)
                    if m:
                        best = max(best or 0, int(m.group(1)))
        except OSError:
            pass
    return best


def leg_kmpc_stream8192(rk, args, steps=200, E=8192):
    """the streamed shooting kernel where its controls are HBM-resident -- 8192 egos x 512 rollouts x 30 steps, a 1.0 GB control buffer
    (four times the 256 MiB Infinity Cache) read once per launch: k_kmpc_shoot_mixed against the 8 TB/s HBM roofline, in the DEFAULT run so that the driver
    sees the figure.  The kernel's duration follows the shader clock (LABNOTES R5): the clock level the driver reports while the launches run is sampled
    from sysfs beside it."""
    import threading
    import numpy as np
    T, R = 30, 512
    ctx, cfg, states, ref, _ = kmpc_setup(rk, args, E, T, R)
    try:
        d_x0, d_ref = ctx.to_device(states), ctx.to_device(ref)
        d_ctrl = ctx.alloc(4 * E * T * 2 * R)
        ctx.kmpc_sample_controls_dev(d_ctrl, E, cfg, seed=12)
        d_steer, d_speed, d_bi = ctx.alloc(8 * E), ctx.alloc(8 * E), ctx.alloc(4 * E)

        def step():
            ctx.kmpc_shoot_dev(d_x0, d_ref, d_ctrl, E, cfg, d_steer, d_speed, d_bi, None)
        for _ in range(5):
            step()
        ctx.sync()
        clocks, stop = [], threading.Event()

        def sample():
            while not stop.is_set():
                c = read_sclk_mhz()
                if c:
                    clocks.append(c)
                time.sleep(0.002)
        th = threading.Thread(target=sample, daemon=True)
        th.start()
        ctx.timer_begin()
        for _ in range(steps):
            step()
        ms = ctx.timer_end() / steps
        stop.set(); th.join(1.0)
        abytes = E * R * T * 8 + E * (T + 1) * 32 + E * 32 + E * 28
        gbs = abytes / (ms * 1e-3) / 1e9
        out = {"workload": f"kmpc shooting, controls streamed: {E} egos x {R} rollouts x {T} steps, {abytes / 1e9:.3f} GB per launch (HBM-resident)",
               "kernel_ms": ms, "steps": steps, "rollout_steps_per_s": float(E) * R * T / (ms * 1e-3),
               "roofline": {"bound": "hbm", "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS, "kernel": "k_kmpc_shoot_mixed",
                            "algorithmic_bytes_per_launch": abytes, "bytes_per_rollout_step": abytes / (E * R * T)},
               "shader_clock_mhz": {"median": float(np.median(clocks)) if clocks else None, "min": min(clocks) if clocks else None, "max": max(clocks) if clocks else None,
                                    "samples": len(clocks), "source": "sysfs pp_dpm_sclk, sampled every 2 ms while the launches run"}}
        if not args.no_cpu_baseline:                          # parity on the first egos (the oracle reads the same control buffer)
            from oracle import oracle
            n_or = 64                                         # (the buffer's first rows: a prefix download, not the whole gigabyte)
            ctrl = d_ctrl.download(np.float32, (n_or, T, 2, R))
            want = oracle.kmpc_shoot_batch(states[:n_or], ref[:n_or], ctrl, cfg, nthreads=oracle.max_threads())
            out["parity"] = {"egos_checked": n_or, "best_idx_mismatches": int((want["best_idx"] != d_bi.download(np.int32, (E,))[:n_or]).sum())}
        return out
    finally:
        ctx.close()


def leg_pursuit(rk, rl, steps=200, E=65536):
    """north_star's first path -- PurePursuitPlanner.plan (control/pure_pursuit/pure_pursuit.py:85-122) -- batched: E egos on the bench's raceline, one
    k_pure_pursuit16<G> launch per step (G egos per wave by batch size), in the DEFAULT run so that the driver's record carries the row; the nearest
    indices and the steering against the oracle on the first 4096 egos.  (`--workload pursuit` is the same workload as a line of its own.)"""
    import numpy as np
    from f1tenth_planning_amd import synth
    poses = synth.make_egos(rl, E, seed=3)[:, :3]
    ctx = rk.open_context()
    try:
        ctx.set_waypoints(rl)
        d_poses = ctx.to_device(poses)
        d_steer, d_speed, d_near, d_la, d_st = ctx.alloc(8 * E), ctx.alloc(8 * E), ctx.alloc(4 * E), ctx.alloc(4 * E), ctx.alloc(4 * E)
        for _ in range(20):
            ctx.pure_pursuit_dev(d_poses, E, 0.8, d_steer, d_speed, d_near, d_la, d_st)
        ctx.sync(); ctx.timer_begin()
        for _ in range(steps):
            ctx.pure_pursuit_dev(d_poses, E, 0.8, d_steer, d_speed, d_near, d_la, d_st)
        ms = ctx.timer_end() / steps
        out = {"workload": f"pure pursuit: {E} egos on a {len(rl)}-point raceline (BASELINE configs[0], batched)", "kernel_ms": ms, "steps": steps,
               "plans_per_s": E / (ms * 1e-3), "algorithmic_bytes_per_launch": 52 * E, "roofline": pursuit_valu_roofline(ms, E),
               "note": "fp64 VALU issue-bound (chunk-pruned nearest scan, intersect_point's 64-segment steps, get_actuation): 52 B per ego of HBM traffic is 1 % of the 8 TB/s roof"}
        from oracle import oracle
        n_or = min(E, 4096)
        want = oracle.pure_pursuit_batch(poses[:n_or], rl, 0.8, nthreads=oracle.max_threads())
        out["parity"] = {"egos_checked": n_or, "near_idx_mismatches": int((d_near.download(np.int32, (E,))[:n_or] != want["near_idx"]).sum()),
                         "status_mismatches": int((d_st.download(np.int32, (E,))[:n_or] != want["status"]).sum()),
                         "max_abs_steer_diff": float(np.abs(d_steer.download(np.float64, (E,))[:n_or] - want["steer"]).max())}
        return out
    finally:
        ctx.close()


def leg_scene_sweep(rl, img, res, origin, cfg, E, C, S, steps, warmup=10, scenes=None, oracle_egos=256, order=True, device=0, clearance=None):
    """the headline workload (E x C x S, steady state of a closed loop, default schedule) on scenes it was NOT tuned on.
      centred       today's bench scene (sigma 0.3 m around the raceline, nothing inside the corridor)
      wall_hugging  sigma 0.9 m of a 1.1 m half-width corridor: many egos next to (or inside) a wall
      obstacles     discs of occupied cells ON the raceline every 10 m: the cheapest candidates of the egos behind one collide, so
                    the collision semantics the reference left as a stub (utils/utils.py:297-301) decide the plan
      moving        the centred fleet advancing 8 cm along the raceline per plan (a 10 m/s vehicle at 125 Hz): plan k's previous
                    path belongs to the pose of plan k-1
    Per scene: ms per plan over `steps` chained plans (HIP events on the ctx stream), the four kernels' own durations, what the lazy station
    pass looked at (f1p_lattice_debug_pass: candidates per ego, rounds), the refinement queue, the runtime audit, bit-identity of every
    output with the all-fp64 kernel (f1p_lattice_set_mode 0) on all E egos and best-index mismatches against the CPU oracle."""
    import numpy as np
    from f1tenth_planning_amd import _abi, synth
    from f1tenth_planning_amd.runtime import Context
    from oracle import oracle    # the checker
    nthr = oracle.max_threads()
    fleet = synth.make_line_egos(rl, E, seed=11)
    img_obs, _ = synth.stamp_obstacles(img, origin, res, rl, spacing=10.0, radius=0.30)
    n_plans = warmup + steps + 1
    all_scenes = {
        "centred": (img, lambda k: synth.make_egos(rl, E, seed=1)),
        "wall_hugging": (img, lambda k: synth.make_egos(rl, E, seed=1, pos_sigma=0.9)),
        "obstacles": (img_obs, lambda k: synth.make_egos(rl, E, seed=1)),
        "obstacles_moving": (img_obs, lambda k: synth.poses_along(rl, fleet, 0.08 * k)),
        "moving": (img, lambda k: synth.poses_along(rl, fleet, 0.08 * k)),
    }
    names = scenes or ["centred", "wall_hugging", "obstacles", "moving", "obstacles_moving"]
    out = {}
    for name in names:
        im, pose_of = all_scenes[name]
        moving = "moving" in name
        ctx = Context(device)
        try:
            ctx.set_waypoints(rl); ctx.set_grid(im, res, origin, 206)
            ctx.lattice_set_closed_loop(True)
            ctx.lattice_set_order(order)
            if clearance is not None:
                ctx.lattice_set_clearance(clearance)      # (A/B: tools/scene_sweep.py --clearance)
            pose_sets = [pose_of(k) for k in range(n_plans)] if moving else [pose_of(0)]
            d_pose = [ctx.to_device(p) for p in pose_sets]
            outs = [ctx.alloc(8 * E), ctx.alloc(8 * E), ctx.alloc(4 * E), ctx.alloc(8 * E), ctx.alloc(4 * E), ctx.alloc(4 * E), ctx.alloc(8 * E * S * 4)]
            k = 0

            def plan(d_prev=None):
                nonlocal k
                ctx.lattice_plan_dev(d_pose[k % len(d_pose)], E, cfg, *outs, d_prev_theta=d_prev)
                k += 1
            for _ in range(warmup):
                plan()
            ctx.sync()
            ctx.timer_begin()
            for _ in range(steps):
                plan()
            ms = ctx.timer_end() / steps
            # the chain's next plan: the one every comparison below repeats with its previous path handed over explicitly
            prev_in = ctx.lattice_closed_loop_prev()
            d_prev_in = ctx.to_device(prev_in)
            k_last = k
            plan()
            ctx.sync()
            ctx.lattice_set_closed_loop(False)
            poses_last = pose_sets[k_last % len(pose_sets)]
            got = {n: b.download(t, sh) for n, b, t, sh in (("steer", outs[0], np.float64, (E,)), ("speed", outs[1], np.float64, (E,)),
                                                          ("best_idx", outs[2], np.int32, (E,)), ("best_cost", outs[3], np.float64, (E,)),
                                                          ("status", outs[4], np.int32, (E,)), ("near_idx", outs[5], np.int32, (E,)),
                                                          ("best_traj", outs[6], np.float64, (E, S, 4)))}
            # (i) all fp64, same poses and previous path: every output bit for bit
            alt = [ctx.alloc(b.nbytes) for b in outs]
            ctx.lattice_set_mode(0)
            ctx.lattice_plan_dev(d_pose[k_last % len(d_pose)], E, cfg, *alt, d_prev_theta=d_prev_in)
            ctx.sync()
            ident = all(np.array_equal(alt[i].download(got[n].dtype, got[n].shape), got[n], equal_nan=(got[n].dtype != np.int32))
                        for i, n in enumerate(("steer", "speed", "best_idx", "best_cost", "status", "near_idx", "best_traj")))
            ctx.lattice_set_mode(1)
            # (ii) per-kernel durations + the station pass's statistics on that same plan
            ctx.lattice_profile(True)
            acc = np.zeros(4)
            n_prof = 10
            for _ in range(n_prof):
                k = k_last; plan(d_prev_in)
                acc += np.array(ctx.lattice_profile(True, read=True))
            ctx.lattice_profile(False)
            acc /= n_prof
            d_pass = ctx.to_device(np.zeros((E, 4), np.int32))
            ctx.lattice_debug_pass(d_pass)
            k = k_last; plan(d_prev_in); ctx.sync()
            ctx.lattice_debug_pass(None)
            ps = d_pass.download(np.int32, (E, 4))
            nq = ctx.lattice_debug_queue(E)
            stat = lambda v: {"mean": float(v.mean()), "p50": float(np.percentile(v, 50)), "p99": float(np.percentile(v, 99)), "max": int(v.max())}   # noqa: E731
            # (iii) runtime audit over the chain's plans (moving: different poses every plan)
            ctx.lattice_audit_read(reset=True)
            ctx.lattice_set_audit(1, min(256, E))
            for j in range(16):
                k = k_last; plan(d_prev_in)
            audit = ctx.lattice_audit_read(reset=True)
            ctx.lattice_set_audit(0)
            # (iv) the oracle on the first egos of that plan
            n_or = min(oracle_egos, E)
            want = oracle.lattice_plan_batch(poses_last[:n_or], rl, cfg, grid=(im, res, origin[0], origin[1], 206), prev_theta=prev_in[:n_or], nthreads=nthr)
            out[name] = {
                "ms_per_plan": ms, "nominal_candidate_steps_per_s": float(E) * C * S / (ms * 1e-3),
                "kernels_ms": {"k_lattice_prologue": float(acc[0]), "k_lattice_filter3": float(acc[1]), "k_lattice_refine": float(acc[2]), "k_lattice_select": float(acc[3])},
                "station_pass_candidates_per_ego": dict(stat(ps[:, 0]), of=C),
                "station_pass_lane_per_candidate_share": float(ps[:, 1].sum()) / max(1.0, float(ps[:, 0].sum())),
                "station_pass_rounds_per_ego": stat(ps[:, 2]),
                "station_pass_second_looks_per_ego": stat(ps[:, 3]),
                "refinement_queue_entries_per_ego": stat(nq),
                "blocked_egos": int((got["status"] == _abi.ST_ALL_BLOCKED).sum()),
                "outputs_bit_identical_to_all_fp64": bool(ident),
                "audit": audit,
                "oracle": {"egos_checked": n_or, "best_idx_mismatches": int((want["best_idx"] != got["best_idx"][:n_or]).sum()),
                           "max_abs_dsteer": float(np.abs(want["steer"] - got["steer"][:n_or]).max())},
            }
        finally:
            ctx.close()
    base = out.get("centred", {}).get("ms_per_plan")
    if base:
        for name in out:
            out[name]["vs_centred"] = out[name]["ms_per_plan"] / base
    return out


def leg_variants(rk, rl, img, res, origin, E, C, S, steps, warmup=10):
    """The other ways north_star / BASELINE.md section 4 name of running the same workload, each on a context of its own (rank 0):
      host_goals     the caller's goal set [E][C][3] instead of the device sampler -- what the reference's add_sample_function plug-in returns
                     (lattice_planner.py:57-70, 113-128); BASELINE.md section 4 row 2 (0.3816 B per candidate-step)
      cubic          cfg.generator = cubic Hermite spline candidates (north_star "clothoid / cubic-spline"), mixed schedule since round 5
      footprint      f1p_set_footprint: the vehicle rectangle covered by three discs along the heading, every station tested at their centres
      materialised   all_traj [E][C][S][4] + all_cost written to HBM, the reference's own data flow (lattice_planner.py:194-201);
                     BASELINE.md section 4 row 3 (32.38 B per candidate-step, HBM-bound) on a bounded ego count
    Each: ms per plan (HIP events on the ctx stream), steady state of a closed loop where the schedule supports it, bit-identity with the
    all-fp64 kernel and best-index mismatches against the CPU oracle on the first egos."""
    import copy
    import numpy as np
    from f1tenth_planning_amd import synth
    from f1tenth_planning_amd.runtime import Context
    from oracle import oracle    # the checker
    nthr = oracle.max_threads()
    grid = (img, res, origin[0], origin[1], 206)
    poses = synth.make_egos(rl, E, seed=1)
    names = ("steer", "speed", "best_idx", "best_cost", "status", "near_idx", "best_traj")
    out = {}

    def bufs(ctx, n):
        return [ctx.alloc(8 * n), ctx.alloc(8 * n), ctx.alloc(4 * n), ctx.alloc(8 * n), ctx.alloc(4 * n), ctx.alloc(4 * n), ctx.alloc(8 * n * S * 4)]

    def fetch(b, n):
        return {k: x.download(t, sh) for k, x, t, sh in zip(names, b, (np.float64, np.float64, np.int32, np.float64, np.int32, np.int32, np.float64),
                                                           ((n,), (n,), (n,), (n,), (n,), (n,), (n, S, 4)))}

    def timed(ctx, fn):
        """ms per plan, HIP events; the better of two passes of `steps` plans (a one-off stall of the box -- seen once: 87 ms inside one leg -- would
        otherwise be recorded as that variant's time; the headline's timed region is a single pass, as the contract demands)"""
        for _ in range(warmup):
            fn()
        best = None
        for _ in range(2):
            ctx.sync()
            ctx.timer_begin()
            for _ in range(steps):
                fn()
            ms = ctx.timer_end() / steps
            best = ms if best is None else min(best, ms)
        return best

    # ---- host goals ---------------------------------------------------------------------------------------------------------------------
    cfg = synth.bench_lattice_cfg(n_cand=C, n_stations=S)
    goals = synth.make_goals(rl, poses, np.linspace(0.6, 3.0, 16), np.linspace(-1.0, 1.0, C // 16))
    with Context(rk.local_rank) as ctx:
        ctx.set_waypoints(rl); ctx.set_grid(img, res, origin, 206)
        ctx.lattice_set_closed_loop(True)
        d_p, d_g, b = ctx.to_device(poses), ctx.to_device(goals), bufs(ctx, E)
        ms = timed(ctx, lambda: ctx.lattice_plan_dev(d_p, E, cfg, *b, d_goals=d_g))
        prev = ctx.lattice_closed_loop_prev(); d_prev = ctx.to_device(prev)
        ctx.lattice_set_closed_loop(False)
        ctx.lattice_plan_dev(d_p, E, cfg, *b, d_goals=d_g, d_prev_theta=d_prev); got = fetch(b, E)
        ctx.lattice_profile(True); acc = np.zeros(4)
        for _ in range(10):
            ctx.lattice_plan_dev(d_p, E, cfg, *b, d_goals=d_g, d_prev_theta=d_prev); acc += np.array(ctx.lattice_profile(True, read=True))
        ctx.lattice_profile(False)
        nq = ctx.lattice_debug_queue(E)
        ctx.lattice_set_mode(0)
        b2 = bufs(ctx, E)
        ms64 = timed(ctx, lambda: ctx.lattice_plan_dev(d_p, E, cfg, *b2, d_goals=d_g, d_prev_theta=d_prev)); ref = fetch(b2, E)
        n_or = min(256, E)
        want = oracle.lattice_plan_batch(poses[:n_or], rl, cfg, grid=grid, goals=goals[:n_or], prev_theta=prev[:n_or], nthreads=nthr)
        abytes = algorithmic_bytes_lattice(E, C, S, rl.shape[0], img.shape[1], img.shape[0], device_goals=False)
        out["host_goals"] = {"ms_per_plan": ms, "nominal_candidate_steps_per_s": float(E) * C * S / (ms * 1e-3), "all_fp64_ms_per_plan": ms64,
                             "kernels_ms": dict(zip(("k_lattice_prologue", "k_lattice_filter3", "k_lattice_refine", "k_lattice_select"), (float(v) / 10 for v in acc))),
                             "refinement_queue_entries_per_ego": float(nq.mean()),
                             "algorithmic_bytes_per_plan": abytes, "bytes_per_candidate_step": abytes / (float(E) * C * S),
                             "hbm_frac_of_8TBs": abytes / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                             "outputs_bit_identical_to_all_fp64": bool(all(np.array_equal(got[k], ref[k], equal_nan=(got[k].dtype != np.int32)) for k in names)),
                             "oracle": {"egos_checked": n_or, "best_idx_mismatches": int((want["best_idx"] != got["best_idx"][:n_or]).sum()),
                                        "max_abs_dsteer": float(np.abs(want["steer"] - got["steer"][:n_or]).max())},
                             "note": "goals [E][C][3] fp64 resident in HBM (synth.make_goals: arc-length look-aheads x lateral offsets in the ego frame), steady state of a "
                                     "closed loop; schedule: k_lattice_prologue (no look-ahead pass) -> k_lattice_filter3<HG> -> refine -> select"}
    # ---- cubic generator ------------------------------------------------------------------------------------------------------------------
    cfg_c = synth.bench_lattice_cfg(n_cand=C, n_stations=S, generator="cubic")
    with Context(rk.local_rank) as ctx:
        ctx.set_waypoints(rl); ctx.set_grid(img, res, origin, 206)
        ctx.lattice_set_closed_loop(True)
        d_p, b = ctx.to_device(poses), bufs(ctx, E)
        ms = timed(ctx, lambda: ctx.lattice_plan_dev(d_p, E, cfg_c, *b))
        prev = ctx.lattice_closed_loop_prev(); d_prev = ctx.to_device(prev)
        ctx.lattice_set_closed_loop(False)
        ctx.lattice_plan_dev(d_p, E, cfg_c, *b, d_prev_theta=d_prev); got = fetch(b, E)
        ctx.lattice_profile(True); acc = np.zeros(4)
        for _ in range(10):
            ctx.lattice_plan_dev(d_p, E, cfg_c, *b, d_prev_theta=d_prev); acc += np.array(ctx.lattice_profile(True, read=True))
        ctx.lattice_profile(False)
        nq = ctx.lattice_debug_queue(E)
        ctx.lattice_set_mode(0)
        b2 = bufs(ctx, E)
        ms64 = timed(ctx, lambda: ctx.lattice_plan_dev(d_p, E, cfg_c, *b2, d_prev_theta=d_prev)); ref = fetch(b2, E)
        n_or = min(128, E)
        want = oracle.lattice_plan_batch(poses[:n_or], rl, cfg_c, grid=grid, prev_theta=prev[:n_or], nthreads=nthr)
        out["cubic"] = {"ms_per_plan": ms, "nominal_candidate_steps_per_s": float(E) * C * S / (ms * 1e-3), "all_fp64_ms_per_plan": ms64,
                        "kernels_ms": dict(zip(("k_lattice_prologue", "k_lattice_filter3", "k_lattice_refine_cubic", "k_lattice_select"), (float(v) / 10 for v in acc))),
                        "refinement_queue_entries_per_ego": float(nq.mean()),
                        "outputs_bit_identical_to_all_fp64": bool(all(np.array_equal(got[k], ref[k], equal_nan=(got[k].dtype != np.int32)) for k in names)),
                        "oracle": {"egos_checked": n_or, "best_idx_mismatches": int((want["best_idx"] != got["best_idx"][:n_or]).sum()),
                                   "max_abs_dsteer": float(np.abs(want["steer"] - got["steer"][:n_or]).max())},
                        "note": "cubic Hermite spline candidates, steady state of a closed loop (similarity term live); round 5: the mixed schedule -- "
                                "k_lattice_prologue -> k_lattice_filter3<cubic> (an f32 walk over the stations with an a-priori error bound, table-driven "
                                "station passes) -> k_lattice_refine_cubic -> k_lattice_select<cubic>"}
    # ---- oriented footprint ----------------------------------------------------------------------------------------------------------------
    n_d, flen, fwid, foff = 3, 0.58, 0.31, 0.145             # the reference's vehicle (kinematic_mpc.py:60-61) covered by three discs, pose near the rear axle
    f_offsets = [foff - 0.5 * flen + (k + 0.5) * flen / n_d for k in range(n_d)]
    f_radius = float(np.hypot(0.5 * flen / n_d, 0.5 * fwid))
    with Context(rk.local_rank) as ctx:
        ctx.set_waypoints(rl); ctx.set_grid(img, res, origin, 206)
        ctx.set_footprint(f_offsets, f_radius)
        ctx.lattice_set_closed_loop(True)
        d_p, b = ctx.to_device(poses), bufs(ctx, E)
        ms = timed(ctx, lambda: ctx.lattice_plan_dev(d_p, E, cfg, *b))
        prev = ctx.lattice_closed_loop_prev(); d_prev = ctx.to_device(prev)
        ctx.lattice_set_closed_loop(False)
        ctx.lattice_plan_dev(d_p, E, cfg, *b, d_prev_theta=d_prev); got = fetch(b, E)
        ctx.lattice_profile(True); acc = np.zeros(4)
        for _ in range(10):
            ctx.lattice_plan_dev(d_p, E, cfg, *b, d_prev_theta=d_prev); acc += np.array(ctx.lattice_profile(True, read=True))
        ctx.lattice_profile(False)
        nq = ctx.lattice_debug_queue(E)
        ctx.lattice_set_mode(0)
        b2 = bufs(ctx, E)
        ms64 = timed(ctx, lambda: ctx.lattice_plan_dev(d_p, E, cfg, *b2, d_prev_theta=d_prev)); ref = fetch(b2, E)
        n_or = min(256, E)
        dil = oracle.inflate_image(img, res, 206, f_radius, nthreads=nthr)
        oracle.set_footprint(f_offsets)
        try:
            want = oracle.lattice_plan_batch(poses[:n_or], rl, cfg, grid=(dil, res, origin[0], origin[1], 206), prev_theta=prev[:n_or], nthreads=nthr)
        finally:
            oracle.set_footprint(())
        out["footprint"] = {"ms_per_plan": ms, "nominal_candidate_steps_per_s": float(E) * C * S / (ms * 1e-3), "all_fp64_ms_per_plan": ms64,
                            "discs": {"offsets_m": f_offsets, "radius_m": f_radius},
                            "kernels_ms": dict(zip(("k_lattice_prologue", "k_lattice_filter3", "k_lattice_refine", "k_lattice_select"), (float(v) / 10 for v in acc))),
                            "refinement_queue_entries_per_ego": float(nq.mean()),
                            "outputs_bit_identical_to_all_fp64": bool(all(np.array_equal(got[k], ref[k], equal_nan=(got[k].dtype != np.int32)) for k in names)),
                            "oracle": {"egos_checked": n_or, "best_idx_mismatches": int((want["best_idx"] != got["best_idx"][:n_or]).sum()),
                                       "max_abs_dsteer": float(np.abs(want["steer"] - got["steer"][:n_or]).max())},
                            "note": "f1p_set_footprint: every station tested at three disc centres along its heading against the disc-dilated bitmap (the "
                                    "reference's collision check is a stub: utils/utils.py:297-301; build-defined glue), steady state of a closed loop; since "
                                    "round 5 on k_lattice_prologue -> k_lattice_filter3<FOOT> -> k_lattice_refine<FOOT> -> k_lattice_select (was: the one-kernel "
                                    "fallback filter)"}
    # ---- all_traj materialised (HBM-bound) ----------------------------------------------------------------------------------------------
    Em = min(E, 1024)
    with Context(rk.local_rank) as ctx:
        ctx.set_waypoints(rl); ctx.set_grid(img, res, origin, 206)
        d_p, b = ctx.to_device(poses[:Em]), bufs(ctx, Em)
        d_ac, d_at = ctx.alloc(8 * Em * C), ctx.alloc(8 * Em * C * S * 4)
        ms = timed(ctx, lambda: ctx.lattice_plan_dev(d_p, Em, cfg, *b, d_all_cost=d_ac, d_all_traj=d_at))
        abytes = algorithmic_bytes_lattice(Em, C, S, rl.shape[0], img.shape[1], img.shape[0]) + Em * C * S * 32 + Em * C * 8
        gbs = abytes / (ms * 1e-3) / 1e9
        out["materialised"] = {"egos": Em, "ms_per_plan": ms, "nominal_candidate_steps_per_s": float(Em) * C * S / (ms * 1e-3),
                               "roofline": {"bound": "hbm", "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS,
                                            "algorithmic_bytes_per_launch": abytes, "bytes_per_candidate_step": abytes / (float(Em) * C * S),
                                            "traffic": None, "kernel": "k_lattice<STAGING> (all fp64, rows staged per wave in LDS and flushed as 128-byte chunks)"},
                               "note": "the reference's all_traj data flow (lattice_planner.py:194-201): every candidate's rows written once; "
                                       "the store-only ceiling of this chip is 4.1-4.4 TB/s (tools/microbench/stream.hip)"}
    return out


def filter_shape(S, r):
    """What k_lattice_filter3 does (csrc/k_lattice_mixed.hip): EVERY candidate gets the f32 fit and the four cost terms with their bracket
    (bracket_f2: nothing there looks at positions); the station pass -- positions and occupancy look-ups -- runs only for the candidates whose
    bracket reaches below the best collision-free one (station_pass_wave; pass_plan is mirrored here): in the clearance mode r the tested
    stations are r, r + G, r + 2 G, ... (G = 2 r + 1) and the last station when the tested ones do not cover it, each reached by ONE
    integrated piece.  r = 0 (every_station: no clearance map): every interval a piece of its own, every station looked up -- for the same lazy set."""
    if r <= 0:
        return {"pieces_integrated_per_candidate": S - 1, "stations_looked_up_per_candidate": S, "clearance_r": 0,
                "station_pass": "lazy, as with a clearance map; every look is the every-station one"}
    G = 2 * r + 1
    if G < S:
        nm = (S - 1 - r) // G
        pos = r + nm * G
        tests = 1 + nm + (1 if S - 1 > pos + r else 0)
    else:
        tests = 1
    return {"pieces_integrated_per_candidate": tests, "stations_looked_up_per_candidate": tests, "clearance_r": r,
            "intervals_per_candidate": S - 1, "stations_per_candidate": S,
            "station_pass": "lazy: only the candidates whose cost bracket reaches below the best collision-free candidate's (see "
                            "station_pass_candidates_per_ego); the fit and the cost bracket are computed for every candidate"}


def algorithmic_ops(poses, rl, cfg, grid, prev_in, n_egos=3, stride=8):
    """"the builder must replace these estimates by an exact count from its own CPU restatement".  oracle/opcount.py is the
    oracle's candidate path on a counting float (tests/test_oracle_opcount.py pins it to the C oracle's costs); here it runs over a sample of
    this run's candidates (every `stride`-th candidate of the first n_egos egos, similarity term and occupancy test included)."""
    from oracle import opcount, oracle
    tot = {"incremental": [], "reference": []}
    n = 0
    classes = None
    for e in range(min(n_egos, len(poses))):
        goals, valid = oracle.lattice_goals(poses[e], rl, cfg)
        g = goals[valid][::stride]
        if not len(g):
            continue
        for scheme in tot:
            _, counts = opcount.count_candidates(g, poses[e], cfg, grid=grid, prev_theta=None if prev_in is None else prev_in[e], scheme=scheme)
            sm = opcount.summarize(counts, len(g), cfg.n_stations)
            tot[scheme].append(sm["ops_per_candidate"])
            if scheme == "incremental":
                classes = sm["by_class_per_candidate"]
        n += len(g)
    if not n:
        return None
    import numpy as np
    return {"ops_per_candidate": float(np.mean(tot["incremental"])), "ops_per_candidate_step": float(np.mean(tot["incremental"])) / cfg.n_stations,
            "ops_per_candidate_reference_order": float(np.mean(tot["reference"])),
            "by_class_per_candidate": classes, "candidates_counted": n,
            "definition": "scalar fp64 ops of oracle/opcount.py's restatement of one candidate (G1 fit by Newton on 16-point Gauss-Legendre moments, "
                          "S stations, occupancy look-up, four cost terms): add/sub, mul, div, sqrt, compare-class and transcendental CALLS count 1 each, "
                          "a multiply-add pair 2.  ops_per_candidate = one 8-point rule per station interval + running sum (what a batched "
                          "implementation does: oracle/numpy_lattice.py); ops_per_candidate_reference_order = every station integrated from 0 as the "
                          "reference's per-station X(s) / Y(s) calls do (utils/utils.py:289-293)"}


# ---------------------------------------------------------------------------------------------------------------------
def leg_host_boundary_latency(ctx, args, poses, cfg, S, steady):
    """p50 / p95 latency of one plan() at the ctypes boundary: host poses in, host results out (H2D + kernel + D2H + sync).  Runs on every
    rank BEFORE the timed region (it also brings the chip's clocks up, so a short --steps run is not measuring the ramp from idle).  Closed
    loop: the similarity term is live in every one of these calls, nothing extra crosses PCIe."""
    import copy
    import numpy as np
    from f1tenth_planning_amd import synth

    def percentiles(fn):
        for _ in range(20):                                  # 20 warm-up + 200 timed calls
            fn()
        ts = []
        for _ in range(args.latency_iters):
            t1 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t1) * 1e3)
        return float(np.percentile(ts, 50)), float(np.percentile(ts, 95))
    p50, p95 = percentiles(lambda: ctx.lattice_plan(poses, cfg, want_traj=True, reuse_outputs=True))
    q50, q95 = percentiles(lambda: ctx.lattice_plan(poses, cfg, want_traj=True))
    r50, r95 = percentiles(lambda: ctx.lattice_plan(poses, cfg, want_traj=False, reuse_outputs=True))
    h50, h95 = percentiles(lambda: ctx.lattice_plan(poses, cfg, want_traj=True, reuse_outputs=True, traj_dtype=np.float32))
    c50, c95 = percentiles(lambda: ctx.lattice_step(poses, cfg))
    cfg_bb = copy.copy(cfg); cfg_bb.prune = 1
    ctx.lattice_set_mode(0)
    b50, b95 = percentiles(lambda: ctx.lattice_plan(poses, cfg_bb, want_traj=True, reuse_outputs=True))
    f50, f95 = percentiles(lambda: ctx.lattice_plan(poses, cfg, want_traj=True, reuse_outputs=True))
    ctx.lattice_set_mode(0 if (args.all_fp64 or args.prune) else 1)
    # BASELINE configs[1]: ONE ego x 512 candidates x 50 stations, the single-vehicle call
    cfg1 = synth.bench_lattice_cfg(n_cand=512, n_stations=S)
    ctx.lattice_set_closed_loop(False); ctx.lattice_set_closed_loop(steady)       # another batch shape: re-armed
    s50, s95 = percentiles(lambda: ctx.lattice_plan(poses[:1], cfg1, want_traj=True))
    u50, u95 = percentiles(lambda: ctx.lattice_plan(poses[:1], cfg1, want_traj=True, reuse_outputs=True))
    ctx.lattice_set_closed_loop(False); ctx.lattice_set_closed_loop(steady)
    return {"p50_ms": p50, "p95_ms": p95, "n": args.latency_iters,
            "includes": "poses in + kernels + steer/speed/idx/cost/status/near/best_traj out + sync (PCIe-inclusive), page-locked host arrays: since round 6 the prologue reads the poses and the selection kernel writes every result column and the rows straight from / into them (no hipMemcpy either way); "
                        "closed loop: the similarity term is live (previous headings stay on the device)",
            "closed_loop": {"p50_ms": c50, "p95_ms": c95,
                            "note": "f1p_lattice_step_batch: poses in, (steer, speed, status) out as ONE packed block the selection kernel writes straight "
                                    "into page-locked host memory; previous headings and best_traj stay on the device (f1p_lattice_fetch_traj on request)"},
            "pageable_host_arrays": {"p50_ms": q50, "p95_ms": q95},
            "without_best_traj": {"p50_ms": r50, "p95_ms": r95},
            "f32_best_traj": {"p50_ms": h50, "p95_ms": h95,
                              "note": "f1p_lattice_plan_batch_f32: the same fp64 plan, best_traj rounded once to f32 on the device (3.3 MB instead of 6.6 MB down)"},
            "all_fp64": {"p50_ms": f50, "p95_ms": f95},
            "all_fp64_branch_and_bound": {"p50_ms": b50, "p95_ms": b95, "note": "cfg.prune = 1 under f1p_lattice_set_mode(0): bit-identical outputs"},
            "config1_single_ego": {"p50_ms": s50, "p95_ms": s95, "workload": f"1 ego x 512 candidates x {S} stations (BASELINE configs[1]), Context.lattice_plan",
                                   "reused_page_locked_arrays": {"p50_ms": u50, "p95_ms": u95, "note": "reuse_outputs=True: results in the context's page-locked arrays instead of fresh numpy arrays"}}}


def leg_other_schedules(ctx, args, cfg, d_poses, d_prev_in, E, C, S, ref):
    """The same plan by the other schedules, every one checked bit for bit against the chain's plan (same previous path):
      all_fp64          the plain kernel (one fp64 thread per candidate; round 1's headline kernel)
      branch_and_bound  all fp64 with cfg.prune = 1 (station loops skipped while a cost lower bound exceeds the best so far)
      every_station     the default schedule with f1p_lattice_set_clearance(0): no clearance map, every station of a looked-at candidate tested on the bitmap
    `ref` = (bidx, ref_cost, steer, ref_traj) of the chain's plan.  Returns (fp64, bnb, every_station)."""
    import copy
    import numpy as np
    bidx, ref_cost, steer, ref_traj = ref
    alt = [ctx.alloc(8 * E), ctx.alloc(8 * E), ctx.alloc(4 * E), ctx.alloc(8 * E), ctx.alloc(4 * E), ctx.alloc(4 * E), ctx.alloc(8 * E * S * 4)]

    def other(cfg_x, mode):
        ctx.lattice_set_mode(mode)
        for _ in range(args.warmup):
            ctx.lattice_plan_dev(d_poses, E, cfg_x, *alt, d_prev_theta=d_prev_in)
        ctx.sync()
        ctx.timer_begin()
        for _ in range(args.steps):
            ctx.lattice_plan_dev(d_poses, E, cfg_x, *alt, d_prev_theta=d_prev_in)
        ms = ctx.timer_end() / args.steps
        same = bool((alt[2].download(np.int32, (E,)) == bidx).all() and
                    np.array_equal(alt[3].download(np.float64, (E,)), ref_cost, equal_nan=True) and
                    np.array_equal(alt[0].download(np.float64, (E,)), steer) and
                    np.array_equal(alt[6].download(np.float64, (E, S, 4)), ref_traj))
        return {"kernel_ms": ms, "candidate_steps_per_s_equivalent": float(E) * C * S / (ms * 1e-3), "outputs_bit_identical_to_the_timed_plan": same}
    cfg_ex = copy.copy(cfg); cfg_ex.prune = 0
    cfg_bb = copy.copy(cfg); cfg_bb.prune = 1
    every_station = None
    fp64 = other(cfg_ex, 0)
    fp64["note"] = "f1p_lattice_set_mode(0): every candidate-step in fp64, one thread per candidate (k_lattice)"
    bnb = other(cfg_bb, 0)
    bnb["note"] = "all fp64 + cfg.prune = 1: candidates sorted by a lower bound of their cost after the fit; a station loop runs only while the bound does not exceed the best cost found"
    if not (args.all_fp64 or args.prune):
        ctx.lattice_set_clearance(0)
        every_station = other(cfg_ex, 1)
        every_station["note"] = ("the default schedule with f1p_lattice_set_clearance(0) -- no clearance map: every look of the lazy station pass is the "
                                 "every-station one (49 single-interval pieces, 50 look-ups on the real bitmap for each candidate that can still win).  Until the end "
                                 "of round 5 this ran the one-kernel fallback filter, every station of EVERY candidate (0.137 ms); that kernel is gone")
        ctx.lattice_set_clearance(2)
    ctx.lattice_set_mode(0 if (args.all_fp64 or args.prune) else 1)
    for b_ in alt:
        b_.free()
    return fp64, bnb, every_station


def leg_kernel_profile(ctx, step, d_prev_in, n, E, C):
    """per-kernel durations of the default schedule (HIP events between its kernels, outside the timed region), same previous path; and the
    entries per ego the filter of that last plan handed to the fp64 refinement"""
    import numpy as np
    ctx.lattice_profile(True)
    acc = np.zeros(4)
    for _ in range(n):
        step(d_prev_in)
        acc += np.array(ctx.lattice_profile(True, read=True))
    ctx.lattice_profile(False)
    acc /= n
    mixed_ms = {"k_lattice_prologue": float(acc[0]), "k_lattice_filter3": float(acc[1]), "k_lattice_refine": float(acc[2]), "k_lattice_select": float(acc[3])}
    try:
        nq = ctx.lattice_debug_queue(E)
        pass_stat = {"mean": float(nq.mean()), "p99": float(np.percentile(nq, 99)), "max": int(nq.max()), "of": C,
                     "note": "entries per ego handed to the fp64 refinement (scene_sweep counts the station pass itself: f1p_lattice_debug_pass)"}
    except Exception as exc:   # noqa: BLE001 -- a statistic, not a gate
        pass_stat = {"error": str(exc)}
    return mixed_ms, pass_stat


def leg_audit(ctx, step, d_prev_in, n_aud, E):
    """runtime audit of the mixed schedule (f1p_lattice_set_audit): the timed plan again, every plan followed by the all-fp64 exhaustive
    kernel on a moving window of 256 egos and a bit-for-bit comparison of every output; outside the timed region"""
    ctx.lattice_audit_read(reset=True)
    ctx.lattice_set_audit(1, min(256, E))
    for _ in range(n_aud):
        step(d_prev_in)
    audit = ctx.lattice_audit_read(reset=True)
    ctx.lattice_set_audit(0)
    audit["note"] = ("every audited plan (similarity term live): all-fp64 exhaustive kernel (cfg.prune = 0) on a moving 256-ego window, all seven outputs "
                     "compared bit for bit; mismatching_egos must be 0")
    return audit


def lattice_valu_and_traffic(args, E, C, S, mixed_ms, kernel_ms, cand_sharded):
    """The dominant kernel's issue-slot figures and the plan's HBM traffic, from the newest committed PMC profile of this configuration
    (parsed at run time: no pasted constants).  Returns (dom_ms, pmc, same_cfg, valu, traffic)."""
    dom_ms = mixed_ms["k_lattice_filter3"] if mixed_ms else kernel_ms         # the dominant kernel's own average duration
    pmc = load_pmc({"egos": E, "cands": C, "stations": S, "workload": args.workload, "generator": args.generator,
                    "schedule": "all_fp64" if args.all_fp64 else ("bnb" if args.prune else "mixed")})
    same_cfg = bool(pmc and not cand_sharded)
    valu = None
    if same_cfg and pmc.get("SQ_INSTS_VALU") and pmc.get("waves"):
        per_cand = pmc["SQ_INSTS_VALU"] / pmc["waves"]            # wave-instructions per wave = lane-instructions per candidate (one lane per candidate)
        valu_tlanes = per_cand * E * C / (dom_ms * 1e-3) / 1e12
        f32_kernel = not (args.all_fp64 or args.prune)
        peak = VALU_PEAK_F32_GUIDE if f32_kernel else VALU_PEAK_SLOW_CLASS
        valu = {"kernel": pmc["kernel"], "achieved": valu_tlanes, "peak": peak, "unit": "T lane-instr/s",
                "frac": valu_tlanes / peak,
                "peak_definition": ("MI355X_MICROARCH.md: SIMD-32, one wave64 f32 VALU instruction per 2 cycles at 2.4 GHz (157.3 TFLOP/s of FMA)" if f32_kernel else
                                    "measured: one fp64 VALU instruction per wave per 4.3 cycles (profiles/r03_valu_issue_cycles.txt)"),
                "arithmetic": "f64" if not f32_kernel else "f32 (the candidate kernel; prologue, refinement and selection after it are fp64 and latency-bound)",
                "valu_instr_per_candidate": per_cand, "source": pmc["source"]}
        if f32_kernel:
            # the same achieved rate against what the chip measurably issues, and against the issue-cycle floor of THIS kernel's own
            # instruction mix (transcendentals at 8.3 cycles, everything else priced at the cheapest class: a lower bound of its time)
            valu["frac_of_measured_f32_issue_peak"] = valu_tlanes / VALU_PEAK_F32_MEASURED
            valu["measured_f32_issue_peak"] = VALU_PEAK_F32_MEASURED
            # instruction classes of the kernel's own stream (gfx950's per-class counters; whatever they do not name -- min / max / compare /
            # select / bit operations / DPP moves / readlane -- is "other")
            cls = {k: pmc[n] / pmc["waves"] for k, n in (("add_f32", "SQ_INSTS_VALU_ADD_F32"), ("mul_f32", "SQ_INSTS_VALU_MUL_F32"), ("fma_f32", "SQ_INSTS_VALU_FMA_F32"),
                                                          ("trans_f32", "SQ_INSTS_VALU_TRANS_F32"), ("cvt", "SQ_INSTS_VALU_CVT"), ("int32", "SQ_INSTS_VALU_INT32"),
                                                          ("add_f64", "SQ_INSTS_VALU_ADD_F64"), ("mul_f64", "SQ_INSTS_VALU_MUL_F64"), ("fma_f64", "SQ_INSTS_VALU_FMA_F64"),
                                                          ("trans_f64", "SQ_INSTS_VALU_TRANS_F64"), ("int64", "SQ_INSTS_VALU_INT64")) if pmc.get(n) is not None}
            if cls:
                cls["other"] = per_cand - sum(cls.values())
                valu["instr_classes_per_candidate"] = cls
            if pmc.get("SQ_INSTS_VALU_TRANS_F32") is not None:
                trans = pmc["SQ_INSTS_VALU_TRANS_F32"] / pmc["waves"]
                floor_cyc = (per_cand - trans) * VALU_CYC["fast"] + trans * VALU_CYC["trans"]
                floor_ms = floor_cyc * (E * C / 64.0) / 1024.0 / 2.4e9 * 1e3
                valu["trans_instr_per_candidate"] = trans
                valu["issue_floor_ms_of_this_mix"] = floor_ms
                valu["frac_of_issue_floor"] = floor_ms / dom_ms
            # both filter kernels together (the prologue runs one wave per EGO: its instructions are spread over the ego's candidates)
            pro = [k for k in pmc.get("all_kernels", []) if "k_lattice_prologue" in k.get("kernel", "")]
            if pro and pro[0].get("SQ_INSTS_VALU") and pro[0].get("waves"):
                valu["valu_instr_per_candidate_incl_prologue"] = per_cand + pro[0]["SQ_INSTS_VALU"] / pmc["waves"]
        if pmc.get("SQ_ACTIVE_INST_VALU") and pmc.get("GRBM_GUI_ACTIVE"):
            # SQ_ACTIVE_INST_VALU counts quad-cycles summed over the SIMDs; GRBM_GUI_ACTIVE sums the 8 XCDs' busy clocks
            valu["busy_frac_profiled"] = pmc["SQ_ACTIVE_INST_VALU"] * 4.0 / (1024.0 * pmc["GRBM_GUI_ACTIVE"] / 8.0)
    traffic = None
    if same_cfg:
        # one plan = every kernel of the schedule (the filter reads the scene, k_lattice_select writes best_traj): their PMC bytes are summed
        names = ("k_lattice_prologue", "k_lattice_filter3", "k_lattice_refine", "k_lattice_select") if mixed_ms else (pmc["kernel"],)
        tb = 0.0
        for k in pmc.get("all_kernels", []):
            if any(nm in k.get("kernel", "") for nm in names) and k.get("FETCH_SIZE_KiB") is not None and k.get("WRITE_SIZE_KiB") is not None:
                tb += (k["FETCH_SIZE_KiB"] * 2 + k["WRITE_SIZE_KiB"]) * 1024    # gfx950 wide-read correction x2 (MI355X_MICROARCH.md)
        traffic = int(tb) if tb > 0 else None
    return dom_ms, pmc, same_cfg, valu, traffic


def leg_cpu_baseline_and_parity(args, out, poses, rl, cfg, img, res, origin, E, C, S, world, prev_in, bidx, steer, materialised):
    """rank 0: the oracle (`kind: "port"`, OpenMP over egos on all host threads) on a bounded sample of the same workload -- the run's parity
    gate and its CPU baseline -- and north_star's single-core numpy baseline"""
    import numpy as np
    from oracle import oracle   # the checker / CPU baseline leg only
    nthr = oracle.max_threads()
    grid = (img, res, origin[0], origin[1], 206)
    n_cpu = args.cpu_egos
    if world > 1:
        n_cpu = min(E, 256)                       # N > 1: parity gate only; the CPU baseline is an N = 1 figure
    if n_cpu <= 0:
        t1 = time.perf_counter()
        oracle.lattice_plan_batch(poses[:nthr], rl, cfg, grid=grid, prev_theta=None if prev_in is None else prev_in[:nthr], nthreads=nthr)
        per_ego = (time.perf_counter() - t1) / nthr
        n_cpu = int(min(E, max(nthr, (12.0 / max(per_ego, 1e-6)) // nthr * nthr)))
    t1 = time.perf_counter()
    want = oracle.lattice_plan_batch(poses[:n_cpu], rl, cfg, grid=grid, prev_theta=None if prev_in is None else prev_in[:n_cpu], nthreads=nthr)
    cpu_s = time.perf_counter() - t1
    mism = int((want["best_idx"] != bidx[:n_cpu]).sum())
    dsteer = float(np.abs(want["steer"] - steer[:n_cpu]).max())
    out["cpu_baseline"] = None if world > 1 else {
        "value": n_cpu * C * S / cpu_s, "unit": "candidate-trajectory-steps/s", "cores": nthr, "kind": "port",
        "sample": f"first {n_cpu} of the {E} egos x {C} candidates x {S} stations, oracle/f1p_oracle.c "
                  f"(fp64 C, OpenMP over egos, {nthr} threads), {cpu_s:.1f} s",
        "note": "the oracle follows the reference's per-station X(s)/Y(s) evaluation (utils.py:289-293): every station is integrated "
                "from 0, O(S^2) per candidate -- a faithful restatement, not a tuned CPU implementation; the GPU/CPU ratio is no credit"}
    out["parity"] = {"egos_checked": n_cpu, "best_idx_mismatches": mism, "max_abs_dsteer": dsteer,
                     "checked_outputs": "the plan of the closed-loop chain right after the timed region (its previous path handed to the oracle)",
                     "similarity_term_live": prev_in is not None}
    if world == 1 and args.generator == "clothoid" and not materialised and os.path.exists(os.path.join(ROOT, "oracle", "numpy_lattice.py")):
        out["cpu_baseline_numpy"] = numpy_baseline(poses, rl, cfg, grid, C, S, bidx, steer, prev_in=prev_in)


def main_lattice(args):
    import numpy as np
    from f1tenth_planning_amd import _abi, synth
    rk = Ranks()
    rank, world = rk.rank, rk.world
    E, C, S = args.egos, args.cands, args.stations
    cfg = synth.bench_lattice_cfg(n_cand=C, n_stations=S, generator=args.generator, prune=args.prune)
    rl = synth.make_raceline(seed=0)
    res = 0.058
    img, origin = synth.make_grid(rl[:, :2], size=(2000, 2000), resolution=res)
    cand_sharded = args.shard == "candidates"
    poses = synth.make_egos(rl, E, seed=1 + (0 if cand_sharded else rank))     # ego-sharded: every rank plans its own egos

    ctx = rk.open_context()
    ctx.set_waypoints(rl)
    ctx.set_grid(img, res, origin, 206)
    if args.all_fp64 or args.prune:
        ctx.lattice_set_mode(0)
    rk.init()
    materialised = args.workload == "lattice-materialised"
    secondary = not args.no_secondary and not materialised and args.generator == "clothoid"
    if secondary or cand_sharded:
        rk.init_rccl(ctx, fatal=cand_sharded)

    d_poses = ctx.to_device(poses)
    d_steer, d_speed = ctx.alloc(8 * E), ctx.alloc(8 * E)
    d_bidx, d_bcost, d_status, d_near = ctx.alloc(4 * E), ctx.alloc(8 * E), ctx.alloc(4 * E), ctx.alloc(4 * E)
    d_traj = ctx.alloc(8 * E * S * 4)
    d_all_cost = ctx.alloc(8 * E * C) if materialised else None
    d_all_traj = ctx.alloc(8 * E * C * S * 4) if materialised else None   # the reference's all_traj data flow (:194-201)

    # Steady state (round 4): the reference's fourth cost, get_similarity_cost (lattice_planner.py:287-296), compares with the PREVIOUS
    # plan's best trajectory, so every plan of a closed loop but the first carries it.  Closed-loop mode keeps the winners' headings on
    # the device (f1p_lattice_set_closed_loop): every timed plan k uses plan k-1's winners as its previous path.  `value` is THIS
    # figure; the first plan of a chain (no previous path: the term is zero, round 3's headline) is timed beside it as `first_plan`.
    steady = not materialised
    ctx.lattice_set_closed_loop(steady)

    lat = None
    if args.latency_iters > 0 and not materialised and not cand_sharded:
        lat = leg_host_boundary_latency(ctx, args, poses, cfg, S, steady)

    cs = None
    if cand_sharded:
        cs, step, cs_exchange = leg_candidate_sharded(rk, ctx, rl, args.steps, E=E, C=C, S=S, timed=False)
    else:
        def step(d_prev=None):
            ctx.lattice_plan_dev(d_poses, E, cfg, d_steer, d_speed, d_bidx, d_bcost, d_status, d_near, d_traj,
                                 d_prev_theta=d_prev, d_all_cost=d_all_cost, d_all_traj=d_all_traj)

    elapsed, kernel_ms_total = timed_region(rk, ctx, step, args.warmup, args.steps)
    per_rank_s = list(rk.last_per_rank_s or [elapsed])
    if args.dump_outputs and rank == 0:                         # before the parity plan below overwrites them
        if cand_sharded:
            dumped = step.outputs()
        else:
            dumped = {"steer": d_steer.download(np.float64, (E,)), "speed": d_speed.download(np.float64, (E,)),
                      "best_idx": d_bidx.download(np.int32, (E,)), "best_cost": d_bcost.download(np.float64, (E,)),
                      "status": d_status.download(np.int32, (E,)), "near_idx": d_near.download(np.int32, (E,)),
                      "best_traj": d_traj.download(np.float64, (E, S, 4))}
            if materialised:
                dumped.update(all_cost=d_all_cost.download(np.float64, (E, C)), all_traj=d_all_traj.download(np.float64, (E, C, S, 4)))
        dump_outputs(args.dump_outputs, dumped)

    # outputs the parity gate and the other schedules are compared with: ONE more plan of the chain, whose previous path (the headings the
    # last timed plan left) is copied first so that every comparison below can hand it over explicitly
    d_prev_in = prev_in = None
    if cand_sharded:
        steer = bidx = status = None
        cs_exchange(min(args.steps, 50))
    else:
        if steady:
            prev_in = ctx.lattice_closed_loop_prev()
            d_prev_in = ctx.to_device(prev_in)
            step()
            ctx.sync()
            ctx.lattice_set_closed_loop(False)                    # from here on the previous path is explicit (d_prev_in)
        steer = d_steer.download(np.float64, (E,)); bidx = d_bidx.download(np.int32, (E,)); status = d_status.download(np.int32, (E,))
        ref_cost = d_bcost.download(np.float64, (E,)); ref_traj = d_traj.download(np.float64, (E, S, 4))

    # the first plan of a chain: no previous path, the similarity term is zero (what rounds 1-3 timed)
    first_plan = None
    if steady and not cand_sharded and not args.only_timed:
        e1, k1 = timed_region(rk, ctx, step, min(args.warmup, 5), args.steps)
        first_plan = {"ms_per_step": e1 / args.steps * 1e3, "kernel_ms": k1 / args.steps, "value": float(E) * C * S * args.steps * world / e1,
                      "note": "closed loop off, prev_theta = NULL: w_similarity multiplies 0 (rounds 1-3 timed this)"}

    bnb = fp64 = every_station = None
    if rank == 0 and not materialised and args.generator == "clothoid" and not cand_sharded and not args.only_timed:
        fp64, bnb, every_station = leg_other_schedules(ctx, args, cfg, d_poses, d_prev_in, E, C, S, (bidx, ref_cost, steer, ref_traj))

    mixed_ms = pass_stat = audit = None
    if rank == 0 and not (args.all_fp64 or args.prune or materialised or cand_sharded or args.only_timed) and args.generator == "clothoid" and E >= 512:
        mixed_ms, pass_stat = leg_kernel_profile(ctx, step, d_prev_in, max(10, min(args.steps, 50)), E, C)
        audit = leg_audit(ctx, step, d_prev_in, max(20, min(args.steps, 64)), E)

    # the headline workload on scenes it was NOT tuned on: wall-hugging egos, obstacles on the raceline, a moving fleet
    scene_sweep = None
    if rank == 0 and world == 1 and secondary and not (args.all_fp64 or args.prune or cand_sharded or args.only_timed) and E >= 512:
        scene_sweep = leg_scene_sweep(rl, img, res, origin, cfg, E, C, S, max(20, min(args.steps, 100)), device=rk.local_rank)

    variants = None
    if rank == 0 and world == 1 and secondary and not (args.all_fp64 or args.prune or cand_sharded or args.only_timed) and E >= 512:
        variants = leg_variants(rk, rl, img, res, origin, E, C, S, max(20, min(args.steps, 100)))

    env_ok = rk.env_ok()
    selftest = kmpc_c4 = None
    if secondary and not cand_sharded and rk.rccl_ok:
        cs, _, _ = leg_candidate_sharded(rk, ctx, rl, max(10, min(args.steps, 100)))
    if (secondary or cand_sharded) and rk.rccl_ok:
        selftest = leg_exchange_selftest(rk, ctx)
    elif not rk.rccl_ok:
        selftest = {"skipped": rk.rccl_note}
    # (before any leg that runs the OpenMP oracle: its worker threads spin for a while after a parallel region and would compete with the
    # thread that issues these launches -- seen once as 0.40 ms per plan instead of 0.07)
    two_in_flight = None
    if secondary and not cand_sharded and not (args.all_fp64 or args.prune):
        two_in_flight = leg_two_plans_in_flight(rk, rl, img, res, origin, poses, cfg, E, C, S, max(20, min(args.steps, 200)))
    kmpc_s8192 = pursuit = None
    if secondary and not cand_sharded:
        kmpc_c4 = leg_kmpc_c4(rk, args, max(10, min(args.steps, 100)))
        if rank == 0 and world == 1 and not args.only_timed:
            kmpc_s8192 = leg_kmpc_stream8192(rk, args)
            if not args.no_cpu_baseline:
                pursuit = leg_pursuit(rk, rl)

    if rank == 0:
        steps_total = float(E) * C * S * args.steps * (1 if cand_sharded else world)
        value = steps_total / elapsed
        kernel_ms = kernel_ms_total / args.steps
        abytes = algorithmic_bytes_lattice(E, C, S, rl.shape[0], img.shape[1], img.shape[0])
        if materialised:
            abytes += E * C * S * 32 + E * C * 8      # every candidate's rows (x, y, theta, |kappa|) + its cost, written once
        dom_ms, pmc, same_cfg, valu, traffic = lattice_valu_and_traffic(args, E, C, S, mixed_ms, kernel_ms, cand_sharded)
        achieved_gbs = abytes / (kernel_ms * 1e-3) / 1e9              # the plan's algorithmic bytes over the plan's kernel time
        pcie_value = (float(E) * C * S / (lat["p50_ms"] * 1e-3)) if lat else None
        default_sched = not (args.all_fp64 or args.prune or materialised or args.generator != "clothoid")
        shape = filter_shape(S, 2) if default_sched else None
        if shape is not None and mixed_ms:
            shape["station_pass_candidates_per_ego"] = pass_stat
        # SURVEY 8d's op count, from the instrumented restatement (rank 0, a few seconds of pure Python)
        algo = None
        if default_sched and not cand_sharded and not args.no_cpu_baseline:
            algo = algorithmic_ops(poses, rl, cfg, (img, res, origin[0], origin[1], 206), prev_in)
            if algo and mixed_ms:
                ops_s = algo["ops_per_candidate"] * E * C / (dom_ms * 1e-3)
                algo["achieved_Tops_per_s_in_the_dominant_kernel"] = ops_s / 1e12
                algo["peak_Tops_per_s"] = 2.0 * VALU_PEAK_F32_GUIDE
                algo["achieved_over_peak"] = ops_s / 1e12 / (2.0 * VALU_PEAK_F32_GUIDE)
                algo["note"] = ("algorithmic ops of the CPU restatement per candidate x candidates / the candidate kernel's duration, against 157.3 T flop/s "
                                "(guide: f32 FMA = 2 flop per lane-instruction).  NOT an efficiency: k_lattice_filter3 reaches the same decisions with "
                                "far fewer operations (f32 fit on ONE 16-node pass, closed-form cost terms, positions and look-ups only for the ~1.5 candidates "
                                "per ego whose collision state can matter: see filter_shape and valu.valu_instr_per_candidate), so this ratio measures how much work "
                                "the algorithm removed as much as how fast the rest runs -- the issue-slot figure is roofline.frac")
        hbm = {"bound": "hbm", "achieved": achieved_gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved_gbs / HBM_PEAK_GBS,
               "algorithmic_bytes_per_launch": abytes, "bytes_per_candidate_step": abytes / (E * C * S),
               "note": ("the reference's all_traj data flow: every candidate's rows written once (32.3 B per candidate-step); the kernel also carries the full fp64 "
                        "evaluation; the store-only ceiling of this chip is 4.1-4.4 TB/s (tools/microbench/stream.hip), 3.9-4.0 for this kernel's 128-byte chunks"
                        if materialised else
                        "0.14 B per candidate-step: the planning kernels are not memory-bound; the HBM fraction is tiny and reported as such")}
        kernels_name = ("k_lattice_prologue + k_lattice_filter3 + k_lattice_refine + k_lattice_select (one plan; the dominant kernel is k_lattice_filter3)"
                        if mixed_ms else (pmc["kernel"] if pmc else "k_lattice"))
        if valu and not materialised:
            # SURVEY 8d / DESIGN 5: the fused lattice path is VALU-bound -- the top-level figures are the dominant kernel's issue-slot utilisation
            roofline = {"bound": "valu", "achieved": valu["achieved"], "peak": valu["peak"], "unit": valu["unit"], "frac": valu["frac"],
                        "frac_definition": "lane-instructions the dominant kernel ISSUES per second (PMC SQ_INSTS_VALU per candidate x candidates / its live duration) "
                                           "over the guide's issue peak: an issue-slot utilisation of the kernel's own instruction stream, not a fraction of an "
                                           "algorithmic bound (see algorithmic_ops_per_candidate for that count)"}
        else:
            roofline = dict(hbm)
        roofline.update({"traffic": traffic, "traffic_source": pmc["source"] if traffic is not None else None, "kernel": kernels_name,
                         "kernel_ms": kernel_ms, "dominant_kernel_ms": dom_ms, "kernels_ms": mixed_ms,
                         "kernels_ms_note": ("per-kernel figures come from a separate run with a HIP event between consecutive kernels; an event is a barrier "
                                             "packet of its own (~1.5-2 us each here), so their sum exceeds kernel_ms -- the unstamped plan of the timed "
                                             "region -- by the stamps, not because kernels overlap (one in-order stream).  "
                                             "profiled_kernels_us holds rocprofv3's own per-kernel averages from the committed trace") if mixed_ms else None,
                         "profiled_kernels_us": ({k["kernel"].split("(")[0].replace("void f1p::", "").replace("f1p::", ""): round(k["avg_us"], 2)
                                                  for k in pmc.get("all_kernels", []) if k.get("avg_us") and "lattice" in k.get("kernel", "")} if same_cfg else None),
                         "algorithmic_bytes_per_launch": abytes, "hbm": hbm, "valu": valu})
        steady_state = None
        if steady and not cand_sharded:
            steady_state = {"ms_per_step": elapsed / args.steps * 1e3, "kernel_ms": kernel_ms, "value": value,
                            "note": "closed loop: plan k's previous path = plan k-1's winners (device-resident headings); all four cost terms live"}
        out = {
            "metric": "candidate-trajectory-steps/sec per GPU; p50 plan() latency @4096 egos",
            "value": value, "unit": "candidate-trajectory-steps/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True,
            "scaling": "strong" if cand_sharded else "weak", "vs_baseline": None,
            "dtype": "f64" if not default_sched else "f32 filter + f64 decision", "data": "synthetic",
            "config": {"workload": (f"batched lattice, candidate-sharded: {E} egos x {C} candidates x {S} stations, candidates split over {world} GPU(s) + RCCL all-reduce(min)"
                                    if cand_sharded else
                                    f"batched lattice{' (all_traj materialised)' if materialised else ''}: {E} egos x {C} candidates x {S} stations per GPU (BASELINE configs[{3 if world == 8 and E == 4096 else 2}])"),
                       "egos_per_gpu": E, "candidates": C, "stations": S, "raceline_points": int(rl.shape[0]),
                       "grid": [int(img.shape[1]), int(img.shape[0])], "goals": "device-sampled 16 x %d" % (C // 16), "generator": args.generator,
                       "cost_terms": "1/L, max|kappa|, mean|kappa|, heading similarity to the previous plan's winner (weights 0.25 each) + occupancy => +inf",
                       "state": "steady state of a closed loop (similarity term live)" if steady else "single plans (no previous path)",
                       "parallelism": (f"one ego batch, candidates sharded over {world} GPU(s), RCCL all-reduce(min)" if cand_sharded
                                       else f"egos sharded over {world} GPU(s), no collective")},
            "value_definition": "E*C*S*steps*n_gpus / wall time of the K timed STEADY-STATE plans, inputs resident in HBM (kernel-only figure).  E*C*S is the "
                                "workload's NOMINAL size (BASELINE's unit): the default schedule does not evaluate every candidate-step literally (filter_shape); "
                                "all_fp64 is the schedule that does (every station of every candidate), timed beside it with bit-identical outputs; every_station is the default "
                                "schedule without its clearance map.  "
                                "The SURVEY 8d host-boundary figure (H2D + kernels + D2H + sync per plan) is pcie_inclusive_value / plan_latency_host_boundary",
            "per_gpu_value": value / (1 if cand_sharded else world),
            "steady_state": steady_state,
            "first_plan": first_plan,
            "pcie_inclusive_value": pcie_value,
            "plan_latency_host_boundary": lat,
            "schedule": ("all fp64" + (" + branch and bound" if args.prune else "")) if not default_sched else
                        ("k_lattice_prologue2 (fp64, two egos per wave: nearest segment, look-ahead centres, goal frames, moments of the previous path) -> "
                         "k_lattice_filter3 (f32, thread per candidate: G1 fit on one 16-node pass, closed-form curvature and similarity terms, cost "
                         "bracket; then the station pass -- integrated pieces + clearance look-ups per filter_shape, a wave per selected candidate -- "
                         "for the few candidates whose bracket reaches below the best collision-free one) -> k_lattice_refine (fp64, the reference's "
                         "arithmetic on the ~1.5 candidates per ego the brackets cannot rank) -> k_lattice_select (fp64 argmin, winner's rows, tracker); "
                         "outputs bit-identical to the all-fp64 kernel"),
            "filter_shape": shape,
            "algorithmic_ops_per_candidate": algo,
            "all_fp64": fp64,
            "branch_and_bound": bnb,
            "every_station": every_station,
            "candidate_sharded": cs,
            # top level for multi-GPU runs: the communicator's own rank count and the exchange alone (HIP events around the two
            # collectives + the two key kernels).  At one rank the "exchange" is a local self-reduce: no xGMI figure.
            "rccl_ranks": None if cs is None else cs.get("rccl_ranks"),
            "exchange_us_p50": None if cs is None else cs.get("exchange_us_p50"),
            "multi_process_env": {"HSA_ENABLE_IPC_MODE_LEGACY": os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY"), "zero_on_every_rank": bool(env_ok)},
            "exchange_selftest": selftest,
            "kmpc_c4": kmpc_c4,
            "kmpc_stream8192": kmpc_s8192,
            "pure_pursuit_65536": pursuit,
            "two_plans_in_flight": two_in_flight,
            "audit": audit,
            "scene_sweep": scene_sweep,
            "variants": variants,
            "per_rank_ms_per_step": {"min": min(per_rank_s) / args.steps * 1e3, "max": max(per_rank_s) / args.steps * 1e3, "ranks": len(per_rank_s),
                                     "note": "wall time of the timed region on every rank / steps: ego sharding has no collective, so launch skew between the ranks is all it can lose"},
            "roofline": roofline,
            "blocked_egos": None if status is None else int((status == _abi.ST_ALL_BLOCKED).sum()),
        }
        # every number README / DESIGN quote, as top-level scalars: the driver's record keeps top-level keys and truncates nested objects
        def _g(d, *ks):
            for k in ks:
                if not isinstance(d, dict) or d.get(k) is None:
                    return None
                d = d[k]
            return d
        out.update({
            "steady_state_ms_per_plan": _g(steady_state, "ms_per_step"), "first_plan_ms_per_plan": _g(first_plan, "ms_per_step"),
            "every_station_ms": _g(every_station, "kernel_ms"), "every_station_value": _g(every_station, "candidate_steps_per_s_equivalent"),
            "all_fp64_ms": _g(fp64, "kernel_ms"), "all_fp64_value": _g(fp64, "candidate_steps_per_s_equivalent"),
            "branch_and_bound_ms": _g(bnb, "kernel_ms"),
            "other_schedules_bit_identical": None if fp64 is None else bool(all(x is None or x["outputs_bit_identical_to_the_timed_plan"] for x in (fp64, bnb, every_station))),
            "host_boundary_p50_ms": _g(lat, "p50_ms"), "host_boundary_f32_traj_p50_ms": _g(lat, "f32_best_traj", "p50_ms"),
            "host_boundary_no_traj_p50_ms": _g(lat, "without_best_traj", "p50_ms"), "closed_loop_step_p50_ms": _g(lat, "closed_loop", "p50_ms"),
            "config1_single_ego_p50_ms": _g(lat, "config1_single_ego", "p50_ms"),
            "two_plans_in_flight_ms_per_plan": _g(two_in_flight, "ms_per_plan"),
            "kernel_ms_prologue": _g(mixed_ms, "k_lattice_prologue"), "kernel_ms_filter3": _g(mixed_ms, "k_lattice_filter3"),
            "kernel_ms_refine": _g(mixed_ms, "k_lattice_refine"), "kernel_ms_select": _g(mixed_ms, "k_lattice_select"),
            "valu_instr_per_candidate": _g(valu, "valu_instr_per_candidate"), "valu_frac_of_issue_floor": _g(valu, "frac_of_issue_floor"),
            "traffic_over_algorithmic_bytes": None if traffic is None else traffic / abytes,
            "audit_mismatching_egos": _g(audit, "mismatching_egos"),
            "candidate_sharded_ranks": _g(cs, "ranks"), "candidate_sharded_bit_identical": _g(cs, "bit_identical_to_unsharded_plan_on_every_rank"),
            "exchange_selftest_ok": _g(selftest, "matches_np_argmin_on_every_rank"), "hsa_ipc_env_zero_on_every_rank": bool(env_ok),
            "kmpc_c4_streamed_ms": _g(kmpc_c4, "ms_per_plan"), "kmpc_c4_generated_ms": _g(kmpc_c4, "generated_in_kernel", "ms_per_plan"),
            "kmpc_c4_cache_stream_frac": _g(kmpc_c4, "roofline", "frac"), "kmpc_c4_generated_roofline_frac": _g(kmpc_c4, "generated_in_kernel", "roofline", "frac"),
            "kmpc_stream8192_ms": _g(kmpc_s8192, "kernel_ms"), "kmpc_stream8192_hbm_frac": _g(kmpc_s8192, "roofline", "frac"),
            "kmpc_stream8192_shader_mhz": _g(kmpc_s8192, "shader_clock_mhz", "median"),
            "pursuit_65536_ms": _g(pursuit, "kernel_ms"), "pursuit_plans_per_s": _g(pursuit, "plans_per_s"), "pursuit_valu_issue_frac": _g(pursuit, "roofline", "frac"), "pursuit_near_idx_mismatches": _g(pursuit, "parity", "near_idx_mismatches"),
            "host_boundary_d2h_ms": (lat["p50_ms"] - lat["without_best_traj"]["p50_ms"]) if (lat and _g(lat, "without_best_traj", "p50_ms")) else None,
        })
        if variants:
            out.update({"host_goals_ms_per_plan": _g(variants, "host_goals", "ms_per_plan"), "host_goals_kernel_ms_filter3": _g(variants, "host_goals", "kernels_ms", "k_lattice_filter3"),
                        "host_goals_bit_identical": _g(variants, "host_goals", "outputs_bit_identical_to_all_fp64"),
                        "host_goals_oracle_mismatches": _g(variants, "host_goals", "oracle", "best_idx_mismatches"),
                        "cubic_ms_per_plan": _g(variants, "cubic", "ms_per_plan"), "cubic_all_fp64_ms_per_plan": _g(variants, "cubic", "all_fp64_ms_per_plan"),
                        "cubic_bit_identical": _g(variants, "cubic", "outputs_bit_identical_to_all_fp64"), "cubic_oracle_mismatches": _g(variants, "cubic", "oracle", "best_idx_mismatches"),
                        "footprint_ms_per_plan": _g(variants, "footprint", "ms_per_plan"), "footprint_all_fp64_ms_per_plan": _g(variants, "footprint", "all_fp64_ms_per_plan"),
                        "footprint_bit_identical": _g(variants, "footprint", "outputs_bit_identical_to_all_fp64"), "footprint_oracle_mismatches": _g(variants, "footprint", "oracle", "best_idx_mismatches"),
                        "materialised_ms_per_plan": _g(variants, "materialised", "ms_per_plan"), "materialised_hbm_frac": _g(variants, "materialised", "roofline", "frac")})
        if scene_sweep:
            out.update({"scene_sweep_worst_vs_centred": max(v["vs_centred"] for v in scene_sweep.values()),
                        "scene_sweep_all_bit_identical": bool(all(v["outputs_bit_identical_to_all_fp64"] for v in scene_sweep.values())),
                        "scene_sweep_oracle_mismatches": int(sum(v["oracle"]["best_idx_mismatches"] for v in scene_sweep.values())),
                        "scene_sweep_audit_mismatching_egos": int(sum(v["audit"]["mismatching_egos"] for v in scene_sweep.values()))})
            for nm, v in scene_sweep.items():
                out["scene_" + nm + "_ms_per_plan"] = v["ms_per_plan"]
        if not args.no_cpu_baseline and not cand_sharded:
            leg_cpu_baseline_and_parity(args, out, poses, rl, cfg, img, res, origin, E, C, S, world, prev_in, bidx, steer, materialised)
        if rk.rccl_note:
            out["rccl_init"] = rk.rccl_note
        emit(out, rk=rk)
    if rk.rccl_hung:                                     # a thread is still inside ncclCommInitRank: no orderly teardown through it
        rk.barrier()
        sys.stdout.flush(); sys.stderr.flush()
        os._exit(0)
    rk.close()
    ctx.close()


def numpy_baseline(poses, rl, cfg, grid, C, S, bidx, steer, budget_s=15.0, prev_in=None):
    """north_star's "same-box CPU numpy baseline": oracle/numpy_lattice.py, the path vectorised over E x C arrays in fp64 numpy.
    numpy's elementwise kernels are single-threaded -> 1 core (BLAS is not on the path; OMP/MKL threads are pinned to 1 anyway).
    Runs on a reduced ego count sized to the time budget; the per-step rate is size-independent above a few egos."""
    import numpy as np
    try:
        from threadpoolctl import threadpool_limits
    except ImportError:      # pragma: no cover
        threadpool_limits = None
    from oracle import numpy_lattice
    n0 = 8

    def run(n):
        t1 = time.perf_counter()
        r = numpy_lattice.lattice_plan_batch(poses[:n], rl, cfg, grid=grid, prev_theta=None if prev_in is None else prev_in[:n])
        return r, time.perf_counter() - t1
    if threadpool_limits:
        with threadpool_limits(limits=1):
            _, t = run(n0)
            n = int(max(n0, min(len(poses), budget_s / max(t / n0, 1e-6))))
            got, cpu_s = run(n)
    else:
        _, t = run(n0)
        n = int(max(n0, min(len(poses), budget_s / max(t / n0, 1e-6))))
        got, cpu_s = run(n)
    return {"value": n * C * S / cpu_s, "unit": "candidate-trajectory-steps/s", "cores": 1, "kind": "port",
            "sample": f"first {n} of the {len(poses)} egos x {C} candidates x {S} stations, oracle/numpy_lattice.py (numpy fp64, vectorised over E x C), "
                      f"{cpu_s:.1f} s; reduced ego count, rate is per candidate-step (no extrapolation needed)",
            "best_idx_mismatches_vs_gpu": int((got["best_idx"] != bidx[:n]).sum()),
            "max_abs_dsteer_vs_gpu": float(np.abs(got["steer"] - steer[:n]).max())}


def main_pursuit(args):
    """Secondary line: batched pure pursuit (BASELINE configs[0] run for many egos): K1 nearest segment with chunk pruning
    + K2 look-ahead + actuation, 24 B in / 28 B out per ego; fp64-VALU bound."""
    import numpy as np
    from f1tenth_planning_amd import synth
    rk = Ranks()
    E = args.egos if args.egos != 4096 else 65536
    rl = synth.make_raceline(seed=0)
    poses = synth.make_egos(rl, E, seed=1 + rk.rank)[:, :3]
    ctx = rk.open_context()
    ctx.set_waypoints(rl)
    rk.init()
    d_poses = ctx.to_device(poses)
    d_steer, d_speed, d_near, d_la, d_st = ctx.alloc(8 * E), ctx.alloc(8 * E), ctx.alloc(4 * E), ctx.alloc(4 * E), ctx.alloc(4 * E)

    def step():
        ctx.pure_pursuit_dev(d_poses, E, 0.8, d_steer, d_speed, d_near, d_la, d_st)
    elapsed, ms_total = timed_region(rk, ctx, step, args.warmup, args.steps)
    kernel_ms = ms_total / args.steps
    if args.dump_outputs and rk.rank == 0:
        dump_outputs(args.dump_outputs, {"steer": d_steer.download(np.float64, (E,)), "speed": d_speed.download(np.float64, (E,)),
                                         "near_idx": d_near.download(np.int32, (E,)), "la_idx": d_la.download(np.int32, (E,)),
                                         "status": d_st.download(np.int32, (E,))})
    if rk.rank == 0:
        out = {"metric": "ego-plans/sec (batched pure pursuit)", "value": E * args.steps * rk.world / elapsed, "unit": "plans/s", "n_gpus": rk.world,
               "steps": args.steps, "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True,
               "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
               "config": {"workload": f"pure pursuit: {E} egos per GPU on a {len(rl)}-point raceline (BASELINE configs[0], batched)"},
               "kernel_ms": kernel_ms, "roofline": pursuit_valu_roofline(kernel_ms, E)}
        if not args.no_cpu_baseline:
            from oracle import oracle
            n_cpu = min(E, 65536)
            t1 = time.perf_counter()
            want = oracle.pure_pursuit_batch(poses[:n_cpu], rl, 0.8, nthreads=oracle.max_threads())
            cpu_s = time.perf_counter() - t1
            near = d_near.download(np.int32, (E,))[:n_cpu]
            steer = d_steer.download(np.float64, (E,))[:n_cpu]
            out["cpu_baseline"] = {"value": n_cpu / cpu_s, "unit": "plans/s", "cores": oracle.max_threads(), "kind": "port",
                                   "sample": f"{n_cpu} egos, oracle/f1p_oracle.c orc_pure_pursuit_batch"}
            out["parity"] = {"egos_checked": int(n_cpu), "near_idx_mismatches": int((near != want["near_idx"]).sum()),
                             "max_abs_steer_diff": float(np.abs(steer - want["steer"]).max())}
        emit(out, rk=rk)
    rk.close()
    ctx.close()


def main_stmpc(args):
    """Secondary line: random shooting on the dynamic single-track model: E egos x 512 rollouts x 40 steps
    of 0.025 s, fp64, controls (steering speed, acceleration) streamed from HBM as f32 [E][T][2][R]."""
    import numpy as np
    from f1tenth_planning_amd import _abi, synth
    rk = Ranks()
    E = args.egos if args.egos != 4096 else 1024
    T, R = (args.horizon if args.horizon != 30 else 40), args.rollouts
    cfg = _abi.stmpc_cfg(horizon=T, n_rollouts=R)
    cl = synth.make_centerline(seed=2)
    rng = np.random.default_rng(12 + rk.rank)
    k = rng.integers(0, len(cl) - 1, E)
    v = rng.uniform(2.5, 5.5, E)
    x0 = np.column_stack([cl[k, 1] + rng.normal(0, 0.1, E), cl[k, 2] + rng.normal(0, 0.1, E), rng.normal(0, 0.05, E), v,
                          cl[k, 3] + rng.normal(0, 0.1, E), rng.normal(0, 0.2, E), rng.normal(0, 0.02, E)])
    ctx = rk.open_context()
    ctx.set_waypoints(cl, cols=(1, 2, 5, 3))
    rk.init()
    ref = ctx.stmpc_ref(x0[:, [0, 1, 3, 4]], T)
    ctrl = np.empty((E, T, 2, R), dtype=np.float32)
    ctrl[:, :, 0, :] = np.clip(rng.normal(0, 1.5, (E, T, R)), -3.2, 3.2)
    ctrl[:, :, 1, :] = np.clip(rng.normal(0, 1.5, (E, T, R)), -3.0, 3.0)
    d_x0, d_ref, d_ctrl = ctx.to_device(x0), ctx.to_device(ref), ctx.to_device(ctrl)
    d_steer, d_speed, d_bi, d_bc = ctx.alloc(8 * E), ctx.alloc(8 * E), ctx.alloc(4 * E), ctx.alloc(8 * E)

    def step():
        ctx.stmpc_shoot_dev(d_x0, d_ref, d_ctrl, E, cfg, d_steer, d_speed, d_bi, d_bc)
    elapsed, ms_total = timed_region(rk, ctx, step, args.warmup, args.steps)
    kernel_ms = ms_total / args.steps
    if args.dump_outputs and rk.rank == 0:
        dump_outputs(args.dump_outputs, {"steer": d_steer.download(np.float64, (E,)), "speed": d_speed.download(np.float64, (E,)),
                                         "best_idx": d_bi.download(np.int32, (E,)), "best_cost": d_bc.download(np.float64, (E,))})
    # the all-fp64 kernel (k_stmpc_shoot) on the same inputs: same outputs bit for bit (tests/test_gpu_stmpc.py), here only timed
    bi_mixed = d_bi.download(np.int32, (E,))
    ctx.stmpc_set_mode(False)
    for _ in range(3): step()
    ctx.sync(); ctx.timer_begin()
    for _ in range(20): step()
    fp64_ms = ctx.timer_end() / 20
    same_idx = bool(np.array_equal(d_bi.download(np.int32, (E,)), bi_mixed))
    ctx.stmpc_set_mode(True)
    step(); ctx.sync()
    if rk.rank == 0:
        abytes = E * R * T * 8 + E * (T + 1) * 56 + E * 56 + E * 28
        out = {"metric": "rollout-steps/sec (dynamic single-track random shooting)", "value": float(E) * R * T * args.steps * rk.world / elapsed,
               "unit": "rollout-steps/s", "n_gpus": rk.world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3,
               "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32 filter + f64 decision, f32 controls", "data": "synthetic",
               "config": {"workload": f"stmpc shooting: {E} egos x {R} rollouts x {T} steps per GPU (SURVEY.md 8f rank 2)"},
               "roofline": {"bound": "hbm", "achieved": abytes / (kernel_ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                            "frac": abytes / (kernel_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, "traffic": None,
                            "kernel": "k_stmpc_filter + k_stmpc_refine + k_stmpc_decide (one plan)", "kernel_ms": kernel_ms},
               "all_fp64": {"kernel": "k_stmpc_shoot", "kernel_ms": fp64_ms, "speedup": fp64_ms / kernel_ms, "same_best_idx": same_idx}}
        pmc = load_pmc({"workload": "stmpc", "egos": E, "rollouts": R, "horizon": T})
        if pmc and pmc.get("SQ_INSTS_VALU") and pmc.get("avg_us"):
            # the dominant kernel (k_stmpc_filter) against ITS OWN profiled duration: the plan's other two kernels are fp64 latency chains
            tl = pmc["SQ_INSTS_VALU"] * 64.0 / (pmc["avg_us"] * 1e-6) / 1e12
            out["roofline"]["valu"] = {"kernel": pmc["kernel"], "kernel_us_profiled": pmc["avg_us"], "achieved": tl, "peak": VALU_PEAK_F32_GUIDE,
                                       "unit": "T lane-instr/s", "frac": tl / VALU_PEAK_F32_GUIDE,
                                       "frac_of_measured_f32_issue_peak": tl / VALU_PEAK_F32_MEASURED,
                                       "valu_instr_per_rollout_step": pmc["SQ_INSTS_VALU"] * 64.0 / (E * R * T), "source": pmc["source"]}
            tr = 0
            for kk in pmc.get("all_kernels", []):
                if any(n in kk.get("kernel", "") for n in ("k_stmpc_filter", "k_stmpc_refine", "k_stmpc_decide")) and kk.get("FETCH_SIZE_KiB") is not None:
                    tr += (kk["FETCH_SIZE_KiB"] * 2 + kk.get("WRITE_SIZE_KiB", 0.0)) * 1024
            if tr:
                out["roofline"]["traffic"] = int(tr)
                out["roofline"]["traffic_source"] = pmc["source"]
        if not args.no_cpu_baseline:
            from oracle import oracle
            nthr = oracle.max_threads()
            n_cpu = min(E, max(nthr, 256))
            t1 = time.perf_counter()
            want = oracle.stmpc_shoot_batch(x0[:n_cpu], ref[:n_cpu], ctrl[:n_cpu], cfg, nthreads=nthr)
            cpu_s = time.perf_counter() - t1
            bi = d_bi.download(np.int32, (E,))[:n_cpu]
            out["cpu_baseline"] = {"value": float(n_cpu) * R * T / cpu_s, "unit": "rollout-steps/s", "cores": nthr, "kind": "port",
                                   "sample": f"{n_cpu} egos, oracle/f1p_oracle.c orc_stmpc_shoot_batch"}
            out["parity"] = {"egos_checked": int(n_cpu), "best_idx_mismatches": int((bi != want["best_idx"]).sum())}
        emit(out, rk=rk)
    rk.close()
    ctx.close()


def main_kmpc(args):
    """Secondary line: kinematic-MPC random shooting (BASELINE configs[4]: 1024 egos x 512 rollouts x 30 steps IN TOTAL over the
    N GPUs, i.e. 1024 / N egos per GPU; `--egos` overrides the total).  The controls stream from HBM (8 B per rollout-step):
    HBM roofline."""
    import numpy as np
    from f1tenth_planning_amd.dist import shard_range
    rk = Ranks()
    rank, world = rk.rank, rk.world
    E_total = args.egos if args.egos != 4096 else 1024
    lo, hi = shard_range(E_total, rank, world)
    E = hi - lo
    T, R = args.horizon, args.rollouts
    ctx, cfg, states, ref, _ = kmpc_setup(rk, args, E, T, R)
    rk.init()
    from f1tenth_planning_amd import _abi
    d_x0, d_ref = ctx.to_device(states), ctx.to_device(ref)
    stream = args.kmpc_stream or args.kmpc_f64
    d_ctrl = ctx.alloc(4 * E * T * 2 * R) if stream or not args.no_cpu_baseline else None
    if stream:
        ctx.kmpc_sample_controls_dev(d_ctrl, E, cfg, seed=2 + rank)
    d_steer, d_speed, d_bi, d_bc = ctx.alloc(8 * E), ctx.alloc(8 * E), ctx.alloc(4 * E), ctx.alloc(8 * E)
    ctx.kmpc_set_mode(not args.kmpc_f64)
    calls = [0]

    def step():
        if stream:
            ctx.kmpc_shoot_dev(d_x0, d_ref, d_ctrl, E, cfg, d_steer, d_speed, d_bi, d_bc if (args.kmpc_cost or args.kmpc_f64) else None)
        else:
            smp = _abi.kmpc_sampler(seed=2 + rank, call=calls[0]); calls[0] += 1
            ctx.kmpc_plan_dev(d_x0, d_ref, E, cfg, smp, d_steer, d_speed, d_bi, d_bc if args.kmpc_cost else None)
    elapsed, ms_total = timed_region(rk, ctx, step, args.warmup, args.steps)
    kernel_ms = ms_total / args.steps
    if args.dump_outputs and rank == 0:
        dumped = {"steer": d_steer.download(np.float64, (E,)), "speed": d_speed.download(np.float64, (E,)), "best_idx": d_bi.download(np.int32, (E,))}
        if args.kmpc_cost or args.kmpc_f64:                                # the step only writes best_cost when asked to
            dumped["best_cost"] = d_bc.download(np.float64, (E,))
        dump_outputs(args.dump_outputs, dumped)
    env_ok = rk.env_ok()
    if not stream and not args.no_cpu_baseline and rank == 0:      # parity leg: the last plan's controls, materialised, for the oracle
        ctx.kmpc_warm_reset()
        smp = _abi.kmpc_sampler(seed=2 + rank, call=12345, use_warm=False)
        ctx.kmpc_plan_dev(d_x0, d_ref, E, cfg, smp, d_steer, d_speed, d_bi, None)
        ctx.kmpc_gen_controls_dev(d_ctrl, E, cfg, smp)
    if rank == 0:
        abytes = (E * R * T * 8 if stream else 0) + E * (T + 1) * 32 + E * 32 + E * 28 + (0 if stream else E * T * 16)
        value = float(E_total) * R * T * args.steps / elapsed
        out = {"metric": "rollout-steps/sec (kinematic-MPC random shooting)", "value": value, "unit": "rollout-steps/s",
               "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3,
               "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f64 on f32 controls" if args.kmpc_f64 else "f32 filter + f64 refinement of the near-minimum set (decision in f64)",
               "data": "synthetic",
               "multi_process_env": {"HSA_ENABLE_IPC_MODE_LEGACY": os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY"), "zero_on_every_rank": bool(env_ok)},
               "config": {"workload": f"kmpc shooting: {E_total} egos x {R} rollouts x {T} steps over {world} GPU(s), {E} egos per GPU (BASELINE configs[4])",
                          "controls": "streamed from HBM (f32 [E][T][2][R])" if stream else "generated in the kernel (Philox4x32-10 around the device-resident warm start)"},
               "roofline": {"bound": "hbm", "achieved": abytes / (kernel_ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                            "frac": abytes / (kernel_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, "traffic": None,
                            "kernel": "k_kmpc_shoot" if args.kmpc_f64 else ("k_kmpc_shoot_mixed" if stream else "k_kmpc_plan_gen"),
                            "kernel_ms": kernel_ms, "algorithmic_bytes_per_launch": abytes,
                            "bytes_per_rollout_step": abytes / (E * R * T),
                            "note": ("below ~2048 egos per GPU the 123 KB-per-ego control buffer is Infinity-Cache resident across launches: "
                                     "the figure is then a cache-stream rate, not HBM evidence") if stream else
                                    "controls are generated in registers: no per-rollout byte ever exists in memory, the kernel is VALU-bound "
                                    "(Philox4x32-10 + the packed-f32 rollout) and the HBM fraction is reported as the tiny number it is; see valu"}}
        pmc = load_pmc({"workload": "kmpc", "egos": E, "rollouts": R, "horizon": T, "controls": "streamed" if stream else "generated"})
        if pmc and stream and pmc.get("FETCH_SIZE_KiB") is not None and pmc.get("WRITE_SIZE_KiB") is not None:
            out["roofline"]["traffic"] = int((pmc["FETCH_SIZE_KiB"] * 2 + pmc["WRITE_SIZE_KiB"]) * 1024)   # gfx950 wide-read correction x2
            out["roofline"]["traffic_source"] = pmc["source"]
        if pmc and not stream and pmc.get("SQ_INSTS_VALU"):
            tl = pmc["SQ_INSTS_VALU"] * 64.0 / (kernel_ms * 1e-3) / 1e12
            out["roofline"]["valu"] = {"kernel": pmc["kernel"], "achieved": tl, "peak": VALU_PEAK_F32_GUIDE, "unit": "T lane-instr/s",
                                       "frac": tl / VALU_PEAK_F32_GUIDE,
                                       "peak_definition": "MI355X_MICROARCH.md: one wave64 f32 VALU instruction per 2 cycles at 2.4 GHz; measured on this chip "
                                                          "(profiles/r03_valu_issue_cycles.txt): 2.5 cycles for plain VGPR-operand f32, 4.3 for packed f32 / integer multiplies / "
                                                          "conversions (most of this kernel: Philox + v_pk_fma), 8.3 for transcendentals",
                                       "frac_of_slow_class_issue_peak": tl / VALU_PEAK_SLOW_CLASS,
                                       "valu_instr_per_rollout_step": pmc["SQ_INSTS_VALU"] * 64.0 / (E * R * T),
                                       "source": pmc["source"]}
            if pmc.get("SQ_ACTIVE_INST_VALU") and pmc.get("GRBM_GUI_ACTIVE"):
                out["roofline"]["valu"]["busy_frac_profiled"] = pmc["SQ_ACTIVE_INST_VALU"] * 4.0 / (1024.0 * pmc["GRBM_GUI_ACTIVE"] / 8.0)
            if pmc.get("FETCH_SIZE_KiB") is not None and pmc.get("WRITE_SIZE_KiB") is not None:
                out["roofline"]["traffic"] = int((pmc["FETCH_SIZE_KiB"] * 2 + pmc["WRITE_SIZE_KiB"]) * 1024)
                out["roofline"]["traffic_source"] = pmc["source"]
        if not args.no_cpu_baseline:
            from oracle import oracle
            nthr = oracle.max_threads()
            n_cpu = min(E, max(nthr, 256))
            ctrl = d_ctrl.download(np.float32, (E, T, 2, R))[:n_cpu]
            t1 = time.perf_counter()
            want = oracle.kmpc_shoot_batch(states[:n_cpu], ref[:n_cpu], ctrl, cfg, nthreads=nthr)
            cpu_s = time.perf_counter() - t1
            got = d_bi.download(np.int32, (E,))[:n_cpu]
            out["cpu_baseline"] = {"value": n_cpu * R * T / cpu_s, "unit": "rollout-steps/s", "cores": nthr, "kind": "port",
                                   "sample": f"first {n_cpu} egos, oracle/f1p_oracle.c, {nthr} threads, {cpu_s:.2f} s"}
            out["parity"] = {"egos_checked": n_cpu, "best_idx_mismatches": int((want["best_idx"] != got).sum())}
        emit(out, rk=rk)
    rk.close()
    ctx.close()


if __name__ == "__main__":
    main()
