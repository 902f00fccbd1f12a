"""Device-event timing of the dynamic MPC on a track set against the raceline entry points (GPU box):
python tools/time_stmpc_tracks.py [--blocks 15] [--reps 20] [--json OUT]

Tracks: K moved and turned copies of the README raceline.  Every ego's state is a state near copy 0 moved and turned with its track, so
each ego's problem is the one the raceline side solves on copy 0: at every K the two sides do the same work.
  reference: f1p_stmpc_ref_tracks_batch against f1p_stmpc_ref_batch at T 40 (both host-pointer calls, staging copies included), and the
             _dev twin alone (kernel only);
  QP plan:   f1p_stmpc_qp_plan_tracks_batch against f1p_stmpc_qp_plan_batch at T 40 / TK 8 for 1024 egos, half of them below V_KS.
Per configuration: the median [min, max] over blocks of the per-call time of `reps` back-to-back calls between two events on the context's
stream (the QP plans with reps / 10 calls a block)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from f1tenth_planning_amd import _abi, synth  # noqa: E402
from f1tenth_planning_amd.runtime import Context  # noqa: E402


def timed(ctx, fn, blocks, reps):
    fn(); ctx.sync()
    per = []
    for _ in range(blocks):
        ctx.timer_begin()
        for _ in range(reps):
            fn()
        per.append(ctx.timer_end() / reps)
    return float(np.median(per)), float(min(per)), float(max(per))


def course_set(base, K, seed):
    """K moved and turned copies of base [N, 5] and their (rotation, offset, angle)"""
    rng = np.random.default_rng(seed)
    tracks, moves = [], []
    for k in range(K):
        ang = 2 * np.pi * k / K
        R = np.array([[np.cos(ang), np.sin(ang)], [-np.sin(ang), np.cos(ang)]])
        off = rng.normal(0, 30, 2) if k else np.zeros(2)
        t = base.copy(); t[:, :2] = base[:, :2] @ R + off; t[:, 3] += ang
        tracks.append(t); moves.append((R, off, ang))
    return tracks, moves


def moved(x, ids, moves):
    """states near copy 0 -> the same states near each ego's own copy (x, y and yaw move; the rest is frame-free)"""
    out = x.copy()
    for k, (R, off, ang) in enumerate(moves):
        m = ids == k
        out[m, :2] = x[m, :2] @ R + off
        out[m, 4 if x.shape[1] == 7 else 3] += ang
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=15)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    base = synth.make_raceline(seed=0)                                # 1692 rows, the README raceline
    rows = []
    with Context(0) as ctx, Context(0) as rctx:
        for E in (4096, 65536):
            for K in (1, 8, 256):
                tracks, moves = course_set(base, K, seed=K)
                ids = np.random.default_rng(E + K).integers(0, K, E).astype(np.int32)
                st0 = synth.make_egos(base, E, seed=7)                # (x, y, theta, v) near copy 0
                s4 = np.ascontiguousarray(st0[:, [0, 1, 3, 2]])       # (x, y, v, yaw)
                s4t = moved(s4, ids, moves)
                ctx.set_tracks([t[:, :4] for t in tracks], cols=(0, 1, 2, 3))
                rctx.set_waypoints(base[:, :4], cols=(0, 1, 2, 3))
                d_s, d_id, d_ref = ctx.to_device(s4t), ctx.to_device(ids), ctx.alloc(8 * E * 7 * 41)
                s = timed(rctx, lambda: rctx.stmpc_ref(s4, 40), a.blocks, max(2, a.reps // 4))
                t = timed(ctx, lambda: ctx.stmpc_ref_tracks(s4t, ids, 40), a.blocks, max(2, a.reps // 4))
                dv = timed(ctx, lambda: ctx.stmpc_ref_tracks_dev(d_s, d_id, E, 40, d_ref), a.blocks, a.reps)
                for b in (d_s, d_id, d_ref):
                    b.free()
                rows.append(dict(call="stmpc_ref T=40 (batch)", E=E, K=K, single_ms=s, tracks_ms=t, tracks_dev_ms=dv))
                print(f"stmpc_ref T=40   E={E:6d} K={K:3d}  single {s[0]:.4f} [{s[1]:.4f}, {s[2]:.4f}] ms   tracks {t[0]:.4f} "
                      f"[{t[1]:.4f}, {t[2]:.4f}] ms   x{t[0] / s[0]:.2f}   tracks _dev {dv[0]:.4f} [{dv[1]:.4f}, {dv[2]:.4f}] ms", flush=True)
        E = 1024
        rng = np.random.default_rng(11)
        k0 = rng.integers(0, len(base) - 1, E)
        v = np.where(np.arange(E) % 2 == 0, rng.uniform(1.0, 1.9, E), rng.uniform(2.5, 5.0, E))   # half below V_KS = 2
        x0 = np.column_stack([base[k0, 0] + rng.normal(0, 0.1, E), base[k0, 1] + rng.normal(0, 0.1, E), rng.normal(0, 0.05, E), v,
                              base[k0, 3] + rng.normal(0, 0.05, E), rng.normal(0, 0.2, E), rng.normal(0, 0.02, E)])
        dcfg, kcfg = _abi.stmpc_cfg(horizon=40), _abi.kmpc_cfg(horizon=8)
        for K in (1, 8):
            tracks, moves = course_set(base, K, seed=K)
            ids = np.random.default_rng(K).integers(0, K, E).astype(np.int32)
            x0t = moved(x0, ids, moves)
            ctx.set_tracks([t[:, :4] for t in tracks], cols=(0, 1, 2, 3))
            rctx.set_waypoints(base[:, :4], cols=(0, 1, 2, 3))
            ctx.stmpc_qp_warm_reset(); rctx.stmpc_qp_warm_reset()
            reps = max(1, a.reps // 10)
            s = timed(rctx, lambda: rctx.stmpc_qp_plan(x0, dcfg, kcfg), a.blocks, reps)
            t = timed(ctx, lambda: ctx.stmpc_qp_plan_tracks(x0t, ids, dcfg, kcfg), a.blocks, reps)
            rows.append(dict(call="stmpc_qp_plan T=40 TK=8", E=E, K=K, single_ms=s, tracks_ms=t))
            print(f"stmpc_qp_plan    E={E:6d} K={K:3d}  single {s[0]:.3f} [{s[1]:.3f}, {s[2]:.3f}] ms   tracks {t[0]:.3f} [{t[1]:.3f}, {t[2]:.3f}] ms"
                  f"   x{t[0] / s[0]:.3f}", flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
