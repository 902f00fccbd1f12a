#!/usr/bin/env python3
"""f32 position error of k_stmpc_filter_gen_col against fp64, on the GPU: the filter's ego-relative (x, y) after every step (a variant build
writes them out) against the rollout of the same applied controls in long double (tests/shoot_ref.dyn_rollout: the truth) and in the
device's fp64 (f1p_stmpc_predict_batch), for the TRUSTED rollouts -- only those can be FREE.  Prints, per case, the worst distance in
metres from either, relative to the reach and beside the derived bound of DESIGN.md 5i, which -- not this measurement -- sets the guard
and, through ob.pos_err, the discs' FREE threshold: exit status 1 when a trusted rollout lies beyond the bound.
    make -C f1tenth_planning_amd/csrc LIB=libf1p_pos.so OBJDIR=build_pos EXTRA=-DF1P_ST_DBG_POS
    F1P_LIBRARY=f1tenth_planning_amd/csrc/libf1p_pos.so python tools/stmpc_pos_error.py [--out FILE]"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import shoot_ref  # noqa: E402
import stmpc_collision_ref as S  # noqa: E402
from f1tenth_planning_amd import _abi  # noqa: E402
from f1tenth_planning_amd.runtime import Context  # noqa: E402


def bound(cfg):
    """st_pos_err_bound of csrc/k_stmpc.hip, restated"""
    u, T = 2.0 ** -24, cfg.horizon
    vmax = max(abs(cfg.max_speed), abs(cfg.min_speed)); reach = vmax * T * cfg.dt
    yr_max = vmax / cfg.wheelbase * math.tan(min(abs(cfg.max_steer), 1.4)); yaw_max = yr_max * T * cfg.dt
    dth = T * u * (yaw_max + 1.0) + 2.5e-7 * yaw_max + 80.0 * u * max(yr_max, 1.0) + 1.0e-6
    return reach * (dth + T * u + 2.0 * u + 1.0e-6 + T * u + 4.0 * u), reach


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--egos", type=int, default=64)
    ap.add_argument("--rollouts", type=int, default=256)
    ap.add_argument("--out")
    args = ap.parse_args()
    E, R = args.egos, args.rollouts
    rows = []
    with Context(0) as ctx:
        for T, sig_a in ((40, 1.5), (12, 1.5), (63, 1.5), (40, 3.0)):
            cfg = _abi.stmpc_cfg(horizon=T, n_rollouts=R)
            s = S.scene_b(E)
            img, res, ox, oy, occ = s["grid"]
            x0 = s["x0"].copy()
            rng = np.random.default_rng(T)
            x0[:, 2] = rng.normal(0, 0.05, E); x0[:, 5] = rng.normal(0, 0.2, E); x0[:, 6] = rng.normal(0, 0.02, E)
            ctx.set_waypoints(s["wp"], cols=(0, 1, 2, 3))
            ctx.set_grid(img, res, (ox, oy), occ)
            ctx.stmpc_set_collision(True, 1)
            smp = _abi.stmpc_sampler(seed=5, call=2, use_warm=True, sigma_steer_v=1.0, sigma_accel=sig_a, sigma_steer=0.15)
            warm = S.warm_start(E, T)
            d_x0, d_ref = ctx.to_device(x0), ctx.to_device(ctx.stmpc_ref(x0[:, [0, 1, 3, 4]], T))
            d = (ctx.alloc(8 * E), ctx.alloc(8 * E), ctx.alloc(4 * E))
            d_ctrl, d_pos = ctx.alloc(4 * E * T * 2 * R), ctx.alloc(4 * (1 + 2 * T) * E * R)
            d_pos.upload(np.full((1 + 2 * T) * E * R, np.nan, np.float32))
            ctx.stmpc_warm_set(warm, np.full(E, 2), T)
            ctx.stmpc_gen_controls_dev(d_ctrl, E, cfg, smp)
            ctrl = d_ctrl.download(np.float32, (E, T, 2, R))
            ctx.stmpc_set_mode(True, d_pos, None)
            ctx.stmpc_plan_dev(d_x0, d_ref, E, cfg, smp, *d)
            ctx.sync()
            ctx.stmpc_set_mode(True)
            buf = d_pos.download(np.float32, (1 + 2 * T, E, R))
            c32, pos = buf[0], buf[1:].reshape(T, 2, E, R).astype(np.float64)
            if np.isnan(pos).all():
                raise SystemExit("no positions came back: this needs the -DF1P_ST_DBG_POS build (see the docstring)")
            worst, worst_ld, dev64, n_trusted = 0.0, 0.0, 0.0, 0
            for e in range(E):
                dv, a = S.applied(ctrl[e], cfg)
                xe = np.repeat(x0[e:e + 1], R, axis=0)
                path = ctx.stmpc_predict(xe, a, dv, cfg)                                     # [R, 7, T+1] fp64
                with np.errstate(all="ignore"):
                    truth = shoot_ref.dyn_rollout(xe, a, dv, cfg)                            # the same in long double
                trusted = np.isfinite(c32[e]) & ~np.isnan(pos[:, 0, e]).any(axis=0)          # (-inf: untrusted or non-finite)
                n_trusted += int(trusted.sum())
                if not trusted.any():
                    continue
                dx = pos[:, 0, e].T - (path[:, 0, 1:] - x0[e, 0]); dy = pos[:, 1, e].T - (path[:, 1, 1:] - x0[e, 1])
                worst = max(worst, float(np.hypot(dx, dy)[trusted].max()))
                lx = (pos[:, 0, e].T - (truth[:, 0, 1:] - x0[e, 0])).astype(np.float64); ly = (pos[:, 1, e].T - (truth[:, 1, 1:] - x0[e, 1])).astype(np.float64)
                worst_ld = max(worst_ld, float(np.hypot(lx, ly)[trusted].max()))
                dev64 = max(dev64, float(np.hypot((path[:, 0] - truth[:, 0]).astype(np.float64), (path[:, 1] - truth[:, 1]).astype(np.float64))[trusted].max()))
            b, reach = bound(cfg)
            row = dict(horizon=T, sigma_accel=sig_a, egos=E, rollouts=R, trusted=n_trusted, worst_m=worst, worst_ld_m=worst_ld, fp64_vs_ld_m=dev64,
                       worst_rel_reach=worst_ld / reach, bound_m=b, guard_m=5.0 * b, cell_m=res)
            rows.append(row)
            print(json.dumps(row), flush=True)
            for buf_ in (d_x0, d_ref, d_ctrl, d_pos) + d:
                buf_.free()
        ctx.stmpc_set_collision(False)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(dict(tool="tools/stmpc_pos_error.py", rows=rows)) + "\n")
    if any(max(r["worst_m"], r["worst_ld_m"]) > r["bound_m"] for r in rows):
        raise SystemExit("a trusted rollout lies beyond st_pos_err_bound")


if __name__ == "__main__":
    main()
