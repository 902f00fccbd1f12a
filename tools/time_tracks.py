"""Device-event timing of the track-set trackers against the single-raceline entry points (GPU box):
python tools/time_tracks.py [--blocks 15] [--reps 20] [--json OUT]

Pure pursuit runs through its _dev entry points (kernels only).  Stanley, LQR and the MPC reference have single-raceline host-pointer entry
points only, so for them both sides are the *_batch calls and the figures include the staging copies.  Per configuration: the
median [min, max] over blocks of the per-call time of `reps` back-to-back calls between two events on the context's stream."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from f1tenth_planning_amd import synth  # noqa: E402
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=15)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    base = synth.make_raceline(seed=0)                                # 1692 rows, the README raceline
    rows = []
    with Context(0) as ctx:
        for E in (4096, 65536):
            for K in (1, 8, 256):
                rng = np.random.default_rng(K)
                tracks = []
                for k in range(K):                                    # K copies of the raceline, each moved and turned
                    t = base.copy(); ang = 2 * np.pi * k / max(K, 1)
                    R = np.array([[np.cos(ang), np.sin(ang)], [-np.sin(ang), np.cos(ang)]])
                    t[:, :2] = base[:, :2] @ R + rng.normal(0, 30, 2); t[:, 3] += ang
                    tracks.append(t)
                ids = rng.integers(0, K, E).astype(np.int32)
                st = np.empty((E, 4))
                for k in range(K):                                    # every ego near its own track
                    m = ids == k
                    if m.any():
                        st[m] = synth.make_egos(tracks[k], int(m.sum()), seed=100 + k)
                ctx.set_tracks(tracks)
                ctx.set_waypoints(tracks[0])
                ctx.pure_pursuit_set_form(0)
                x0 = st[:, [0, 1, 3, 2]].copy()
                d = {n: ctx.to_device(v) for n, v in dict(poses=np.ascontiguousarray(st[:, :3]), ids=ids, x0=x0).items()}
                o = {n: ctx.alloc(b) for n, b in dict(steer=8 * E, speed=8 * E, near=4 * E, la=4 * E, status=4 * E).items()}
                err = np.zeros((E, 2))
                calls = {
                    "pure_pursuit": (lambda: ctx.pure_pursuit_dev(d["poses"], E, 0.8, o["steer"], o["speed"], o["near"], o["la"], o["status"]),
                                     lambda: ctx.pure_pursuit_tracks_dev(d["poses"], d["ids"], E, 0.8, o["steer"], o["speed"], o["near"], o["la"],
                                                                         o["status"])),
                    "stanley (batch)": (lambda: ctx.stanley(st), lambda: ctx.stanley_tracks(st, ids)),
                    "lqr (batch)": (lambda: ctx.lqr(st, err), lambda: ctx.lqr_tracks(st, ids, err)),
                    "kmpc_ref T=8 (batch)": (lambda: ctx.kmpc_ref(x0, 8), lambda: ctx.kmpc_ref_tracks(x0, ids, 8)),
                }
                for name, (single, trk) in calls.items():
                    reps = a.reps if "batch" not in name else max(2, a.reps // 4)
                    s = timed(ctx, single, a.blocks, reps)
                    t = timed(ctx, trk, a.blocks, reps)
                    rows.append(dict(call=name, E=E, K=K, single_ms=s, tracks_ms=t))
                    print(f"{name:16s} E={E:6d} K={K:3d}  single {s[0]:.4f} [{s[1]:.4f}, {s[2]:.4f}] ms   tracks {t[0]:.4f} [{t[1]:.4f}, {t[2]:.4f}] ms"
                          f"   x{t[0] / s[0]:.2f}", flush=True)
                for b in list(d.values()) + list(o.values()):
                    b.free()
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
