"""Device-event timing of the lattice plan on a track set against the single-raceline plan (GPU box):
python tools/time_lattice_tracks.py [--blocks 15] [--reps 10] [--json OUT]

The bench scene (raceline, map with obstacles, 256 candidates x 50 stations); both sides through the _dev entry points (kernels only,
device buffers).  Tracks: K moved and turned copies of the bench raceline, the single-raceline side plans every ego on copy 0 -- at K = 1
the two plans do the same work.  Per configuration: the median [min, max] over blocks of the per-plan time of `reps` back-to-back plans
between two events on the context's stream."""
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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    rl = synth.make_raceline(seed=0)
    img, origin = synth.make_grid(rl[:, :2], size=(2000, 2000), resolution=0.058)
    cfg = synth.bench_lattice_cfg(n_cand=256, n_stations=50)
    rows = []
    with Context(0) as ctx:
        ctx.set_grid(img, 0.058, origin, 206)
        for E, Ks in ((4096, (1, 8, 256)), (65536, (1, 256))):
            for K in Ks:
                rng = np.random.default_rng(K)
                tracks = [rl.copy()]
                for k in range(1, K):                                 # small turns and moves: every copy stays on the map's area
                    ang = 0.02 * rng.normal(); c, s = np.cos(ang), np.sin(ang)
                    t = rl.copy(); t[:, 0] = c * rl[:, 0] - s * rl[:, 1] + rng.normal(0, 0.2); t[:, 1] = s * rl[:, 0] + c * rl[:, 1] + rng.normal(0, 0.2)
                    t[:, 3] += ang
                    tracks.append(t)
                ids = rng.integers(0, K, E).astype(np.int32)
                poses = synth.make_egos(rl, E, seed=7)
                ctx.set_tracks(tracks); ctx.set_waypoints(rl)
                d = dict(poses=ctx.to_device(np.ascontiguousarray(poses)), ids=ctx.to_device(ids))
                o = {n: ctx.alloc(b) for n, b in dict(steer=8 * E, speed=8 * E, idx=4 * E, cost=8 * E, status=4 * E, near=4 * E,
                                                     traj=32 * E * 50).items()}
                single = lambda: ctx.lattice_plan_dev(d["poses"], E, cfg, o["steer"], o["speed"], o["idx"], o["cost"], o["status"], o["near"], o["traj"])  # noqa: E731
                trk = lambda: ctx.lattice_plan_tracks_dev(d["poses"], d["ids"], E, cfg, o["steer"], o["speed"], o["idx"], o["cost"], o["status"],  # noqa: E731
                                                          o["near"], o["traj"])
                s = timed(ctx, single, a.blocks, a.reps)
                t = timed(ctx, trk, a.blocks, a.reps)
                rows.append(dict(E=E, K=K, single_ms=s, tracks_ms=t))
                print(f"lattice E={E:6d} K={K:3d}  single {s[0]:.4f} [{s[1]:.4f}, {s[2]:.4f}] ms   tracks {t[0]:.4f} [{t[1]:.4f}, {t[2]:.4f}] ms"
                      f"   x{t[0] / s[0]:.3f}", flush=True)
                for b in list(d.values()) + list(o.values()):
                    b.free()
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
