"""Seeded sessions of one long-lived Context, and the replay that checks them (tests/test_gpu_session_replay.py on the GPU,
tests/test_session_script_host.py on fakes).

A session is a list of Op records: mutators change what a context carries (scene, switches, held obstacles, groups, courses, warm
starts), queries return arrays.  Nothing in script() touches a GPU: an Op holds a kind, plain keyword arguments and the seed of its input
arrays, which Driver.inputs builds when the session is played.

replay() plays a session on one context and, before every query, builds a fresh witness context that is given only the current values
of the mutators the query reads (READS), in one canonical order (the order of MUTATORS), plus the data the long-lived context carries
for that query (warm starts, closed-loop headings) handed over explicitly.  Both must return the same arrays bit for bit, or raise the
same error.  The witness is the reference: a result that depends on what the long-lived context did before is a bug.

Where a session expects an error it must be the library's own (Driver.library_code): F1P_ESTATE for held obstacles of another batch size,
F1P_EINVAL for a bad argument; an error of the driver's Python, the same on both contexts, fails the step.

Sessions are not random mixes.  Every seed holds the patterns a-j below (the phases of _Gen), in a seeded order and with seeded shapes;
script() checks each of them on the finished list with a scan of its own (_has_a .. _has_j) before it returns:
 a  every owner of a scratch block laid out by capacity: the largest E, the smallest, a middle one, another subsystem in between
 b  the clearance bitmap: a mode-2 lattice plan, then set_grid / inflate_grid / set_footprint on / off / lattice_set_clearance, each
    followed by another one; and a plan whose clearance distance falls inside the reuse window of the map the plan before it built
    (ensure_clear_map, k_grid.hip: held >= wanted and held <= 1.3 wanted + 0.5).  inflate_grid and set_grid always mark the map stale,
    so the window is entered by a change of lattice_set_clearance on an unchanged bitmap, after a small inflation
 c  a shorter, then a longer raceline, each followed by a tracker, kmpc_ref, a lattice plan and three profile predictions of the rivals
    (a min_speed, the same again, another)
 d  another track set between two *_tracks queries of every family
 e  more than eight distinct f1p_kmpc_cfg values through kmpc_shoot / kmpc_plan / stmpc_plan's kinematic branch between two calls of the
    other family with one cfg, so that the eight-slot table wraps in between
 f  obstacles held for one E, a plan of another E (an error on both contexts), cleared, the same plan
 g  an argument error (ValueError, nothing launched) between two identical queries of each family
 h  every switch away from its default and back, a query that reads it after each flip
 i  closed-loop chains of plans and of steps, interrupted by a plan of another E and a kmpc_plan, then resumed
 j  warm-started chains of the four planners interleaved, with a change of shape and a return to the old one
"""
import dataclasses
import functools
import time

import numpy as np

from f1tenth_planning_amd import _abi, synth
from f1tenth_planning_amd import runtime as rt

SEEDS = (11, 23, 37)

E_SET = (1, 5, 33, 65, 130, 300)
E_BIG, E_SMALL = 300, 1
E_MID = (33, 65, 130)
SPACING = 0.1
RACELINES = ((101, 150), (102, 320), (103, 600))                     # (seed, n_pts): 15 m, 32 m, 60 m loops
TRACK_SETS = {1: ((111, 120),), 3: ((121, 100), (122, 180), (123, 260)),
              6: ((131, 90), (132, 140), (133, 200), (134, 110), (135, 300), (136, 160))}
# one map around each raceline: other heights, widths (150 and 168 are no multiples of 32 cells) and resolutions
MAPS = (dict(line=0, h=200, w=168, res=0.05), dict(line=1, h=170, w=150, res=0.1), dict(line=2, h=400, w=384, res=0.07))
HALF_WIDTH = 0.6
FOOTPRINT = ((0.0, 0.15, 0.3), 0.1)
LATTICE_GRIDS = {"4x7": ((0.4, 0.6, 0.8, 1.0), tuple(np.linspace(-0.4, 0.4, 7))),
                 "8x8": (tuple(np.linspace(0.5, 1.6, 8)), tuple(np.linspace(-0.45, 0.45, 8)))}
V_KS = 2.0
F1P_KMPC_CFG_SLOTS = 8                  # csrc/f1p_internal.h


@dataclasses.dataclass
class Op:
    kind: str
    kw: dict = dataclasses.field(default_factory=dict)
    seed: int = 0
    tag: str = ""          # the pattern (a-j) or "cover" the generator made it for
    expect: str = ""       # "": arrays; "error": both contexts raise; "einval": both raise ValueError
    same_as: int = -1      # index of an earlier query whose arrays this one must repeat (pattern g)


# ---- the mutators, in the witness's canonical order, with the value a fresh context holds ------------------------------------------
MUTATORS = {
    "set_waypoints": dict(line=None),
    "set_tracks": dict(K=0),
    "set_grid": dict(map=None),
    "inflate_grid": dict(radius=0.0),
    "set_footprint": dict(on=False),
    "lattice_set_clearance": dict(r=2),
    "lattice_set_mode": dict(mixed=1),
    "lattice_set_pipeline": dict(chunks=0),
    "lattice_set_split": dict(groups=0),
    "lattice_set_order": dict(heavy_first=1),
    "lattice_set_closed_loop": dict(on=False),
    "pure_pursuit_set_form": dict(egos_per_wave=0),
    "kmpc_set_mode": dict(mixed=True),
    "stmpc_set_mode": dict(mixed=True),
    "kmpc_set_groups": dict(groups=0),
    "kmpc_set_yaw_fixup": dict(on=True),
    "kmpc_qp_set_pack": dict(egos_per_wave=0),
    "kmpc_set_collision": dict(on=False, n_sub=1),
    "stmpc_set_collision": dict(on=False, n_sub=1, n_sub_k=2),
    "kmpc_qp_set_avoid": dict(on=False),
    "kmpc_qp_set_walls": dict(on=False),
    "stmpc_qp_set_avoid": dict(on=False),
    "stmpc_qp_set_walls": dict(on=False),
    "lattice_set_obstacles": dict(E=0),
    "kmpc_set_obstacles": dict(E=0),
    "stmpc_set_obstacles": dict(E=0),
    "rivals_set_groups": dict(E=0),
    "rivals_set_course": dict(E=0),
}
RESETS = ("kmpc_warm_reset", "kmpc_qp_warm_reset", "stmpc_warm_reset", "stmpc_qp_warm_reset")

_GRID = ("set_grid", "inflate_grid", "set_footprint")
_LAT = _GRID + ("lattice_set_clearance", "lattice_set_mode", "lattice_set_pipeline", "lattice_set_split", "lattice_set_order",
                "lattice_set_closed_loop", "lattice_set_obstacles")
_KSHOOT = _GRID + ("kmpc_set_mode", "kmpc_set_groups", "kmpc_set_collision", "kmpc_set_obstacles")
_SSHOOT = _GRID + ("stmpc_set_mode", "stmpc_set_collision", "stmpc_set_obstacles")
# query kind -> the mutators it reads
READS = {k: frozenset(v) for k, v in {
    "nearest_point": ("set_waypoints",), "intersect_point": ("set_waypoints",), "stanley": ("set_waypoints",), "lqr": ("set_waypoints",),
    "pure_pursuit": ("set_waypoints", "pure_pursuit_set_form"),
    "nearest_point_tracks": ("set_tracks",), "pure_pursuit_tracks": ("set_tracks",), "stanley_tracks": ("set_tracks",),
    "lqr_tracks": ("set_tracks",),
    "kmpc_ref": ("set_waypoints", "kmpc_set_yaw_fixup"), "kmpc_ref_tracks": ("set_tracks", "kmpc_set_yaw_fixup"),
    "stmpc_ref": ("set_waypoints",), "stmpc_ref_tracks": ("set_tracks",),
    "kmpc_predict": (), "stmpc_predict": (),
    "grid_occupied": _GRID, "grid_distance": ("set_grid",),
    "lattice_plan": ("set_waypoints",) + _LAT, "lattice_step": ("set_waypoints",) + _LAT, "lattice_plan_tracks": ("set_tracks",) + _LAT,
    "kmpc_shoot": _KSHOOT, "kmpc_plan": ("set_waypoints", "kmpc_set_yaw_fixup") + _KSHOOT,
    "stmpc_shoot": _SSHOOT, "stmpc_plan": ("set_waypoints", "kmpc_set_mode", "kmpc_set_groups") + _SSHOOT,
    "kmpc_qp": ("kmpc_qp_set_pack",), "kmpc_qp_avoid": ("kmpc_qp_set_pack",), "kmpc_qp_walls": ("kmpc_qp_set_pack",) + _GRID,
    "stmpc_qp": (), "stmpc_qp_avoid": (), "stmpc_qp_walls": _GRID,
    "kmpc_qp_plan": ("set_waypoints", "kmpc_set_yaw_fixup", "kmpc_qp_set_pack", "kmpc_qp_set_avoid", "kmpc_qp_set_walls",
                     "kmpc_set_obstacles") + _GRID,
    "stmpc_qp_plan": ("set_waypoints", "kmpc_qp_set_pack", "stmpc_qp_set_avoid", "stmpc_qp_set_walls", "stmpc_set_obstacles") + _GRID,
    "stmpc_qp_plan_tracks": ("set_tracks", "kmpc_qp_set_pack", "stmpc_qp_set_avoid", "stmpc_qp_set_walls", "stmpc_set_obstacles") + _GRID,
    "rivals": ("rivals_set_groups",),
    "rivals_predict": ("rivals_set_groups", "rivals_set_course", "set_waypoints", "set_tracks"),
}.items()}
QUERIES = tuple(READS)
# queries that read data the context carries from its earlier calls -> how replay() hands it to the witness (Driver.carried)
CARRIES = {"kmpc_plan": "kmpc_warm", "kmpc_qp_plan": "kmpc_qp_warm", "stmpc_plan": "stmpc_warm", "stmpc_qp_plan": "stmpc_qp_warm",
           "stmpc_qp_plan_tracks": "stmpc_qp_warm", "lattice_plan": "closed_loop", "lattice_plan_tracks": "closed_loop",
           "lattice_step": "closed_loop"}
# outputs exempt from bit-identity: (query kind, output name) -> the reason.  None was needed; the issue allows two at most.
EXEMPT = {}


class Model:
    """what a context holds now: mutator kind -> (index of the op that set it, kw, seed)"""

    def __init__(self):
        self.v = {k: (-1, dict(d), 0) for k, d in MUTATORS.items()}

    def apply(self, i, op):
        if op.kind in RESETS:
            return
        self.v[op.kind] = (i, dict(op.kw), op.seed)
        if op.kind == "set_grid":                      # f1p_set_grid drops the inflation and the footprint with the old grid
            for k in ("inflate_grid", "set_footprint"):
                self.v[k] = (-1, dict(MUTATORS[k]), 0)

    def kw(self, kind):
        return self.v[kind][1]

    def is_default(self, kind):
        return self.v[kind][1] == MUTATORS[kind]

    def setup_for(self, query):
        """the witness's set-up for `query`: the mutators it reads that are off their default, in the canonical order"""
        return [Op(k, dict(self.v[k][1]), self.v[k][2]) for k in MUTATORS if k in READS[query] and not self.is_default(k)]

    def describe(self):
        return "; ".join(f"{k}@{i}={kw}" for k, (i, kw, _) in self.v.items() if i >= 0)


# ---- scenes and inputs (host only) ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def raceline(i):
    seed, n = RACELINES[i]
    return synth.make_raceline(seed=seed, n_pts=n, spacing=SPACING)


@functools.lru_cache(maxsize=None)
def track_set(K):
    return tuple(synth.make_raceline(seed=s, n_pts=n, spacing=SPACING) for s, n in TRACK_SETS[K])


@functools.lru_cache(maxsize=None)
def grid_map(i):
    m = MAPS[i]
    img, origin = synth.make_grid(raceline(m["line"])[:, :2], size=(m["h"], m["w"]), resolution=m["res"], half_width=HALF_WIDTH, wall_px=2)
    return img, m["res"], origin


def lattice_cfg(kw):
    la, wd = LATTICE_GRIDS[kw["grid"]]
    return _abi.lattice_cfg(lookaheads=la, widths=wd, n_stations=kw["S"], weights=(0.25, 0.25, 0.25, 0.25), check_collision=True,
                            generator=kw.get("gen", "clothoid"), prune=kw.get("prune", False))


def clear_dist_cells(kw, res, clear_r, footprint):
    """the clearance distance [cells] a mixed lattice plan asks ensure_clear_map for (k_lattice_mixed.hip, the clearance mode's parameters)"""
    la, wd = LATTICE_GRIDS[kw["grid"]]
    ds = 1.2 * float(np.hypot(max(abs(v) for v in la), max(abs(v) for v in wd))) / max(kw["S"] - 1, 1)
    if kw.get("goals") == "host":
        ds = 1.2 * 4.0 / max(kw["S"] - 1, 1)
    if footprint:
        ds *= 1.0 + max(abs(o) for o in FOOTPRINT[0])
    return clear_r * ds * 1.001 / res + 1.41422 + 1.0


def _egos(line, E, seed, sigma=0.1):
    """(nearest row [E], poses [E, 4] = (x, y, theta, v)) scattered along a polyline"""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, line.shape[0] - 1, E)
    return k, np.ascontiguousarray(np.column_stack([line[k, 0] + rng.normal(0, sigma, E), line[k, 1] + rng.normal(0, sigma, E),
                                                    line[k, 3] + rng.normal(0, 0.1, E), rng.uniform(0.5, 6.0, E)]))


def _track_egos(K, E, seed):
    rng = np.random.default_rng(seed + 7)
    ids = rng.integers(0, K, E).astype(np.int32)
    k = np.empty(E, np.int64); poses = np.empty((E, 4))
    for t in range(K):
        m = np.nonzero(ids == t)[0]
        if m.size:
            k[m], poses[m] = _egos(track_set(K)[t], m.size, seed + 13 * t)
    return ids, k, poses


def _discs(poses, M, seed):
    """[E, M, 5] discs (x, y, vx, vy, r) ahead of each pose, the last slot empty"""
    rng = np.random.default_rng(seed + 3)
    E = poses.shape[0]
    ahead = rng.uniform(0.5, 1.5, (E, M)); side = rng.normal(0, 0.25, (E, M))
    c, s = np.cos(poses[:, 2])[:, None], np.sin(poses[:, 2])[:, None]
    obs = np.stack([poses[:, 0, None] + ahead * c - side * s, poses[:, 1, None] + ahead * s + side * c, rng.normal(0, 0.3, (E, M)),
                    rng.normal(0, 0.3, (E, M)), np.full((E, M), 0.15)], axis=-1)
    obs[:, -1] = (0.0, 0.0, 0.0, 0.0, -1.0)
    return np.ascontiguousarray(obs)


def _ref_rows(line, k, T, n):
    """a host-made reference [E, n, T + 1]: the rows of `line` from each ego's nearest one on, as (x, y, v, yaw) (n = 4) or in the dynamic
    model's columns (n = 7)"""
    idx = (k[:, None] + 2 * np.arange(T + 1)[None, :]) % (line.shape[0] - 1)
    ref = np.zeros((k.shape[0], n, T + 1))
    for col, src in zip((0, 1, 2, 3) if n == 4 else (0, 1, 3, 4), (0, 1, 2, 3)):
        ref[:, col] = line[idx, src]
    return ref


def _line_of(kw):
    return raceline(kw["line"]) if kw.get("line") is not None else track_set(kw["K"])[0]


def _st7(poses, seed):
    rng = np.random.default_rng(seed + 5)
    E = poses.shape[0]
    return np.ascontiguousarray(np.column_stack([poses[:, 0], poses[:, 1], rng.normal(0, 0.05, E), poses[:, 3], poses[:, 2], rng.normal(0, 0.2, E),
                                                 rng.normal(0, 0.02, E)]))


def _kcfg(kw, T=None):
    return _abi.kmpc_cfg(horizon=kw["T"] if T is None else T, n_rollouts=kw.get("R", 64), max_speed=6.0 + 0.01 * kw.get("cfg", 0))


def _dcfg(kw):
    return _abi.stmpc_cfg(horizon=kw["T"], n_rollouts=kw.get("R", 64))


class Driver:
    """how replay() talks to a context.  This one drives runtime.Context; the host tests drive fakes through a subclass."""

    def create(self):
        return rt.Context(0)

    def close(self, ctx):
        ctx.close()

    def library_code(self, exc):
        """the F1P_E* code when `exc` was raised by the runtime for a call the library rejected (runtime.core._raise), else None"""
        tb = exc.__traceback__
        while tb.tb_next is not None:
            tb = tb.tb_next
        if tb.tb_frame.f_code is not rt.core._raise.__code__:
            return None
        return _abi.F1P_EINVAL if isinstance(exc, ValueError) else exc.code

    # -- mutators ---------------------------------------------------------------------------------------------------------------------
    def mutate(self, ctx, kind, kw, seed):
        if kind in RESETS:
            return getattr(ctx, kind)()
        if kind == "set_waypoints":
            return ctx.set_waypoints(raceline(kw["line"]))
        if kind == "set_tracks":
            return ctx.set_tracks(list(track_set(kw["K"])) if kw["K"] else [])
        if kind == "set_grid":
            if kw["map"] is None:
                return ctx.set_grid(None, 0.0, (0.0, 0.0), 0)
            img, res, origin = grid_map(kw["map"])
            return ctx.set_grid(img, res, origin, 128)
        if kind == "inflate_grid":
            return ctx.inflate_grid(kw["radius"])
        if kind == "set_footprint":
            return ctx.set_footprint(FOOTPRINT[0] if kw["on"] else (), FOOTPRINT[1])
        if kind in ("lattice_set_obstacles", "kmpc_set_obstacles", "stmpc_set_obstacles"):
            obs = _discs(_egos(_line_of(kw), kw["E"], seed)[1], kw["M"], seed) if kw["E"] else None
            if kind == "lattice_set_obstacles":
                return rt.lattice_set_obstacles(ctx, obs, None if obs is None else np.full(kw["E"], 0.25))
            return getattr(rt, kind)(ctx, obs)
        if kind == "rivals_set_groups":
            return rt.rivals_set_groups(ctx, np.random.default_rng(seed).integers(-1, kw["n"], kw["E"]) if kw["E"] else None)
        if kind == "rivals_set_course":
            return rt.rivals_set_course(ctx, np.random.default_rng(seed).integers(0, kw["K"], kw["E"]) if kw["E"] else None)
        if kind in ("kmpc_qp_set_avoid", "stmpc_qp_set_avoid"):
            return getattr(rt, kind)(ctx, _abi.kmpc_qp_avoid(margin=kw["margin"]) if kw["on"] else None)
        if kind in ("kmpc_qp_set_walls", "stmpc_qp_set_walls"):
            return getattr(rt, kind)(ctx, _abi.kmpc_qp_walls(n_samples=kw["n_samples"]) if kw["on"] else None)
        if kind == "lattice_set_clearance":
            return ctx.lattice_set_clearance(kw["r"])
        return getattr(ctx, kind)(**kw)             # the switches whose kw are the method's own

    # -- the data a stateful query inherits, read from the long-lived context just before the call ----------------------------------------
    def carried(self, ctx, op):
        kw, what = op.kw, CARRIES.get(op.kind)
        try:
            if what == "kmpc_warm":
                return ctx.kmpc_warm_get(kw["E"], kw["T"])
            if what == "kmpc_qp_warm":
                return ctx.kmpc_qp_warm_get(kw["E"], kw["T"])
            if what == "stmpc_warm":
                return ctx.stmpc_warm_get(kw["E"], kw["T"], kw["TK"])
            if what == "stmpc_qp_warm":
                return ctx.stmpc_qp_warm_get(kw["E"], kw["T"])
        except rt.F1PError:                         # no warm start of this shape is held: the witness starts as the fresh context it is
            return None
        if what == "closed_loop":
            prev = ctx.lattice_closed_loop_prev()
            return prev if prev is not None and prev.shape == (kw["E"], kw["S"]) else None
        return None

    def hand_over(self, ctx, op, carried):
        kw, what = op.kw, CARRIES.get(op.kind)
        if carried is None or what == "closed_loop":
            return
        if what == "kmpc_warm":
            ctx.kmpc_warm_set(carried)
        elif what == "kmpc_qp_warm":
            ctx.kmpc_qp_warm_set(carried)
        elif what == "stmpc_warm":
            ctx.stmpc_warm_set(carried[0], carried[1], kw["T"], kw["TK"])
        elif what == "stmpc_qp_warm":
            ctx.stmpc_qp_warm_set(carried[0], carried[1])

    # -- queries ----------------------------------------------------------------------------------------------------------------------
    def inputs(self, op):
        """every array the query takes, built once and given to both contexts"""
        kw, E, seed, i = op.kw, op.kw.get("E", 0), op.seed, {}
        if op.kind == "grid_distance":
            return i
        if "K" in kw and op.kind != "rivals_predict":
            i["ids"], i["k"], i["poses"] = _track_egos(kw["K"], E, seed)
            i["line"] = track_set(kw["K"])[0]
        else:
            i["line"] = raceline(kw["line"])
            i["k"], i["poses"] = _egos(i["line"], E, seed)
        p = i["poses"]
        i["xyvyaw"] = np.ascontiguousarray(p[:, [0, 1, 3, 2]])
        if op.kind.startswith("stmpc"):
            if "vmax" in kw:
                p[:, 3] = np.random.default_rng(seed + 9).uniform(kw["vmin"], kw["vmax"], E)
                p[0, 3], p[-1, 3] = kw["vmax"], kw["vmin"]          # both branches in every batch (one ego: the kinematic one)
            i["x7"] = _st7(p, seed)
        T = kw.get("T")
        if op.kind in ("kmpc_shoot", "stmpc_shoot"):
            i["controls"] = synth.make_controls(E, T, kw["R"], seed=seed)
        if op.kind in ("kmpc_shoot", "kmpc_qp", "kmpc_qp_avoid", "kmpc_qp_walls"):
            i["ref"] = _ref_rows(i["line"], i["k"], T, 4)
        if op.kind in ("stmpc_shoot", "stmpc_qp", "stmpc_qp_avoid", "stmpc_qp_walls"):
            i["ref"] = _ref_rows(i["line"], i["k"], T, 7)
        if op.kind in ("kmpc_predict", "stmpc_predict"):
            rng = np.random.default_rng(seed + 11)
            i["oa"], i["od"] = rng.normal(0, 1.0, (E, T)), rng.normal(0, 0.1, (E, T))
        if "M" in kw and op.kind.startswith(("kmpc_qp", "stmpc_qp")):
            i["obs"] = _discs(p, kw["M"], seed)
        if op.kind in ("lattice_plan", "lattice_plan_tracks"):
            cfg = lattice_cfg(kw)
            if kw.get("goals") == "host":
                la, wd = LATTICE_GRIDS[kw["grid"]]
                if "ids" in i:
                    g = np.empty((E, cfg.n_cand, 3))
                    for t in range(kw["K"]):
                        m = np.nonzero(i["ids"] == t)[0]
                        if m.size:
                            g[m] = synth.make_goals(track_set(kw["K"])[t], p[m], la, wd)
                    i["goals"] = g
                else:
                    i["goals"] = synth.make_goals(i["line"], p, la, wd)
            if kw.get("prev"):
                i["prev"] = np.random.default_rng(seed + 17).normal(0, 0.3, (E, kw["S"])) + p[:, 2, None]
        if op.kind == "grid_occupied":               # scattered as wide as the corridor: free cells, walls and the unknown outside
            i["pts"] = p[:, :2] + np.random.default_rng(seed + 23).normal(0, HALF_WIDTH, (E, 2))
        if op.kind == "lqr" or op.kind == "lqr_tracks":
            i["err"] = np.random.default_rng(seed + 19).normal(0, 0.05, (E, 2))
        return i

    def query(self, ctx, op, i, carried):
        """run the query on `ctx`; `carried` (the witness only): the long-lived context's headings as an explicit prev_theta"""
        kind, kw, bad = op.kind, op.kw, op.kw.get("bad", False)
        E = kw.get("E", 0)
        tid = (i["ids"],) if "ids" in i else ()
        if kind in ("nearest_point", "nearest_point_tracks"):
            return getattr(ctx, kind)(i["poses"][:, :2], *tid)
        if kind == "intersect_point":
            return ctx.intersect_point(i["poses"][:, :2], kw["radius"], i["k"].astype(np.float64), wrap=kw["wrap"])
        if kind in ("pure_pursuit", "pure_pursuit_tracks"):
            return getattr(ctx, kind)(i["poses"][:, :3], *tid, kw["lookahead"])
        if kind in ("stanley", "stanley_tracks"):
            return getattr(ctx, kind)(i["xyvyaw"], *tid)
        if kind in ("lqr", "lqr_tracks"):
            return getattr(ctx, kind)(i["xyvyaw"], *tid, i["err"], timestep=0.0 if bad else 0.01)
        if kind in ("kmpc_ref", "kmpc_ref_tracks", "stmpc_ref", "stmpc_ref_tracks"):
            return getattr(ctx, kind)(i["xyvyaw"], *tid, 0 if bad else kw["T"])
        if kind == "kmpc_predict":
            return ctx.kmpc_predict(i["xyvyaw"], i["oa"], i["od"], _kcfg(kw))
        if kind == "stmpc_predict":
            return ctx.stmpc_predict(i["x7"], i["oa"], i["od"], _dcfg(kw))
        if kind == "grid_occupied":
            return ctx.grid_occupied(i["pts"])
        if kind == "grid_distance":
            return ctx.grid_distance(0 if bad else kw["cap"])
        if kind in ("lattice_plan", "lattice_plan_tracks"):
            cfg = lattice_cfg(dict(kw, S=1) if bad else kw)
            prev = i.get("prev", carried)
            out = getattr(ctx, kind)(i["poses"], *tid, cfg, goals=i.get("goals"), prev_theta=prev, reuse_outputs=kw.get("reuse", False) and prev is None,
                                     traj_dtype=np.float32 if kw.get("f32") else np.float64)
            return {k: np.array(v) for k, v in out.items()}           # (page-locked arrays the next plan overwrites)
        if kind == "lattice_step":
            cfg = lattice_cfg(kw)
            if carried is not None:                 # the witness has no chain: the same plan with the chain's headings as prev_theta
                out = ctx.lattice_plan(i["poses"], cfg, prev_theta=carried)
                return dict(steer=out["steer"], speed=out["speed"], status=out["status"], traj=out["best_traj"])
            out = {k: np.array(v) for k, v in ctx.lattice_step(i["poses"], cfg, keep_traj=True).items()}
            out["traj"] = ctx.lattice_fetch_traj(E, kw["S"])
            return out
        if kind == "kmpc_shoot":
            return ctx.kmpc_shoot(i["xyvyaw"], i["ref"], i["controls"], _kcfg(kw))
        if kind == "stmpc_shoot":
            return ctx.stmpc_shoot(i["x7"], i["ref"], i["controls"], _dcfg(kw))
        if kind == "kmpc_plan":
            smp = _abi.kmpc_sampler(seed=op.seed, call=kw.get("call", 0), use_warm=kw.get("use_warm", True), sigma_accel=-1.0 if bad else 1.5)
            return ctx.kmpc_plan(i["xyvyaw"], _kcfg(kw), smp)
        if kind == "stmpc_plan":
            smp = _abi.stmpc_sampler(seed=op.seed, call=kw.get("call", 0), use_warm=kw.get("use_warm", True))
            return ctx.stmpc_plan(i["x7"], _dcfg(kw), _kcfg(kw, kw["TK"]), smp, v_ks=V_KS)
        opts = _abi.kmpc_qp_opts(tol=-1.0) if bad else None
        if kind == "kmpc_qp":
            return ctx.kmpc_qp(i["xyvyaw"], i["ref"], _kcfg(kw), opts=opts, want_xk=True, want_duals=True)
        if kind == "stmpc_qp":
            return ctx.stmpc_qp(i["x7"], i["ref"], _dcfg(kw), opts=opts, want_x=True, want_duals=True)
        if kind == "kmpc_qp_avoid":
            return rt.kmpc_qp_avoid(ctx, i["xyvyaw"], i["ref"], i["obs"], _kcfg(kw), want_planes=True, want_avoid_duals=True)
        if kind == "kmpc_qp_walls":
            return rt.kmpc_qp_walls(ctx, i["xyvyaw"], i["ref"], i["obs"], _kcfg(kw), want_planes=True)
        if kind == "stmpc_qp_avoid":
            return rt.stmpc_qp_avoid(ctx, i["x7"], i["ref"], i["obs"], _dcfg(kw), want_planes=True, want_avoid_duals=True)
        if kind == "stmpc_qp_walls":
            return rt.stmpc_qp_walls(ctx, i["x7"], i["ref"], i["obs"], _dcfg(kw), want_planes=True)
        if kind == "kmpc_qp_plan":
            return ctx.kmpc_qp_plan(i["xyvyaw"], _kcfg(kw), opts=opts)
        if kind in ("stmpc_qp_plan", "stmpc_qp_plan_tracks"):
            return getattr(ctx, kind)(i["x7"], *tid, _dcfg(kw), _kcfg(kw, kw["TK"]), v_ks=V_KS, opts=opts)
        if kind == "rivals":
            return rt.rivals(ctx, i["poses"], "pose", 0 if bad else kw["M"], 0.25, min_speed=kw.get("min_speed", 0.5))
        if kind == "rivals_predict":
            return rt.rivals_predict(ctx, i["poses"], "pose", kw["M"], 0.25, 1.0, min_speed=kw["min_speed"], speed=kw["speed"])
        raise KeyError(kind)


# ---- the replay -------------------------------------------------------------------------------------------------------------------
def _arrays(out):
    if isinstance(out, dict):
        return {k: np.asarray(v) for k, v in out.items()}
    if isinstance(out, tuple):
        return {str(n): np.asarray(v) for n, v in enumerate(out)}
    return {"out": np.asarray(out)}


def _outcome(fn, driver):
    """("ok", arrays) or ("error", the exception's type, its message, the library's error code -- None: not the library's)"""
    try:
        return ("ok", _arrays(fn()))
    except Exception as e:  # noqa: BLE001  (the error IS the outcome: both contexts must raise the same one)
        return ("error", type(e).__name__, str(e), driver.library_code(e))


def differences(kind, got, want):
    """what differs between two outcomes of one query, as a list of lines (empty: equal bit for bit, or the same error)"""
    if got[0] != want[0]:
        say = lambda o: f"raised {o[1:]}" if o[0] == "error" else "returned arrays"      # noqa: E731
        return [f"the long-lived context {say(got)}, the witness {say(want)}"]
    if got[0] == "error":
        return [] if got == want else [f"errors differ: long-lived {got[1:]}, witness {want[1:]}"]
    a, b = got[1], want[1]
    if set(a) != set(b):
        return [f"outputs differ: {sorted(a)} against {sorted(b)}"]
    lines = []
    for k in sorted(a):
        if (kind, k) in EXEMPT:
            continue
        if a[k].dtype != b[k].dtype or a[k].shape != b[k].shape:
            lines.append(f"{k}: {a[k].dtype}{a[k].shape} against {b[k].dtype}{b[k].shape}")
        elif not np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"):
            ne = ~((a[k] == b[k]) | ((a[k] != a[k]) & (b[k] != b[k]))) if a[k].dtype.kind == "f" else a[k] != b[k]
            first = tuple(int(v) for v in np.argwhere(ne)[0]) if ne.ndim else ()
            lines.append(f"{k}: {int(ne.sum())} of {ne.size} entries differ, first at {first}: {a[k][first]!r} against the witness's {b[k][first]!r}")
    return lines


def replay(ops, driver, seed=None, check=True, stats=None):
    """play `ops` on one long-lived context of `driver`, every query against a fresh witness; AssertionError at the first difference.
    check=False only plays (a dry run of the calls).  stats: a dict that receives the number of queries and the witnesses' seconds."""
    model, kept = Model(), {}
    wanted = {op.same_as for op in ops if op.same_as >= 0}
    long = driver.create()
    n_q, t_wit = 0, 0.0
    try:
        for n, op in enumerate(ops):
            def fail(lines):
                raise AssertionError(f"seed {seed}, op {n} {op.kind} {op.kw} (input seed {op.seed}, pattern {op.tag!r}):\n  " + "\n  ".join(lines) +
                                     f"\n  last mutators: {model.describe()}")
            if op.kind in MUTATORS or op.kind in RESETS:
                driver.mutate(long, op.kind, op.kw, op.seed)
                model.apply(n, op)
                continue
            inputs = driver.inputs(op)
            carried = driver.carried(long, op)
            if op.kind in ("lattice_plan", "lattice_plan_tracks") and not model.kw("lattice_set_closed_loop")["on"]:
                carried = None                      # (headings a chain of steps left behind: a plan outside closed-loop mode does not read them)
            got = _outcome(lambda: driver.query(long, op, inputs, None), driver)
            t0 = time.perf_counter()
            wit = driver.create()
            try:
                for m in model.setup_for(op.kind):
                    driver.mutate(wit, m.kind, m.kw, m.seed)
                t_wit += time.perf_counter() - t0
                driver.hand_over(wit, op, carried)
                want = _outcome(lambda: driver.query(wit, op, inputs, carried), driver)
            finally:
                t0 = time.perf_counter()
                driver.close(wit)
                t_wit += time.perf_counter() - t0
            n_q += 1
            if n in wanted:
                kept[n] = got
            if not check:
                continue
            lines = differences(op.kind, got, want)
            if not lines and op.expect and got[0] != "error":
                lines = [f"expected an error ({op.expect}), both contexts returned arrays"]
            code = {"error": _abi.F1P_ESTATE, "einval": _abi.F1P_EINVAL}.get(op.expect)
            if not lines and op.expect and got[3] != code:             # (an error of the driver's own Python proves nothing about the library)
                lines = [f"expected the library's error {code} ({op.expect}), got {got[1:]}"]
            if not lines and not op.expect and got[0] == "error":
                lines = [f"both contexts raised {got[1:]}: the session asks for something the library rejects"]
            if not lines and op.same_as >= 0:
                lines = [f"differs from the identical query at op {op.same_as}: " + s for s in differences(op.kind, got, kept[op.same_as])]
            if lines:
                fail(lines)
    finally:
        driver.close(long)
        if stats is not None:
            stats.update(queries=n_q, witness_seconds=t_wit)


# ---- the generator ----------------------------------------------------------------------------------------------------------------
class _Gen:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.ops, self.model, self.tag = [], Model(), ""

    def pick(self, seq):
        return seq[int(self.rng.integers(0, len(seq)))]

    def m(self, kind, **kw):
        """a mutator -- skipped when the model already holds that value, unless it carries an array"""
        if kind in MUTATORS and self.model.kw(kind) == kw and "E" not in kw:
            return
        op = Op(kind, kw, int(self.rng.integers(1, 2 ** 31)), self.tag)
        self.model.apply(len(self.ops), op)
        self.ops.append(op)
        return op

    def q(self, kind, expect="", same_as=-1, seed=None, **kw):
        if "line" in kw and kw["line"] is None:
            kw["line"] = self.model.kw("set_waypoints")["line"]
        op = Op(kind, kw, int(self.rng.integers(1, 2 ** 31)) if seed is None else seed, self.tag, expect, same_as)
        self.ops.append(op)
        return len(self.ops) - 1

    @property
    def line(self):
        return self.model.kw("set_waypoints")["line"]

    @property
    def K(self):
        return self.model.kw("set_tracks")["K"]

    def scene(self, line=0, K=3, grid=True):
        self.m("set_waypoints", line=line)
        self.m("set_tracks", K=K)
        self.m("set_grid", map=line if grid else None)

    def plan(self, E, **kw):
        kw.setdefault("grid", "4x7"); kw.setdefault("S", 20)
        return self.q("lattice_plan", E=E, line=self.line, **kw)

    def other(self, family):
        """a query of another subsystem than `family`"""
        if family == "lattice":
            return self.q("kmpc_ref", E=5, T=8, line=self.line)
        return self.q("nearest_point", E=5, line=self.line)

    def obstacles(self, kind, E, M=3):
        if E:
            op = self.m(kind, E=E, M=M, line=self.line)
        else:
            op = self.m(kind, E=0)
        return op

    # a: capacity-laid-out scratch -- the largest E, the smallest, a middle one, another subsystem's query in between
    def phase_a(self):
        self.scene(self.pick((0, 1)))
        mid, S = self.pick(E_MID), self.pick((20, 37))
        ln = self.line

        def triple(family, fn, before=None):
            for n, E in enumerate((E_BIG, E_SMALL, mid)):
                if before:
                    before(E)
                fn(E)
                if n < 2:
                    self.other(family)

        self.m("lattice_set_mode", mixed=2)
        triple("lattice", lambda E: self.plan(E, S=S))                                          # d_mix_scratch, d_rec_scratch, d_order
        triple("lattice", lambda E: self.plan(E, S=S), lambda E: self.obstacles("lattice_set_obstacles", E))   # d_lat_obs_xf
        self.obstacles("lattice_set_obstacles", 0)
        self.m("lattice_set_mode", mixed=0)
        triple("lattice", lambda E: self.plan(E, S=S, prune=True, grid="8x8"))                 # d_bb_scratch
        self.m("lattice_set_split", groups=2)
        triple("lattice", lambda E: self.plan(E, S=S, grid="8x8"))                             # d_split_scratch
        self.m("lattice_set_split", groups=0)
        self.m("lattice_set_mode", mixed=1)
        self.m("lattice_set_closed_loop", on=True)
        triple("lattice", lambda E: (self.plan(E, S=S), self.plan(E, S=S)))                    # d_cl_theta[2]
        self.m("lattice_set_closed_loop", on=False)
        triple("lattice", lambda E: self.q("lattice_step", E=E, grid="4x7", S=S, line=ln))     # the step blocks
        triple("lattice", lambda E: self.q("lattice_plan_tracks", E=E, K=self.K, grid="4x7", S=S))
        self.m("kmpc_set_groups", groups=2)
        triple("mpc", lambda E: self.q("kmpc_plan", E=E, T=8, R=256, line=ln))                  # d_kmpc_scratch (kmpc_cap_E / R)
        self.m("kmpc_set_groups", groups=0)
        triple("mpc", lambda E: self.q("stmpc_shoot", E=E, T=20, R=64, line=ln))               # d_st_scratch
        triple("mpc", lambda E: self.q("stmpc_plan", E=E, T=20, TK=8, R=64, vmin=0.5, vmax=4.0, line=ln))
        triple("mpc", lambda E: self.q("kmpc_qp_plan", E=E, T=8, line=ln))                      # the arena, the warm buffers
        triple("mpc", lambda E: self.q("stmpc_qp_plan", E=E, T=10, TK=8, vmin=0.5, vmax=4.0, line=ln))
        triple("rivals", lambda E: self.q("rivals_predict", E=E, M=4, speed="profile", min_speed=0.5, line=ln))   # d_riv_rec / idx
        triple("rivals", lambda E: self.q("rivals", E=E, M=4, line=ln),
               lambda E: self.m("rivals_set_groups", E=E, n=3))                                # d_riv_mem / rng (riv_cap)
        self.m("rivals_set_groups", E=0)

    # b: the clearance bitmap
    def phase_b(self):
        self.scene(0)
        E = self.pick(E_MID)
        self.m("lattice_set_mode", mixed=2)
        self.plan(E)
        self.m("set_grid", map=1); self.m("set_waypoints", line=1)
        self.plan(E)
        self.m("inflate_grid", radius=0.3)
        self.plan(E)
        self.m("set_footprint", on=True)
        self.plan(E)
        self.m("set_footprint", on=False)
        self.plan(E)
        self.m("lattice_set_clearance", r=0)
        self.plan(E)
        self.m("lattice_set_clearance", r=2)
        self.m("inflate_grid", radius=0.1)           # a small step: the map is stale all the same, the plan rebuilds it for r = 2 ...
        self.plan(E)
        self.m("lattice_set_clearance", r=1)         # ... and this plan's smaller distance falls inside that map's reuse window
        self.plan(E)
        self.m("kmpc_set_collision", on=True, n_sub=2)   # the shooting filter asks the same bitmap for its own distance
        self.q("kmpc_plan", E=E, T=8, R=64, line=self.line)
        self.plan(E)
        self.m("kmpc_set_collision", on=False, n_sub=1)
        self.m("lattice_set_clearance", r=2)
        self.m("inflate_grid", radius=0.0)
        self.plan(E)
        self.m("lattice_set_mode", mixed=1)

    # c: a shorter, then a longer raceline
    def phase_c(self):
        self.scene(1)
        self.q("rivals_predict", E=33, M=4, speed="profile", min_speed=0.5, line=1)
        for line in (0, 2):
            self.m("set_waypoints", line=line); self.m("set_grid", map=line)
            E = self.pick(E_MID)
            self.q(self.pick(("pure_pursuit", "stanley", "nearest_point")), E=E, lookahead=0.8, line=line)
            self.q("kmpc_ref", E=E, T=8, line=line)
            self.plan(E)
            for ms in (0.5, 0.5, 1.0):
                self.q("rivals_predict", E=E, M=4, speed="profile", min_speed=ms, line=line)
            self.q("rivals_predict", E=E, M=4, speed="constant", min_speed=0.5, line=line)

    # d: another track set between two *_tracks queries of every family
    def phase_d(self):
        self.scene(self.line if self.line is not None else 0, K=3)
        for K in (3,) + self.pick(((6, 1), (1, 6))):
            self.m("set_tracks", K=K)
            E = self.pick((5, 33))
            for kind in ("nearest_point_tracks", "pure_pursuit_tracks", "stanley_tracks", "lqr_tracks", "kmpc_ref_tracks", "stmpc_ref_tracks"):
                self.q(kind, E=E, K=K, T=8, lookahead=0.8)
            self.q("lattice_plan_tracks", E=E, K=K, grid="4x7", S=20)
            self.q("stmpc_qp_plan_tracks", E=E, K=K, T=10, TK=8, vmin=0.5, vmax=4.0)
            self.m("rivals_set_course", E=E, K=K)
            self.q("rivals_predict", E=E, M=4, speed="profile", min_speed=0.5, line=self.line)
            self.m("rivals_set_course", E=0)

    # e: the eight-slot table of shooting configurations wraps while the other family is between two of its own calls
    def phase_e(self):
        self.scene(0)
        ln = self.line
        self.q("kmpc_plan", E=5, T=8, R=64, cfg=0, line=ln)
        for c in range(1, 10):
            self.q("stmpc_plan", E=5, T=self.pick((20, 21)), TK=8, R=64, cfg=c, vmin=0.5, vmax=3.5, line=ln)
        self.q("kmpc_plan", E=5, T=8, R=64, cfg=0, line=ln)
        self.q("kmpc_shoot", E=5, T=8, R=64, cfg=0, line=ln)
        self.q("stmpc_plan", E=5, T=20, TK=8, R=64, cfg=1, vmin=0.5, vmax=3.5, line=ln)
        for c in range(10, 19):
            self.q(self.pick(("kmpc_shoot", "kmpc_plan")), E=5, T=self.pick((8, 20)), R=64, cfg=c, line=ln)
        self.q("stmpc_plan", E=5, T=20, TK=8, R=64, cfg=1, vmin=0.5, vmax=3.5, line=ln)

    # f: obstacles held for one E, a plan of another E, cleared, the same plan
    def phase_f(self):
        self.scene(0)
        ln = self.line
        plans = {"lattice_set_obstacles": lambda E, **k: self.plan(E, **k),
                 "kmpc_set_obstacles": lambda E, **k: self.q("kmpc_plan", E=E, T=8, R=64, line=ln, **k),
                 "stmpc_set_obstacles": lambda E, **k: self.q("stmpc_plan", E=E, T=20, TK=8, R=64, vmin=0.5, vmax=4.0, line=ln, **k)}
        for kind, plan in plans.items():
            self.obstacles(kind, 33)
            plan(33)
            plan(5, expect="error")
            self.obstacles(kind, 0)
            plan(5)

    # g: an argument error between two identical queries of each family
    def phase_g(self):
        self.scene(0)
        ln = self.line
        for first, bad in ((dict(kind="stanley", E=5), dict(kind="lqr", E=5)),
                           (dict(kind="kmpc_ref", E=5, T=8), dict(kind="stmpc_ref", E=5, T=8)),
                           (dict(kind="grid_occupied", E=5), dict(kind="grid_distance", cap=8)),
                           (dict(kind="lattice_plan", E=5, grid="4x7", S=20), dict(kind="lattice_plan", E=5, grid="4x7", S=20)),
                           (dict(kind="kmpc_shoot", E=5, T=8, R=64), dict(kind="kmpc_plan", E=5, T=8, R=64)),
                           (dict(kind="kmpc_qp", E=5, T=8), dict(kind="kmpc_qp_plan", E=5, T=8)),
                           (dict(kind="rivals", E=5, M=4), dict(kind="rivals", E=5, M=4))):
            a = self.q(line=ln, **first)
            self.q(line=ln, bad=True, expect="einval", **bad)
            self.q(line=ln, same_as=a, seed=self.ops[a].seed, **first)

    # h: every switch away from its default and back, a reader after each flip
    def phase_h(self):
        self.scene(0)
        ln = self.line
        E = self.pick((5, 33))
        plan = lambda: self.plan(E)                                                            # noqa: E731
        kplan = lambda: self.q("kmpc_plan", E=E, T=8, R=256, line=ln)                          # noqa: E731
        splan = lambda: self.q("stmpc_plan", E=E, T=20, TK=8, R=64, vmin=0.5, vmax=4.0, line=ln)   # noqa: E731
        kqp = lambda: self.q("kmpc_qp_plan", E=E, T=8, line=ln)                                # noqa: E731
        sqp = lambda: self.q("stmpc_qp_plan", E=E, T=10, TK=8, vmin=0.5, vmax=4.0, line=ln)    # noqa: E731
        flips = [("inflate_grid", dict(radius=0.3), plan), ("set_footprint", dict(on=True), plan),
                 ("lattice_set_clearance", dict(r=1), plan), ("lattice_set_mode", dict(mixed=0), plan), ("lattice_set_mode", dict(mixed=2), plan),
                 ("lattice_set_pipeline", dict(chunks=2), lambda: self.plan(E_BIG)), ("lattice_set_split", dict(groups=2), plan),
                 ("lattice_set_order", dict(heavy_first=0), plan), ("lattice_set_closed_loop", dict(on=True), plan),
                 ("pure_pursuit_set_form", dict(egos_per_wave=4), lambda: self.q("pure_pursuit", E=E, lookahead=0.8, line=ln)),
                 ("kmpc_set_mode", dict(mixed=False), kplan), ("stmpc_set_mode", dict(mixed=False), splan),
                 ("kmpc_set_groups", dict(groups=2), kplan), ("kmpc_set_yaw_fixup", dict(on=False), lambda: self.q("kmpc_ref", E=E, T=8, line=ln)),
                 ("kmpc_qp_set_pack", dict(egos_per_wave=1), lambda: self.q("kmpc_qp", E=E, T=8, line=ln)),
                 ("kmpc_set_collision", dict(on=True, n_sub=2), kplan), ("stmpc_set_collision", dict(on=True, n_sub=2, n_sub_k=2), splan),
                 ("kmpc_qp_set_walls", dict(on=True, n_samples=24), kqp), ("stmpc_qp_set_walls", dict(on=True, n_samples=24), sqp),
                 ("rivals_set_groups", dict(E=E, n=3), lambda: self.q("rivals", E=E, M=4, line=ln)),
                 ("rivals_set_course", dict(E=E, K=self.K), lambda: self.q("rivals_predict", E=E, M=4, speed="constant", min_speed=0.5, line=ln)),
                 ("set_grid", dict(map=None), plan), ("set_tracks", dict(K=1), lambda: self.q("nearest_point_tracks", E=E, K=self.K))]
        order = self.rng.permutation(len(flips))
        for j in order:
            kind, away, reader = flips[int(j)]
            back = dict(self.model.kw(kind))
            self.m(kind, **away)
            reader()
            self.m(kind, **back)
            reader()
        for kind, reader in (("lattice_set_obstacles", plan), ("kmpc_set_obstacles", kplan), ("stmpc_set_obstacles", splan)):
            self.obstacles(kind, E)
            reader()
            self.obstacles(kind, 0)
            reader()
        for sw, obs, reader in (("kmpc_qp_set_avoid", "kmpc_set_obstacles", kqp), ("stmpc_qp_set_avoid", "stmpc_set_obstacles", sqp)):
            self.obstacles(obs, E)
            self.m(sw, on=True, margin=0.05)
            reader()
            self.m(sw, on=False)
            reader()
            self.obstacles(obs, 0)
        for kind in RESETS:                                  # the four warm resets, each read by its planner
            reader = dict(kmpc_warm_reset=kplan, kmpc_qp_warm_reset=kqp, stmpc_warm_reset=splan, stmpc_qp_warm_reset=sqp)[kind]
            reader()
            self.m(kind)
            reader()

    # i: closed-loop chains, interrupted and resumed
    def phase_i(self):
        self.scene(0)
        ln = self.line
        E, S = self.pick(E_MID), self.pick((20, 37))
        self.m("lattice_set_closed_loop", on=True)
        for _ in range(3):
            self.plan(E, S=S, reuse=True)
        self.plan(5, S=S)
        self.q("kmpc_plan", E=E, T=8, R=64, line=ln)
        for _ in range(2):
            self.plan(E, S=S)
        self.plan(E, S=S, prev=True)
        self.plan(E, S=S)
        self.m("lattice_set_closed_loop", on=False)
        for _ in range(2):
            self.q("lattice_step", E=E, grid="4x7", S=S, line=ln)
        self.plan(5, S=S)
        self.q("kmpc_plan", E=E, T=8, R=64, line=ln)
        self.q("lattice_step", E=E, grid="4x7", S=S, line=ln)

    # j: warm-started chains of the four planners, interleaved; another shape, and back
    def phase_j(self):
        self.scene(0)
        ln = self.line
        E = self.pick((33, 65))

        def round_(E, T, Td, call):
            self.q("kmpc_plan", E=E, T=T, R=64, call=call, line=ln)
            self.q("kmpc_qp_plan", E=E, T=T if T <= 16 else 16, line=ln)
            self.q("stmpc_plan", E=E, T=Td, TK=8, R=64, call=call, vmin=0.5, vmax=4.0, line=ln)
            self.q("stmpc_qp_plan", E=E, T=10 if Td == 20 else 20, TK=8, vmin=0.5, vmax=4.0, line=ln)

        round_(E, 8, 20, 0)
        round_(E, 8, 20, 1)
        round_(5, 8, 20, 2)          # another batch size
        round_(E, 8, 20, 3)          # ... and back
        round_(E, 20, 21, 4)         # another horizon
        round_(E, 8, 20, 5)          # ... and back
        round_(E, 8, 20, 6)

    # every query kind and variant once more, with seeded shapes
    def phase_cover(self):
        self.scene(self.pick((0, 1, 2)))
        ln, K = self.line, self.K
        E = lambda: self.pick(E_SET[:5])                                                       # noqa: E731
        for kind in ("nearest_point", "stanley", "lqr"):
            self.q(kind, E=E(), line=ln)
        self.q("intersect_point", E=E(), radius=0.8, wrap=True, line=ln)
        self.q("pure_pursuit", E=E(), lookahead=0.8, line=ln)
        self.q("stmpc_ref", E=E(), T=20, line=ln)
        self.q("kmpc_predict", E=E(), T=self.pick((8, 20)), line=ln)
        self.q("stmpc_predict", E=E(), T=self.pick((20, 21)), line=ln)
        self.q("grid_occupied", E=E(), line=ln)
        self.q("grid_distance", cap=8)
        for kw in (dict(goals="host"), dict(prev=True), dict(f32=True), dict(prune=True), dict(gen="cubic"), dict(grid="8x8", S=37),
                   dict(goals="host", prev=True, f32=True, reuse=True)):
            self.plan(E(), **kw)
        self.q("lattice_plan_tracks", E=E(), K=K, grid="8x8", S=37, goals="host")
        self.q("kmpc_shoot", E=E(), T=20, R=256, line=ln)
        self.q("stmpc_shoot", E=E(), T=21, R=256, line=ln)
        for T in (8, 16):
            self.q("kmpc_qp", E=E(), T=T, line=ln)
            self.q("kmpc_qp_avoid", E=E(), T=T, M=3, line=ln)
            self.q("kmpc_qp_walls", E=E(), T=T, M=3, line=ln)
        for T in (10, 20):
            self.q("stmpc_qp", E=E(), T=T, line=ln)
            self.q("stmpc_qp_avoid", E=E(), T=T, M=3, line=ln)
            self.q("stmpc_qp_walls", E=E(), T=T, M=3, line=ln)
        self.q("kmpc_qp_plan", E=E(), T=16, line=ln)
        self.q("stmpc_qp_plan", E=E(), T=20, TK=8, vmin=0.5, vmax=4.0, line=ln)


PHASES = "abcdefghij"


def script(seed):
    """the session of `seed`: a list of Op; deterministic; holds every pattern a-j (each asserted here by its own scan, _has_a .. _has_j) and every
    mutator and query kind"""
    g = _Gen(seed)
    order = [PHASES[int(j)] for j in g.rng.permutation(len(PHASES))] + ["cover"]
    for name in order:
        g.tag = name
        getattr(g, "phase_" + name)()
    ops = g.ops
    for check in (_has_a, _has_b, _has_c, _has_d, _has_e, _has_f, _has_g, _has_h, _has_i, _has_j):
        check(ops)
    missing = (set(MUTATORS) | set(RESETS) | set(QUERIES)) - {op.kind for op in ops}
    assert not missing, missing
    assert all(op.kw.get("E", 1) in E_SET or op.kw.get("E") == 0 for op in ops)
    return ops


# ---- script()'s own check of the patterns: one small scan each, over kinds and arguments only (the tags play no part) ----------------
def _states(ops):
    """(index, op, the Model before it) -- one Model, updated as the walk goes on"""
    model = Model()
    for n, op in enumerate(ops):
        yield n, op, model
        if op.kind in MUTATORS:
            model.apply(n, op)


def _is_query(op):
    return op.kind in READS


def _subsystem(kind):
    return "lattice" if kind.startswith(("lattice", "grid")) else "rivals" if kind.startswith("rivals") else \
        "mpc" if kind.startswith(("kmpc", "stmpc")) else "trackers"


def _has_a(ops):
    on = lambda m, k: m.kw(k)                                                                  # noqa: E731
    owners = {"mix": ("lattice_plan", lambda op, m: on(m, "lattice_set_mode")["mixed"] == 2 and not on(m, "lattice_set_obstacles")["E"]),
              "obs_xf": ("lattice_plan", lambda op, m: on(m, "lattice_set_mode")["mixed"] == 2 and on(m, "lattice_set_obstacles")["E"] == op.kw["E"]),
              "bb": ("lattice_plan", lambda op, m: on(m, "lattice_set_mode")["mixed"] == 0 and op.kw.get("prune")),
              "split": ("lattice_plan", lambda op, m: on(m, "lattice_set_split")["groups"] > 0),
              "cl_theta": ("lattice_plan", lambda op, m: on(m, "lattice_set_closed_loop")["on"]),
              "step": ("lattice_step", lambda op, m: True), "tracks": ("lattice_plan_tracks", lambda op, m: True),
              "kmpc_scratch": ("kmpc_plan", lambda op, m: on(m, "kmpc_set_groups")["groups"] > 1 and op.kw["R"] > 128),
              "st_scratch": ("stmpc_shoot", lambda op, m: on(m, "stmpc_set_mode")["mixed"]), "st_plan": ("stmpc_plan", lambda op, m: True),
              "qp_warm": ("kmpc_qp_plan", lambda op, m: True), "stqp_warm": ("stmpc_qp_plan", lambda op, m: True),
              "riv_rec": ("rivals_predict", lambda op, m: True), "riv_mem": ("rivals", lambda op, m: on(m, "rivals_set_groups")["E"] == op.kw["E"])}
    for name, (kind, cond) in owners.items():
        stage, between = 0, True
        for n, op, m in _states(ops):
            if not _is_query(op) or stage == 3:
                continue
            if op.kind == kind and between and cond(op, m) and (op.kw["E"] == (E_BIG, E_SMALL)[stage] if stage < 2 else op.kw["E"] in E_MID):
                stage, between = stage + 1, False
            elif stage and _subsystem(op.kind) != _subsystem(kind):
                between = True
        assert stage == 3, f"pattern a: {name} ({kind}) lacks the largest / smallest / middle batch with another subsystem in between"


def _has_b(ops):
    seen, pending, started = set(), None, False
    for n, op, m in _states(ops):
        mode2 = op.kind == "lattice_plan" and m.kw("lattice_set_mode")["mixed"] == 2 and m.kw("set_grid")["map"] is not None
        if started and op.kind in _GRID + ("lattice_set_clearance",):
            old = m.kw("set_grid")["map"]
            if op.kind == "set_grid":
                other = None not in (old, op.kw["map"]) and all(MAPS[old][k] != MAPS[op.kw["map"]][k] for k in ("h", "w", "res"))
                pending = "set_grid" if other else None
            else:
                pending = op.kind + (" on" if op.kw.get("on") else "")
        elif _is_query(op):
            if mode2 and pending:
                seen.add(pending)
            started, pending = started or (mode2 and m.kw("lattice_set_clearance")["r"] > 0), None
    want = {"set_grid", "inflate_grid", "set_footprint on", "set_footprint", "lattice_set_clearance"}
    assert seen == want, f"pattern b: no mode-2 plan right after {want - seen}"
    assert any(op.kind == "inflate_grid" and 0.0 < op.kw["radius"] <= 0.1 for op in ops), "pattern b: no small inflation step"
    _assert_window(ops)


def _has_c(ops):
    found, prev, span = set(), None, None
    for op in list(ops) + [Op("set_waypoints", dict(line=None))]:
        if op.kind == "set_waypoints":
            if span is not None:
                kinds, ms = {o.kind for o in span[1]}, [o.kw["min_speed"] for o in span[1] if o.kind == "rivals_predict" and o.kw["speed"] == "profile"]
                if kinds & {"pure_pursuit", "stanley", "nearest_point"} and {"kmpc_ref", "lattice_plan"} <= kinds and \
                        any(x == y != z for x, y, z in zip(ms, ms[1:], ms[2:])):
                    found.add(span[0])
            line = op.kw["line"]
            span = None if prev is None or line is None else ("shorter" if RACELINES[line][1] < RACELINES[prev][1] else "longer", [])
            prev = line
        elif span is not None and _is_query(op):
            span[1].append(op)
    assert found == {"shorter", "longer"}, f"pattern c: only {found}"


def _has_d(ops):
    for kind in [k for k in QUERIES if k.endswith("_tracks")] + ["rivals_predict"]:
        Ks = [m.kw("set_tracks")["K"] for n, op, m in _states(ops) if op.kind == kind and (kind != "rivals_predict" or m.kw("rivals_set_course")["E"])]
        assert len(set(Ks)) >= 2, f"pattern d: {kind} sees one track set only"


def _has_e(ops):
    calls = [("k" if op.kind != "stmpc_plan" else "s", (op.kw["TK" if op.kind == "stmpc_plan" else "T"], op.kw["R"], op.kw.get("cfg", 0)))
             for op in ops if op.kind in ("kmpc_shoot", "kmpc_plan", "stmpc_plan")]
    assert len({c for _, c in calls}) >= 10, "pattern e: fewer than ten shooting configurations"
    for fam in "ks":
        last, ok = {}, False
        for n, (f, c) in enumerate(calls):
            if f == fam:
                if c in last and len({c2 for f2, c2 in calls[last[c] + 1:n] if f2 != fam and c2 != c}) >= F1P_KMPC_CFG_SLOTS:
                    ok = True
                last[c] = n
        assert ok, f"pattern e: the table does not wrap between two calls of family {fam}"
    # the kinematic branch reaches the table only with an ego at or below V_KS (Driver.inputs pins one at vmin and one at vmax)
    assert all(op.kw["vmin"] <= V_KS < op.kw["vmax"] for op in ops if op.kind in ("stmpc_plan", "stmpc_qp_plan", "stmpc_qp_plan_tracks"))


def _has_f(ops):
    for kind, plan in (("lattice_set_obstacles", "lattice_plan"), ("kmpc_set_obstacles", "kmpc_plan"), ("stmpc_set_obstacles", "stmpc_plan")):
        stage, E = 0, None
        for n, op, m in _states(ops):
            held = m.kw(kind)["E"]
            if stage == 0 and op.kind == plan and held and op.kw["E"] != held and op.expect == "error":
                stage, E = 1, op.kw["E"]
            elif stage == 1 and (op.kind == kind or _is_query(op)):
                stage = 2 if op.kind == kind and op.kw["E"] == 0 else 0
            elif stage == 2 and (_is_query(op) or op.kind == kind):
                stage = 3 if op.kind == plan and op.kw["E"] == E and not op.expect else 0
        assert stage == 3, f"pattern f: {kind}"
    for n, op, m in _states(ops):                                     # ... and an error is expected nowhere else
        if op.expect == "error":
            assert any(m.kw(k)["E"] not in (0, op.kw["E"]) for k in ("lattice_set_obstacles", "kmpc_set_obstacles", "stmpc_set_obstacles")), n


def _has_g(ops):
    q = [(n, op) for n, op in enumerate(ops) if _is_query(op)]
    firsts = {a.kind for (na, a), (_, bad), (_, c) in zip(q, q[1:], q[2:])
              if bad.expect == "einval" and bad.kw.get("bad") and not a.expect and (a.kind, a.kw, a.seed) == (c.kind, c.kw, c.seed) and c.same_as == na}
    want = {"stanley", "kmpc_ref", "grid_occupied", "lattice_plan", "kmpc_shoot", "kmpc_qp", "rivals"}      # one per family, none of them stateful
    assert firsts >= want, f"pattern g: {want - firsts}"
    assert all(bool(op.kw.get("bad")) == (op.expect == "einval") for _, op in q)


def _has_h(ops):
    flips = {}
    for a, b in zip(ops, ops[1:]):
        if a.kind in MUTATORS and _is_query(b) and a.kind in READS[b.kind]:
            flips.setdefault(a.kind, set()).add(a.kw == MUTATORS[a.kind])
    missing = [k for k in MUTATORS if k not in ("set_waypoints", "set_tracks") and flips.get(k) != {True, False}]
    assert not missing, f"pattern h: no reader after a flip away and one back of {missing}"
    for reset in RESETS:
        plan = {"kmpc_warm_reset": "kmpc_plan", "kmpc_qp_warm_reset": "kmpc_qp_plan", "stmpc_warm_reset": "stmpc_plan", "stmpc_qp_warm_reset": "stmpc_qp_plan"}[reset]
        assert any(a.kind == c.kind == plan and a.kw == c.kw and b.kind == reset for a, b, c in zip(ops, ops[1:], ops[2:])), f"pattern h: {reset}"


def _has_i(ops):
    for kind, armed, need in (("lattice_plan", True, 3), ("lattice_step", False, 2)):
        run, shape, stage = 0, None, 0
        for n, op, m in _states(ops):
            if stage == 4:
                break
            if op.kind == "lattice_set_closed_loop" or (_is_query(op) and m.kw("lattice_set_closed_loop")["on"] != armed):
                run, shape, stage = 0, None, 0
            elif _is_query(op):
                s = (op.kw.get("E"), op.kw.get("S"))
                if op.kind == kind and stage == 0:
                    run, shape = (run + 1 if s == shape else 1), s
                    stage = int(run >= need)
                elif stage == 1 and op.kind == "lattice_plan" and s[0] != shape[0]:
                    stage = 2
                elif stage == 2 and op.kind == "kmpc_plan":
                    stage = 3
                elif stage == 3 and op.kind == kind and s == shape:
                    stage = 4
        assert stage == 4, f"pattern i: no chain of {need} {kind}, a plan of another E, a kmpc_plan and the chain again"


def _has_j(ops):
    four = ("kmpc_plan", "kmpc_qp_plan", "stmpc_plan", "stmpc_qp_plan")
    seq = [op for op in ops if op.kind in four]
    starts = [k for k in range(len(seq) - 3) if tuple(o.kind for o in seq[k:k + 4]) == four]
    assert len(starts) >= 6, "pattern j: fewer than six interleaved rounds"
    for j, kind in enumerate(four):
        shapes = [(seq[k + j].kw["E"], seq[k + j].kw["T"]) for k in starts]
        trips = list(zip(shapes, shapes[1:], shapes[2:]))
        assert any(x == z and x[0] != y[0] for x, y, z in trips) and any(x == z and x[0] == y[0] and x[1] != y[1] for x, y, z in trips), \
            f"pattern j: {kind} does not change its batch size and its horizon and return"


def _assert_window(ops):
    """pattern b's reuse-window step: two mode-2 plans on an unchanged bitmap, the second's clearance distance inside the window of the
    map the first one built"""
    model, held = Model(), None
    for n, op in enumerate(ops):
        if op.kind in MUTATORS:
            model.apply(n, op)
            if op.kind in _GRID:
                held = None
            continue
        if op.kind != "lattice_plan" or op.tag != "b" or model.kw("lattice_set_mode")["mixed"] != 2 or model.kw("set_grid")["map"] is None:
            if op.kind in ("kmpc_plan", "stmpc_plan"):
                held = None
            continue
        r = model.kw("lattice_set_clearance")["r"]
        if r == 0:
            continue
        want = clear_dist_cells(op.kw, MAPS[model.kw("set_grid")["map"]]["res"], r, model.kw("set_footprint")["on"])
        # (both distances below 8 cells: the clearance mode needs dist <= tile_rows / 4, and the occupancy tile has at least 32 rows)
        if held is not None and want < held <= 1.3 * want + 0.5 and held <= 8.0:
            return
        held = want
    raise AssertionError("no plan inside the clearance map's reuse window")
