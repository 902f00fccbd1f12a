"""Rivals on the GPU (include/f1p.h "Rivals"): k_rivals against the numpy reference of the rule (tests/rivals_ref.py) on two
scenes built for exact ties, coincident vehicles, every race-size path of the kernel and empty slots; the NaN rule, the error codes, E == 1,
the host-array wrapper; and planner.rivals end to end on the three planner classes."""
import ctypes as C
import functools

import numpy as np
import pytest

import rivals_ref as ref
from f1tenth_planning_amd import Rivals, _abi, synth
from f1tenth_planning_amd.runtime import Context, F1PError, lattice_set_obstacles, rivals, rivals_dev, rivals_set_groups

pytestmark = pytest.mark.gpu

RADIUS = 0.375
SIZES = (1, 2, 3, 4, 5, 16, 17, 18, 64, 65)                    # race sizes of scene A: below, at and above M + 1 for M in {1, 4, 16}; one lane stride and one more


@pytest.fixture(scope="module")
def ctx():
    with Context(0) as c:
        yield c


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> dict(x, y, v, h, yaw, beta, groups): scene A -- E = 200 on a 12 x 12 grid of pitch 0.25 (every d2 exact, ties and coincident vehicles in
    plenty), races of SIZES plus five ungrouped egos, ids shuffled over the batch; scene B -- no groups, E = 130: two full lane strides and two more"""
    rng = np.random.default_rng(0)
    E = 200 if name == "A" else 130
    x = rng.integers(0, 12, E) * 0.25
    y = rng.integers(0, 12, E) * 0.25
    v = rng.uniform(-2.0, 6.0, E)
    v[::9] = rng.uniform(-0.5, 0.5, E)[::9]                         # some below min_speed
    h = rng.uniform(-40.0, 40.0, E)                                 # a heading is unbounded here
    h[::17] = rng.uniform(-1.0, 1.0, E)[::17] * 1e6
    beta = rng.uniform(-0.3, 0.3, E)
    groups = None
    if name == "A":
        ids = [11, 3, 2_000_000_000, 7, 0, 500, 42, 43, 8, 1000]    # any values
        groups = np.concatenate([np.full(n, i) for n, i in zip(SIZES, ids)] + [np.array([-1, -7, -1, -2_000_000_000, -3])]).astype(np.int32)
        assert groups.shape == (E,)
        rng.shuffle(groups)
    return dict(x=x, y=y, v=v, h=h, yaw=h - beta, beta=beta, groups=groups)


def states(s, layout):
    E = s["x"].shape[0]
    if layout == ref.XYVYAW:
        return np.column_stack([s["x"], s["y"], s["v"], s["h"]])
    if layout == ref.POSE:
        return np.column_stack([s["x"], s["y"], s["h"], s["v"]])
    rng = np.random.default_rng(1)
    return np.column_stack([s["x"], s["y"], rng.normal(size=E), s["v"], s["yaw"], rng.normal(size=E), s["beta"]])


@functools.lru_cache(maxsize=None)
def want(name, layout, M, reach):
    s = scene(name)
    return ref.rivals(states(s, layout), layout, M, RADIUS, reach=reach, groups=s["groups"])


def compare(got, exp, st, layout):
    """idx exact on every ego; x, y, r, the empty slots and pace bit-equal; vx, vy within 1e-12 * max(1, |v|) (outputs through device trig)"""
    np.testing.assert_array_equal(got["idx"], exp["idx"])
    assert got["obs"][..., [0, 1, 4]].tobytes() == exp["obs"][..., [0, 1, 4]].tobytes()
    empty = exp["idx"] < 0
    assert got["obs"][empty].tobytes() == exp["obs"][empty].tobytes()
    assert got["pace"].tobytes() == exp["pace"].tobytes()
    v = ref.columns(st, layout)[2]
    tol = 1e-12 * np.maximum(1.0, np.abs(np.where(empty, 0.0, v[np.maximum(exp["idx"], 0)])))
    for c in (2, 3):
        err = np.abs(got["obs"][..., c] - exp["obs"][..., c])
        assert (np.isnan(exp["obs"][..., c]) == np.isnan(got["obs"][..., c])).all()
        assert not (err > tol).any(), (c, np.nanmax(err))


def test_scene_properties():
    """what scene A is built to hold: exact ties at the M cut, coincident rivals, slots emptied by reach = 1.0"""
    s = scene("A")
    g, x, y = s["groups"], s["x"], s["y"]
    assert sorted(np.bincount(np.unique(g[g >= 0], return_inverse=True)[1]).tolist()) == sorted(SIZES) and (g < 0).sum() == 5
    coincident = 0
    ties = {1: 0, 4: 0, 16: 0}
    for i in range(200):
        if g[i] < 0:
            continue
        j = np.nonzero((g == g[i]) & (np.arange(200) != i))[0]
        d2 = np.sort((x[j] - x[i]) ** 2 + (y[j] - y[i]) ** 2)
        coincident += bool(d2.size and d2[0] == 0.0)
        for M in ties:
            ties[M] += bool(d2.size > M and d2[M - 1] == d2[M])
    assert coincident >= 20 and all(n >= 30 for n in ties.values()), (coincident, ties)
    for M, least in ((1, 5), (4, 50), (16, 500)):
        full, cut = want("A", ref.XYVYAW, M, np.inf)["idx"], want("A", ref.XYVYAW, M, 1.0)["idx"]
        assert ((cut < 0) & (full >= 0)).sum() >= least


@pytest.mark.parametrize("layout", [ref.XYVYAW, ref.POSE, ref.ST7])
@pytest.mark.parametrize("reach", [np.inf, 1.0])
@pytest.mark.parametrize("M", [1, 4, 16])
@pytest.mark.parametrize("name", ["A", "B"])
def test_kernel_equals_the_reference(ctx, name, M, reach, layout):
    s = scene(name)
    st = states(s, layout)
    rivals_set_groups(ctx, s["groups"])
    got = rivals(ctx, st, layout, M, RADIUS, reach=reach)
    rivals_set_groups(ctx, None)
    compare(got, want(name, layout, M, reach), st, layout)


def test_layout_names_and_batch_equals_dev(ctx):
    s = scene("A")
    E, M = 200, 4
    rivals_set_groups(ctx, s["groups"])
    for layout, nm in ((ref.XYVYAW, "xyvyaw"), (ref.POSE, "pose"), (ref.ST7, "st7")):
        st = states(s, layout)
        a = rivals(ctx, st, nm, M, RADIUS, reach=2.0, min_speed=0.75)
        d_st, d_obs, d_pace, d_idx = ctx.to_device(st), ctx.alloc(40 * E * M), ctx.alloc(8 * E), ctx.alloc(4 * E * M)
        rivals_dev(ctx, d_st, layout, E, M, RADIUS, d_obs, d_pace, d_idx, reach=2.0, min_speed=0.75)
        b = dict(obs=d_obs.download(np.float64, (E, M, 5)), pace=d_pace.download(np.float64, (E,)), idx=d_idx.download(np.int32, (E, M)))
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k
        ctx.lib.f1p_memset(ctx.h, d_obs.ptr, 0x5A, C.c_size_t(40 * E * M))
        rivals_dev(ctx, d_st, nm, E, M, RADIUS, d_obs, reach=2.0)           # pace and idx are optional
        assert d_obs.download(np.float64, (E, M, 5)).tobytes() == a["obs"].tobytes()
        for buf in (d_st, d_obs, d_pace, d_idx):
            buf.free()
    rivals_set_groups(ctx, None)


def test_one_nan_position_blocks_its_race_and_only_its_race(ctx):
    s = scene("A")
    g = s["groups"]
    st = states(s, ref.XYVYAW)
    race = np.nonzero(g == 42)[0]                                    # the race of 17
    assert race.size == 17
    bad = int(race[5])
    st_nan = st.copy(); st_nan[bad, 0] = np.nan
    rivals_set_groups(ctx, g)
    clean = rivals(ctx, st, ref.XYVYAW, 4, RADIUS)
    got = rivals(ctx, st_nan, ref.XYVYAW, 4, RADIUS, reach=0.5)       # (reach does not drop a NaN d2)
    rivals_set_groups(ctx, None)
    compare(got, ref.rivals(st_nan, ref.XYVYAW, 4, RADIUS, reach=0.5, groups=g), st_nan, ref.XYVYAW)
    others = race[race != bad]
    assert (got["idx"][others, 0] == bad).all() and np.isnan(got["obs"][others, 0, 0]).all()      # slot 0 of every member: a NaN slot value blocks
    assert got["idx"][bad].tolist() == others[:4].tolist()           # its own d2 are all NaN: by index
    rest = np.setdiff1d(np.arange(200), race)
    full = rivals(ctx, st_nan, ref.XYVYAW, 4, RADIUS)                 # ungrouped again: one race of all -- everybody's slot 0
    assert (np.delete(full["idx"][:, 0], bad) == bad).all()
    rivals_set_groups(ctx, g)
    got_inf = rivals(ctx, st_nan, ref.XYVYAW, 4, RADIUS)
    rivals_set_groups(ctx, None)
    for k in ("obs", "idx", "pace"):                                 # no ego outside the race sees any difference
        assert got_inf[k][rest].tobytes() == clean[k][rest].tobytes(), k


def test_reach_cut_on_the_device(ctx):
    """d2 == reach^2 is kept, one ulp above is dropped; reach 0 keeps a coincident vehicle only"""
    st = np.column_stack([np.array([[0.0, 0.0], [1.25, 0.0], [-1.25, 2.0 ** -26], [0.0, 0.0]]), np.ones(4), np.zeros(4)])
    for reach, row0 in ((1.25, [3, 1, -1]), (0.0, [3, -1, -1]), (np.inf, [3, 1, 2])):
        got = rivals(ctx, st, ref.XYVYAW, 3, RADIUS, reach=reach)
        assert got["idx"][0].tolist() == row0
        compare(got, ref.rivals(st, ref.XYVYAW, 3, RADIUS, reach=reach), st, ref.XYVYAW)


def test_e_equals_one(ctx):
    for layout, n in ((ref.XYVYAW, 4), (ref.POSE, 4), (ref.ST7, 7)):
        st = np.arange(1.0, n + 1.0)[None]
        got = rivals(ctx, st, layout, 3, RADIUS)
        assert (got["idx"] == -1).all() and (got["obs"] == ref.EMPTY).all()
        assert got["pace"][0] == 1.0 / abs(ref.columns(st, layout)[2][0])
    rivals_set_groups(ctx, [5])
    assert (rivals(ctx, np.ones((1, 4)), 0, 16, RADIUS)["idx"] == -1).all()
    rivals_set_groups(ctx, None)


def test_error_codes_and_nothing_launched(ctx):
    E, M = 6, 2
    st = states(scene("B"), ref.XYVYAW)[:E].copy()
    d_st, d_obs = ctx.to_device(st), ctx.alloc(40 * E * M)
    ctx.lib.f1p_memset(ctx.h, d_obs.ptr, 0x5A, C.c_size_t(40 * E * M))
    obs, pace, idx = np.full((E, M, 5), 7.0), np.full(E, 7.0), np.full((E, M), 7, np.int32)
    ptr = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    nan = float("nan")
    good = dict(layout=0, E=E, M=M, radius=0.3, reach=np.inf, min_speed=0.5, states=True, obs=True)
    bad = [dict(layout=3), dict(layout=-1), dict(M=0), dict(M=17), dict(radius=-0.1), dict(radius=nan), dict(reach=-1.0), dict(reach=nan),
           dict(min_speed=0.0), dict(min_speed=-1.0), dict(min_speed=nan), dict(states=False), dict(obs=False), dict(E=0)]

    def call(dev, **kw):
        a = dict(good, **kw)
        if dev:
            return ctx.lib.f1p_rivals_dev(ctx.h, d_st.ptr if a["states"] else None, a["layout"], a["E"], a["M"], a["radius"], a["reach"], a["min_speed"],
                                          d_obs.ptr if a["obs"] else None, None, None)
        return ctx.lib.f1p_rivals_batch(ctx.h, ptr(st) if a["states"] else None, a["layout"], a["E"], a["M"], a["radius"], a["reach"], a["min_speed"],
                                        ptr(obs) if a["obs"] else None, ptr(pace), ptr(idx))
    for dev in (True, False):
        for kw in bad:
            assert call(dev, **kw) == _abi.F1P_EINVAL, (dev, kw)
            assert b"rivals" in ctx.lib.f1p_last_error(ctx.h)
    rivals_set_groups(ctx, np.zeros(E + 1, np.int32))                # the groups of another E
    for dev in (True, False):
        assert call(dev) == _abi.F1P_ESTATE
        assert b"f1p_rivals_set_groups" in ctx.lib.f1p_last_error(ctx.h)
    with pytest.raises(F1PError) as ei:
        rivals(ctx, st, 0, M, 0.3)
    assert ei.value.code == _abi.F1P_ESTATE
    assert ctx.lib.f1p_rivals_set_groups(ctx.h, ptr(np.zeros(1, np.int32)), 0) == _abi.F1P_EINVAL
    assert call(True) == _abi.F1P_ESTATE                             # a refused set leaves the groups as they were
    rivals_set_groups(ctx, None)
    with pytest.raises(ValueError, match="M must be"):
        rivals(ctx, st, 0, 17, 0.3)
    ctx.sync()
    assert (d_obs.download(np.uint8, (40 * E * M,)) == 0x5A).all()   # nothing was launched
    assert (obs == 7.0).all() and (pace == 7.0).all() and (idx == 7).all()
    assert call(True) == _abi.F1P_OK and call(False) == _abi.F1P_OK  # ... and with everything in order the same calls run
    assert d_obs.download(np.float64, (E, M, 5)).tobytes() == obs.tobytes() and (idx >= 0).all()
    d_st.free(); d_obs.free()


# ---- end to end: planner.rivals on the three classes -------------------------------------------------------------------------------------
E2E, RACES = 48, 6
GROUPS = ((np.arange(E2E) % RACES) * 10 + 3).astype(np.int32)      # six races of 8, interleaved over the batch
RIV = dict(count=3, radius=0.45, reach=6.0)


@functools.lru_cache(maxsize=None)
def pack():
    """48 vehicles on one raceline, six packs of eight: in every pack a fast vehicle closes in on a slow one 0.6 .. 1.2 m ahead of it, so the
    winner of the fast one runs through the slow one's disc -> dict(rl, x, y, psi, v).  Packs 0 and 1 share their stretch of the line: only
    the groups keep them apart."""
    rl = synth.make_raceline(seed=0)
    s = np.concatenate([[0.0], np.cumsum(np.hypot(np.diff(rl[:, 0]), np.diff(rl[:, 1])))])
    calm = np.nonzero(np.abs(rl[:-60, 3]) < 2.0)[0]                  # away from the +-pi seam of the heading column
    bases = calm[np.linspace(0, calm.size - 1, RACES - 1).astype(int)]
    off = np.cumsum([0.0, 0.6, 0.9, 0.6, 1.1, 0.7, 1.2, 0.7])
    speed = np.array([5.0, 1.0, 5.0, 1.0, 4.0, 1.5, 5.0, 1.0])
    x, y, psi, v = (np.empty(E2E) for _ in range(4))
    for e in range(E2E):
        r, m = e % RACES, e // RACES
        b = bases[max(r - 1, 0)]                                     # packs 0 and 1 on the same stretch
        k = min(int(np.searchsorted(s, s[b] + off[m])), len(rl) - 1)
        lat = 0.12 if r == 1 else 0.0
        x[e], y[e], psi[e], v[e] = rl[k, 0] - lat * np.sin(rl[k, 3]), rl[k, 1] + lat * np.cos(rl[k, 3]), rl[k, 3], speed[m]
    return dict(rl=rl, x=x, y=y, psi=psi, v=v)


def moved(p, dt=0.05):
    return dict(p, x=p["x"] + p["v"] * np.cos(p["psi"]) * dt, y=p["y"] + p["v"] * np.sin(p["psi"]) * dt)


def _same(a, b, what):
    assert sorted(a) == sorted(b)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")


def _end_to_end(ctx, make, to_states, layout, plan=lambda p, st: p.plan_batch(st)):
    """A plans with planner.rivals, B with planner.obstacles = runtime.rivals(...)["obs"], two consecutive steps with moved states (the borrowed
    arrays are rewritten in place); every output bit for bit.  Then: at least one winner differs from a plan without rivals, and a call with
    rivals = None after reset() equals a fresh planner's."""
    A, B, fresh = make(), make(), make()
    A.rivals = Rivals(groups=GROUPS, **RIV)
    rivals_set_groups(ctx, GROUPS)
    outs = []
    for step, p in enumerate((pack(), moved(pack()))):
        st = to_states(p)
        r = rivals(ctx, st, layout, RIV["count"], RIV["radius"], reach=RIV["reach"])
        assert (r["idx"][:, 0] >= 0).all()
        a = {k: np.array(v) for k, v in plan(A, st).items()}
        B.obstacles = r["obs"]
        b = plan(B, st)
        _same(a, b, f"step {step}")
        outs.append((st, r, a))
    rivals_set_groups(ctx, None)
    assert A.rivals is not None and B.obstacles is None
    st = outs[0][0]
    free = {k: np.array(v) for k, v in plan(fresh, st).items()}
    changed = outs[0][2]["best_idx"] != free["best_idx"] if "best_idx" in free else outs[0][2]["steer"] != free["steer"]
    assert changed.any(), "no ego changed its winner: the scene does not exercise the rivals"
    A.rivals = None
    if hasattr(A, "reset"):
        A.reset()                                                    # the call counter and the warm start: like with like
    _same({k: np.array(v) for k, v in plan(A, st).items()}, free, "rivals = None")
    return outs, A, B


def test_kmpc_planner_end_to_end(ctx):
    from f1tenth_planning_amd.control.kinematic_mpc.kinematic_mpc import KMPCPlanner, mpc_config
    rl = pack()["rl"]

    def make():
        return KMPCPlanner(waypoints=[rl[:, 0].copy(), rl[:, 1].copy(), rl[:, 3].copy(), rl[:, 2].copy()],
                           config=mpc_config(N_ROLLOUTS=128, SEED=5, COLLISION_SUBSTEPS=2))
    _end_to_end(ctx, make, lambda p: np.column_stack([p["x"], p["y"], p["v"], p["psi"]]), ref.XYVYAW)


def test_stmpc_planner_end_to_end(ctx):
    from f1tenth_planning_amd.control.dynamic_mpc.dynamic_mpc import STMPCPlanner, mpc_config
    rl = pack()["rl"]

    def make():
        return STMPCPlanner(waypoints=[rl[:, 0].copy(), rl[:, 1].copy(), rl[:, 3].copy(), rl[:, 2].copy()],
                            config=mpc_config(N_ROLLOUTS=128, SEED=5, COLLISION_SUBSTEPS=2, COLLISION_SUBSTEPS_K=2))

    def to_states(p):
        z = np.zeros(E2E)
        return np.column_stack([p["x"], p["y"], z, p["v"], p["psi"] - 0.01, z, z + 0.01])      # (heading = yaw + beta)
    outs, _, _ = _end_to_end(ctx, make, to_states, ref.ST7)
    assert set(outs[0][2]["branch"].tolist()) == {0, 1}             # both models of the batch took their rivals


def test_lattice_planner_end_to_end(ctx):
    from f1tenth_planning_amd.planning.lattice_planner.lattice_planner import LatticePlanner
    rl = pack()["rl"]

    def make():
        p = LatticePlanner(waypoints=rl, device=0)
        p.configure(lookahead_distances=np.linspace(0.6, 3.0, 8), widths=np.linspace(-1.0, 1.0, 5), num_stations=20)
        return p

    def to_states(p):
        return np.column_stack([p["x"], p["y"], p["psi"], p["v"]])
    outs, A, B = _end_to_end(ctx, make, to_states, ref.POSE)
    # the returned pace is the one the class forms on the host for explicit obstacles ...
    st, r, a = outs[1]
    assert r["pace"].tobytes() == (1.0 / np.maximum(np.abs(st[:, 3]), B.obstacle_min_speed)).tobytes()
    bctx = B._context()
    lattice_set_obstacles(bctx, r["obs"], r["pace"])                 # ... and at the context level it gives the same plan
    _same(a, bctx.lattice_plan(st, B._cfg()), "obs and pace through lattice_set_obstacles")
    lattice_set_obstacles(bctx, None)
    # step_batch: the same feed
    keys = ("steer", "speed", "status")
    A.rivals = Rivals(groups=GROUPS, **RIV)
    for st, r, a in outs:
        got = {k: np.array(v) for k, v in A.step_batch(st).items()}
        B.obstacles = r["obs"]
        _same(got, {k: np.array(v) for k, v in B.step_batch(st).items()}, "step_batch")
        _same({k: got[k] for k in keys}, {k: a[k] for k in keys}, "step_batch against plan_batch")
