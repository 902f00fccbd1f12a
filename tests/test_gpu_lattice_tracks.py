"""Lattice plans on a track set (f1p_lattice_plan_tracks_* / f1p_lattice_step_tracks_batch): ego e plans along track track_id[e].

Bar: each ego's outputs are BIT-identical to f1p_lattice_plan_* on a second context with the same map whose raceline is that ego's track
(steer, speed, best_idx, best_cost, status, near_idx, fp64 / f32 rows; NaN patterns included), on every path the single-raceline call
takes: f1p_lattice_set_mode 0-3, clothoid and cubic, oriented footprint, clearance 0 / 2, no map, host goals, candidate slices, page-locked
arrays (zero-copy, sliced past 8192 egos), the pipeline, MultiContext; and against the oracle at the bars of lattice_helpers.compare."""
import numpy as np
import pytest

from f1tenth_planning_amd import _abi, synth
from lattice_helpers import batch_cuts, compare, edge_egos

pytestmark = pytest.mark.gpu
RES = 0.058
KEYS = ("steer", "speed", "best_idx", "best_cost", "status", "near_idx", "best_traj")


def _turn(rl, ang, dx, dy):
    """a moved and turned copy of a raceline [x, y, v, psi, kappa]"""
    c, s = np.cos(ang), np.sin(ang)
    out = rl.copy()
    out[:, 0] = c * rl[:, 0] - s * rl[:, 1] + dx
    out[:, 1] = s * rl[:, 0] + c * rl[:, 1] + dy
    out[:, 3] = rl[:, 3] + ang
    return out


def _lane(rl, off):
    """the raceline offset sideways by `off` metres (a lane of it), its own speed profile"""
    out = rl.copy()
    out[:, 0] -= off * np.sin(rl[:, 3]); out[:, 1] += off * np.cos(rl[:, 3])
    out[:, 2] = rl[:, 2] * (1.0 + 0.1 * off)
    return out


def _poly(n, seed, radius, cx, cy):
    rng = np.random.default_rng(seed)
    a = np.linspace(0.0, 1.7 * np.pi, n) + rng.uniform(0, 1)
    r = radius + rng.normal(0, 0.02, n)
    x, y = cx + r * np.cos(a), cy + r * np.sin(a)
    return np.column_stack([x, y, rng.uniform(1, 8, n), a + np.pi / 2, np.full(n, 1.0 / radius)])


@pytest.fixture(scope="module")
def scene(golden):
    rl = synth.make_raceline(seed=0)
    img, origin = synth.make_grid(rl[:, :2], size=(2000, 2000), resolution=RES)
    img, _ = synth.stamp_obstacles(img, origin, RES, rl, spacing=10.0, radius=0.30)
    g = golden("tracks.npz")
    cx, cy = rl[:, 0].mean(), rl[:, 1].mean()
    tr = [_lane(rl, -0.5), rl.copy(), _lane(rl, 0.5), g["spielberg"][:, :5].copy(), g["levine"][:, [1, 2, 5, 3, 4]].copy()]
    for i, n in enumerate((2, 3, 64, 65, 2049, 2113, 4097, 5000)):
        tr.append(_poly(n, seed=50 + i, radius=3.0 + 0.004 * n, cx=cx + 2.0 * i, cy=cy - 1.5 * i))
    dup = np.repeat(_poly(300, seed=7, radius=8.0, cx=cx, cy=cy), 2, axis=0)[:500]   # zero-length segments
    tr.append(dup)
    far = rl.copy(); far[:, :2] += 1.0e5                                              # infinite chunk boxes in f32
    tr.append(far)
    return rl, img, origin, [np.ascontiguousarray(t) for t in tr]


def _egos(tracks, E, seed):
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, len(tracks), E).astype(np.int32)
    poses = np.empty((E, 4))
    for e in range(E):
        t = tracks[ids[e]]
        j = rng.integers(0, t.shape[0])
        poses[e, :2] = t[j, :2] + rng.normal(0, 0.2, 2)
        poses[e, 2] = t[j, 3] + rng.normal(0, 0.1)
        poses[e, 3] = rng.uniform(0.5, 6.0)
    return ids, poses


def _ctx(scene, grid=True, mode=1):
    from f1tenth_planning_amd.runtime import Context
    rl, img, origin, tr = scene
    c = Context(0)
    if grid:
        c.set_grid(img, RES, origin, 206)
    c.lattice_set_mode(mode)
    return c


@pytest.fixture(scope="module")
def pair(scene):
    a, b = _ctx(scene), _ctx(scene)
    a.set_tracks(scene[3])
    yield a, b
    a.close(); b.close()


def _reference(ref, tracks, ids, plan):
    """plan(mask) with ref's raceline = track k, for every k, scattered into ego order"""
    out = None
    for k, t in enumerate(tracks):
        m = ids == k
        if not m.any():
            continue
        ref.set_waypoints(t)
        o = plan(m)
        if out is None:
            out = {key: np.empty((len(ids),) + v.shape[1:], v.dtype) for key, v in o.items()}
        for key, v in o.items():
            out[key][m] = v
    return out


def _same(got, want, what):
    for k in want:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape, f"{what}: {k}"
        if a.tobytes() != b.tobytes():
            bad = np.unique(np.argwhere(a.reshape(len(a), -1).view(np.uint8) != b.reshape(len(b), -1).view(np.uint8))[:, 0])
            raise AssertionError(f"{what}: {k} differs for {len(bad)} egos, first {bad[:8]}")


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("gen", ["clothoid", "cubic"])
def test_modes_and_generators_bit_identical(pair, scene, mode, gen):
    ctx, ref = pair
    tr = scene[3]
    cfg = synth.bench_lattice_cfg(n_cand=256, n_stations=50, generator=gen, prune=True)
    ids, poses = _egos(tr, 1536, seed=11 + mode)
    ctx.lattice_set_mode(mode); ref.lattice_set_mode(mode)
    got = ctx.lattice_plan_tracks(poses, ids, cfg)
    assert len(np.unique(got["status"])) >= 2
    want = _reference(ref, tr, ids, lambda m: ref.lattice_plan(poses[m], cfg))
    _same(got, want, f"mode {mode} {gen}")
    ctx.lattice_set_mode(1); ref.lattice_set_mode(1)


@pytest.mark.parametrize("shape", ["footprint", "clear0", "nomap", "host_goals", "f32", "prev_theta", "all"])
def test_plan_shapes_bit_identical(scene, shape):
    tr = scene[3]
    a, b = _ctx(scene, grid=shape != "nomap"), _ctx(scene, grid=shape != "nomap")
    try:
        a.set_tracks(tr)
        cfg = synth.bench_lattice_cfg(n_cand=256, n_stations=50, prune=True)
        if shape == "nomap":
            cfg.check_collision = 0
        E = 96 if shape == "all" else 1200
        ids, poses = _egos(tr, E, seed=23)
        kw, g, pt = {}, None, None
        if shape == "footprint":
            for c in (a, b):
                c.set_footprint([-0.2, 0.0, 0.2], 0.16)
        if shape == "clear0":
            a.lattice_set_clearance(0); b.lattice_set_clearance(0)
        if shape == "host_goals":
            rng = np.random.default_rng(5)
            g = np.column_stack([rng.uniform(0.5, 3.0, E * 256), rng.uniform(-1, 1, E * 256), rng.uniform(-0.5, 0.5, E * 256)]).reshape(E, 256, 3)
        if shape == "f32":
            kw["traj_dtype"] = np.float32
        if shape == "prev_theta":
            pt = np.random.default_rng(6).normal(0, 0.2, (E, 50))
        if shape == "all":
            kw["want_all"] = True
        got = a.lattice_plan_tracks(poses, ids, cfg, goals=g, prev_theta=pt, **kw)
        want = _reference(b, tr, ids, lambda m: b.lattice_plan(poses[m], cfg, goals=None if g is None else g[m],
                                                               prev_theta=None if pt is None else pt[m], **kw))
        _same(got, want, shape)
    finally:
        a.close(); b.close()


def test_candidate_slices_few_egos_many_candidates(scene):
    tr = scene[3]
    a, b = _ctx(scene, mode=0), _ctx(scene, mode=0)
    try:
        a.set_tracks(tr)
        cfg = _abi.lattice_cfg(lookaheads=np.linspace(0.6, 3.0, 32), widths=np.linspace(-1, 1, 32), n_stations=50, prune=True)
        ids, poses = _egos(tr, 7, seed=31)
        for G in (0, 4):
            a.lattice_set_split(G); b.lattice_set_split(G)
            got = a.lattice_plan_tracks(poses, ids, cfg)
            want = _reference(b, tr, ids, lambda m: b.lattice_plan(poses[m], cfg))
            _same(got, want, f"split {G}")
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("E,pin,chunks", [(33, True, 0), (4095, True, 0), (12289, True, 0), (5003, False, 3)])
def test_batch_cuts(pair, scene, E, pin, chunks):
    ctx, ref = pair
    tr = scene[3]
    cfg = synth.bench_lattice_cfg(n_cand=256, n_stations=50, prune=True)
    ids, poses = _egos(tr, E, seed=E)
    cuts = batch_cuts(E, chunks=(chunks,) if chunks else ())
    edges = edge_egos(cuts)
    ctx.lattice_set_pipeline(chunks)
    try:
        got = ctx.lattice_plan_tracks(poses, ids, cfg, reuse_outputs=pin)
        got = {k: np.array(v) for k, v in got.items()}
    finally:
        ctx.lattice_set_pipeline(0)
    want = _reference(ref, tr, ids, lambda m: ref.lattice_plan(poses[m], cfg))
    _same(got, want, f"E {E}")
    assert all(0 <= e < E for e in edges) and got["status"][edges].min() >= 0


def test_multicontext_two_ranges(scene):
    from f1tenth_planning_amd.runtime import MultiContext
    tr = scene[3]
    rl, img, origin, _ = scene
    mc = MultiContext([0, 0])
    a = _ctx(scene)
    try:
        mc.set_grid(img, RES, origin, 206)
        mc.set_tracks(tr); a.set_tracks(tr)
        cfg = synth.bench_lattice_cfg(n_cand=256, n_stations=50, prune=True)
        ids, poses = _egos(tr, 3001, seed=4)
        _same(mc.lattice_plan_tracks(poses, ids, cfg), a.lattice_plan_tracks(poses, ids, cfg), "MultiContext")
    finally:
        mc.close(); a.close()


def test_bad_ids_and_errors(pair, scene):
    ctx, ref = pair
    tr = scene[3]
    K = len(tr)
    cfg = synth.bench_lattice_cfg(n_cand=256, n_stations=50, prune=True)
    ids, poses = _egos(tr, 2048, seed=77)
    bad_ids = ids.copy()
    bad = np.arange(3, 2048, 37)
    bad_ids[bad] = np.resize(np.array([-1, K, np.iinfo(np.int32).min, np.iinfo(np.int32).max], np.int32), len(bad))
    for mode in (1, 0):
        ctx.lattice_set_mode(mode)
        good = ctx.lattice_plan_tracks(poses, ids, cfg)
        got = ctx.lattice_plan_tracks(poses, bad_ids, cfg)
        ok = np.ones(2048, bool); ok[bad] = False
        _same({k: v[ok] for k, v in got.items()}, {k: v[ok] for k, v in good.items()}, f"mode {mode} others")
        assert np.isnan(got["steer"][bad]).all() and np.isnan(got["speed"][bad]).all() and np.isnan(got["best_cost"][bad]).all()
        assert (got["best_idx"][bad] == -1).all() and (got["near_idx"][bad] == -1).all()
        assert (got["status"][bad] == _abi.ST_BAD_TRACK).all() and (got["best_traj"][bad] == 0).all()
    ctx.lattice_set_mode(1)
    lib, h = ctx.lib, ctx.h
    import ctypes as C
    z = np.zeros(4); o = np.zeros(1); oi = np.zeros(1, np.int32); tid = np.zeros(1, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    sh = synth.bench_lattice_cfg(n_cand=256, n_stations=50); sh.cand_count = 16
    EINVAL = -1
    assert lib.f1p_lattice_plan_tracks_batch(h, p(z), None, None, p(tid), 1, C.byref(sh), None, None, p(oi), p(o), None, p(oi), None, None, None) == EINVAL
    assert lib.f1p_lattice_plan_tracks_batch(h, p(z), None, None, None, 1, C.byref(cfg), p(o), p(o), p(oi), None, None, None, None, None, None) == EINVAL
    assert lib.f1p_lattice_step_tracks_batch(h, p(z), None, 1, C.byref(cfg), p(o), p(o), None, 0) == EINVAL
    # no track set; a set without a heading column with device goals (host goals still plan); no raceline needed
    from f1tenth_planning_amd.runtime import Context, F1PError
    c = Context(0)
    try:
        with pytest.raises(F1PError):
            c.lattice_plan_tracks(poses[:4], ids[:4] * 0, cfg)
        c.set_tracks([t[:, :3] for t in tr])
        with pytest.raises(F1PError):
            c.lattice_plan_tracks(poses[:4], ids[:4], cfg)
        g = np.tile(np.array([[1.0, 0.0, 0.0]]), (4, 256, 1))
        assert c.lattice_plan_tracks(poses[:4], ids[:4], cfg, goals=g)["status"].shape == (4,)
        c.set_tracks(tr)
        free = synth.bench_lattice_cfg(n_cand=256, n_stations=50, prune=True)
        free.check_collision = 0                                                   # (this context has no map)
        out = c.lattice_plan_tracks(poses[:64], ids[:64], free)                    # a context without a raceline plans
        want = _reference(ref, tr, ids[:64], lambda m: ref.lattice_plan(poses[:64][m], free))
        _same(out, want, "no raceline")
    finally:
        c.close()


def test_closed_loop_step_chain_and_audit(scene):
    tr = [_turn(scene[0], 0.3 * k, 4.0 * k, -3.0 * k) for k in range(8)]
    a, b = _ctx(scene, grid=False), _ctx(scene, grid=False)
    try:
        for c in (a, b):
            c.set_tracks(tr)
        cfg = synth.bench_lattice_cfg(n_cand=256, n_stations=50, prune=True)
        cfg.check_collision = 0
        E = 4096
        ids, poses = _egos(tr, E, seed=8)
        prev = None
        for step in range(200):
            s = a.lattice_step_tracks(poses, ids, cfg, keep_traj=True)
            p = b.lattice_plan_tracks(poses, ids, cfg, prev_theta=prev)
            np.testing.assert_array_equal(s["steer"], p["steer"]); np.testing.assert_array_equal(s["speed"], p["speed"])
            np.testing.assert_array_equal(s["status"], p["status"])
            np.testing.assert_array_equal(a.lattice_fetch_traj(E, 50), p["best_traj"])
            prev = p["best_traj"][:, :, 2].copy()
            sp = np.nan_to_num(p["speed"]) * 0.02
            poses[:, 0] += sp * np.cos(poses[:, 2]); poses[:, 1] += sp * np.sin(poses[:, 2])
            poses[:, 2] += np.nan_to_num(p["steer"]) * 0.02
        a.lattice_set_audit(1, 256)
        a.lattice_audit_read(reset=True)
        for _ in range(3):
            a.lattice_plan_tracks(poses, ids, cfg)
        au = a.lattice_audit_read()
        assert au["plans"] >= 3 and au["egos"] > 0 and au["mismatching_egos"] == 0
    finally:
        a.close(); b.close()


def test_oracle_contact(scene, orc):
    rl, img, origin, _ = scene
    grid = (img, RES, origin[0], origin[1], 206)
    cfg = synth.bench_lattice_cfg(n_cand=256, n_stations=50)
    for E, K in ((4096, 8), (65536, 256)):
        tr = [_turn(rl, 0.0, 0.0, 0.0)] + [_lane(rl, 0.8 * ((k % 5) / 4.0 - 0.5)) for k in range(1, K)]
        a = _ctx(scene)
        try:
            a.set_tracks(tr)
            ids = np.random.default_rng(K).integers(0, K, E).astype(np.int32)
            poses = np.empty((E, 4))
            ego = synth.make_egos(rl, E, seed=K)
            poses[:] = ego
            got = a.lattice_plan_tracks(poses, ids, cfg)
            sub = np.arange(0, E, E // 256)
            want = {k: np.empty((len(sub),) + got[k].shape[1:], got[k].dtype) for k in KEYS}
            for k in np.unique(ids[sub]):
                m = ids[sub] == k
                o = orc.lattice_plan_batch(poses[sub][m], tr[k], cfg, grid=grid)
                for key in KEYS:
                    want[key][m] = o[key]
            compare({k: got[k][sub] for k in KEYS}, want)
        finally:
            a.close()


def test_classes(scene):
    from f1tenth_planning_amd.planning.lane_switcher.lane_switcher import LaneSwitcherPlanner
    from f1tenth_planning_amd.planning.lattice_planner.lattice_planner import LatticePlanner
    rl = scene[0]
    tr = [_lane(rl, o) for o in (-0.4, 0.0, 0.4)]
    ids = np.random.default_rng(2).integers(0, 3, 300).astype(np.int32)
    poses = np.asarray(synth.make_egos(rl, 300, seed=2), np.float64)[:, :4]
    lp = LatticePlanner(waypoints=rl)
    out = lp.plan_batch(poses, tracks=tr, track_ids=ids)
    c = lp._context()
    _same(out, c.lattice_plan_tracks(poses, ids, lp._cfg()), "LatticePlanner")
    _same(lp.plan_batch(poses, tracks=tr, track_ids=ids, devices=[0]), out, "devices")
    with pytest.raises(ValueError):
        lp.plan_batch(poses, tracks=tr)
    ls = LaneSwitcherPlanner(waypoints=rl)
    o2 = ls.plan_batch(poses, tracks=tr, track_ids=ids)
    assert o2["lane"].shape == (300,) and set(np.unique(o2["lane"])) <= {-1, 0, 1, 2}
    st = poses.copy()                                                 # a kinematic closed loop: every step's commands move the egos
    for _ in range(20):
        s = lp.step_batch(st, tracks=tr, track_ids=ids)
        assert np.isfinite(s["steer"]).all()
        sp = s["speed"] * 0.02
        st[:, 0] += sp * np.cos(st[:, 2]); st[:, 1] += sp * np.sin(st[:, 2]); st[:, 2] += s["steer"] * 0.02
