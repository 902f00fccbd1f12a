"""Lattice batches past 4096 egos: every host / kernel path the library picks by batch size, at the sizes where it cuts a batch, against the
all-fp64 exhaustive kernel on EVERY ego and against the oracle on the egos around every cut.

Paths (f1p_lattice.hip lattice_plan_batch_impl, k_lattice_mixed.hip): the staged path with the one-copy gather of the result columns (packed up
to 1 MB, partly per array above it), page-locked rows planned in min(E / 4096, 8) slices with the rows' D2H on a second stream (fp64 and f32
rows), page-locked columns without rows, device buffers, the plan pipelined in 2 / 3 / 8 chunks on two streams (two-egos-per-wave prologue
from 3072 egos a chunk), and f1p_lattice_step_batch.  Sizes: 8192 (2 slices), 12 289 (3, odd split), 20 483 (5, uneven), 32 768 (8:
BASELINE configs[3]) and 36 865 (9 by E / 4096, capped at 8).  The scene has obstacles on the raceline (several refinement entries an ego,
a mix of statuses); off-map, NaN-x, inf-yaw and raceline-seam egos sit at the first and the last ego of every slice and chunk.

Stale data never passes as a result: the outputs a path reuses (page-locked arrays, device buffers) are filled with NaN / -1 before every
call, and consecutive calls alternate two pose sets.  Each path plans three times in a row (the second and third plan of a batch size take
the dispatch order the previous one left, and the page-locked arrays it allocated).
"""
import numpy as np
import pytest

from f1tenth_planning_amd import _abi, synth
from lattice_helpers import batch_cuts, compare, edge_egos

pytestmark = pytest.mark.gpu
RES = 0.058
SIZES = (8192, 12289, 20483, 32768, 36865)
N_CAND, N_ST = 256, 50
PIPE = (2, 3, 8)
KINDS = ("off_map", "nan_x", "inf_yaw", "seam")


@pytest.fixture(scope="module")
def scene():
    rl = synth.make_raceline(seed=0)
    img, origin = synth.make_grid(rl[:, :2], size=(2000, 2000), resolution=RES)
    img, _ = synth.stamp_obstacles(img, origin, RES, rl, spacing=10.0, radius=0.30)
    return rl, img, origin, (img, RES, origin[0], origin[1], 206)


@pytest.fixture(scope="module")
def cfg():
    return synth.bench_lattice_cfg(n_cand=N_CAND, n_stations=N_ST)      # weights (0.25,) * 4: the similarity term carries weight


def _context(scene, device=0, mode=1):
    from f1tenth_planning_amd.runtime import Context
    rl, img, origin, _ = scene
    c = Context(device)
    c.set_waypoints(rl); c.set_grid(img, RES, origin, 206)
    c.lattice_set_mode(mode)
    return c


@pytest.fixture(scope="module")
def ctxs(scene):
    """(the context under test: default schedule, the reference: all-fp64 exhaustive kernel)"""
    a, ref = _context(scene), _context(scene, mode=0)
    yield a, ref
    a.close(); ref.close()


def _plant(poses, rl, at, shift, rng):
    """the position j of `at` gets kind (j + shift) % 4: shifting by one between pose sets gives every planted ego another kind in the other set"""
    n = len(rl)                                                    # (the raceline is closed: row n - 1 repeats row 0)
    for j, e in enumerate(at):
        kind = KINDS[(j + shift) % len(KINDS)]
        if kind == "off_map":
            poses[e, :2] += 400.0
        elif kind == "nan_x":
            poses[e, 0] = np.nan
        elif kind == "inf_yaw":
            poses[e, 2] = np.inf
        else:
            w = (0, 1, n - 3, n - 2)[(j // len(KINDS)) % 4]
            poses[e, :2] = rl[w, :2] + rng.normal(0, 0.2, 2)
            poses[e, 2] = rl[w, 3] + rng.normal(0, 0.1)


def _make_poses(rl, E, cuts, seed):
    """two pose sets of E egos, the first and last ego of every range between `cuts` and a few odd egos planted; the planted egos"""
    planted = sorted(set(edge_egos(cuts)) | {1, 2, E // 3, E // 2 + 1, E - 2})
    rng = np.random.default_rng(seed)
    sets = []
    for shift in (0, 1):
        p = synth.make_egos(rl, E, seed=seed + shift, pos_sigma=0.35, yaw_sigma=0.2)
        _plant(p, rl, planted, shift, rng)
        sets.append(p)
    return sets, planted


def _subset(E, cuts, planted, n_max=768):
    """the egos the oracle sees: the four egos on either side of every cut (the selection kernel takes four egos a workgroup, the prologue two a
    wave), the planted ones, a stride over the rest"""
    near = {e for c in cuts for e in range(c - 4, c + 4) if 0 <= e < E} | set(planted)
    stride = max(1, E // max(n_max - len(near), 1))
    return np.array(sorted(near | set(range(3, E, stride))))


@pytest.fixture(scope="module", params=SIZES, ids=lambda E: f"E{E}")
def case(request, scene, cfg, ctxs):
    E = request.param
    rl = scene[0]
    cuts = batch_cuts(E, PIPE)
    poses, planted = _make_poses(rl, E, cuts, seed=E)
    refs = [ctxs[1].lattice_plan(p, cfg) for p in poses]
    return dict(E=E, cuts=cuts, planted=planted, poses=poses, refs=refs, sub=_subset(E, cuts, planted))


def _poison(out):
    for a in out.values():
        a[...] = -1 if a.dtype.kind == "i" else np.nan


def _same(got, want, what, f32=False):
    for k, v in got.items():
        w = want[k].astype(np.float32) if (f32 and k == "best_traj") else want[k]
        np.testing.assert_array_equal(np.asarray(v), w, err_msg=f"{what}: {k}")


class _DevPath:
    """lattice_plan_dev on device buffers, every output buffer filled with NaN / -1 before the plan"""
    OUT = (("steer", np.float64, ()), ("speed", np.float64, ()), ("best_idx", np.int32, ()), ("best_cost", np.float64, ()),
           ("status", np.int32, ()), ("near_idx", np.int32, ()), ("best_traj", np.float64, (N_ST, 4)))

    def __init__(self, ctx, E):
        self.ctx, self.E = ctx, E
        self.bufs = {k: (ctx.alloc(np.dtype(t).itemsize * E * int(np.prod(sh, dtype=np.int64))), t, (E,) + sh) for k, t, sh in self.OUT}
        self.d_poses = ctx.alloc(32 * E)

    def __call__(self, poses, cfg):
        for b, t, sh in self.bufs.values():
            b.upload(np.full(sh, -1 if np.dtype(t).kind == "i" else np.nan, t))
        self.d_poses.upload(poses)
        B = {k: v[0] for k, v in self.bufs.items()}
        self.ctx.lattice_plan_dev(self.d_poses, self.E, cfg, B["steer"], B["speed"], B["best_idx"], B["best_cost"], B["status"], B["near_idx"], B["best_traj"])
        self.ctx.sync()
        return {k: b.download(t, sh) for k, (b, t, sh) in self.bufs.items()}

    def free(self):
        for b, _, _ in self.bufs.values():
            b.free()
        self.d_poses.free()


def _pipelined(ctx, k, **kw):
    def plan(poses, cfg):
        ctx.lattice_set_pipeline(k)
        try:
            return ctx.lattice_plan(poses, cfg, **kw)
        finally:
            ctx.lattice_set_pipeline(1)
    return plan


def _step(ctx, fresh_chain=True):
    def plan(poses, cfg):
        if fresh_chain:
            ctx.lattice_set_closed_loop(False)                    # the first step of a fresh chain: no similarity term
        out = ctx.lattice_step(poses, cfg, keep_traj=True)
        out["best_traj"] = ctx.lattice_fetch_traj(len(poses), cfg.n_stations)
        return out
    return plan


def _paths(ctx, dev):
    """name -> (plan(poses, cfg) -> outputs, rows are f32)"""
    paths = {
        "default schedule, pageable (staged + gather)": (lambda p, c: ctx.lattice_plan(p, c), False),
        "page-locked fp64 rows (sliced)": (lambda p, c: ctx.lattice_plan(p, c, reuse_outputs=True), False),
        "page-locked f32 rows (sliced <float>)": (lambda p, c: ctx.lattice_plan(p, c, reuse_outputs=True, traj_dtype=np.float32), True),
        "page-locked, no rows": (lambda p, c: ctx.lattice_plan(p, c, reuse_outputs=True, want_traj=False), False),
        "device buffers": (dev, False),
    }
    for k in PIPE:
        paths[f"pipelined in {k} chunks"] = (_pipelined(ctx, k), False)
    paths["step + fetch_traj"] = (_step(ctx), False)
    return paths


def test_every_path_equals_the_fp64_reference_on_every_ego(ctxs, cfg, case):
    ctx, _ = ctxs
    E, poses, refs = case["E"], case["poses"], case["refs"]
    for r in refs:                                                 # the scene does what it is for
        st = r["status"]
        assert (st == _abi.ST_INTERSECT).mean() > 0.8 and (st == _abi.ST_ALL_BLOCKED).sum() >= len(case["planted"]) // 2
    dev = _DevPath(ctx, E)
    try:
        for name, (plan, f32) in _paths(ctx, dev).items():
            out = None
            for i in (1, 0, 1):
                if out is not None:
                    _poison(out)
                out = plan(poses[i], cfg)
                _same(out, refs[i], f"{name}, E {E}, pose set {i}", f32=f32)
                if f32:
                    assert out["best_traj"].dtype == np.float32
            if name.startswith("default"):
                assert (ctx.lattice_debug_queue(E) >= 2).any()     # egos with several refinement entries
    finally:
        dev.free()


def test_cut_egos_vs_oracle(ctxs, cfg, case, scene, orc):
    """the reference (every path equals it bit for bit), the default schedule and the f32 rows against the oracle on the egos around every cut"""
    ctx, _ = ctxs
    rl, grid = scene[0], scene[3]
    sub, poses, ref = case["sub"], case["poses"][0], case["refs"][0]
    want = orc.lattice_plan_batch(poses[sub], rl, cfg, grid=grid, nthreads=orc.max_threads())
    compare({k: v[sub] for k, v in ref.items()}, want)
    got = ctx.lattice_plan(poses, cfg)
    compare({k: v[sub] for k, v in got.items()}, want)
    f32 = ctx.lattice_plan(poses, cfg, reuse_outputs=True, traj_dtype=np.float32)
    _, d = compare({k: np.asarray(v)[sub] for k, v in f32.items()}, want, tol_traj=1e-4)
    assert d < 2e-6                                                # what f32 gives on a 4 m path
    assert set(np.unique(want["status"])) >= {_abi.ST_INTERSECT, _abi.ST_ALL_BLOCKED}


def test_runtime_audit_over_every_path(ctxs, cfg, case):
    """f1p_lattice_set_audit(1, 256): every mixed plan of each path re-planned on a window of egos by the all-fp64 kernel, bit for bit"""
    ctx, _ = ctxs
    dev = _DevPath(ctx, case["E"])
    try:
        for name, (plan, _) in _paths(ctx, dev).items():
            ctx.lattice_audit_read(reset=True)
            ctx.lattice_set_audit(1, 256)
            try:
                plan(case["poses"][0], cfg)
            finally:
                ctx.lattice_set_audit(0)
            audit = ctx.lattice_audit_read(reset=True)
            assert audit["egos"] > 0 and audit["mismatching_egos"] == 0, (name, audit)
    finally:
        dev.free()


def _drive(poses, k, step=0.08):
    p = poses.copy()
    ok = np.isfinite(p).all(axis=1)
    p[ok, 0] += step * k * np.cos(p[ok, 2]); p[ok, 1] += step * k * np.sin(p[ok, 2])
    return p


def _reference_chain(ref_ctx, chain, cfg):
    """each link planned by the all-fp64 kernel with the previous link's winner headings as explicit prev_theta"""
    out, prev = [], None
    for p in chain:
        out.append(ref_ctx.lattice_plan(p, cfg, prev_theta=prev))
        prev = out[-1]["best_traj"][:, :, 2].copy()
    return out


def test_closed_loop_chain(ctxs, cfg, case, scene, orc):
    """a chain of three closed-loop plans (the previous winners' headings kept on the device: similarity term) through the sliced path, the
    pipelined path and f1p_lattice_step_batch; every link equal to the all-fp64 plan given the previous link's headings, the last against the oracle"""
    ctx, ref_ctx = ctxs
    rl, grid = scene[0], scene[3]
    chain = [_drive(case["poses"][k % 2], k) for k in range(3)]
    want = _reference_chain(ref_ctx, chain, cfg)
    heads = [w["best_traj"][:, :, 2] for w in want]
    routes = {"sliced": lambda p, c: ctx.lattice_plan(p, c, reuse_outputs=True), "pipelined in 3 chunks": _pipelined(ctx, 3)}
    for name, plan in routes.items():
        ctx.lattice_set_closed_loop(True)
        try:
            out = None
            for k, p in enumerate(chain):
                if out is not None:
                    _poison(out)
                    np.testing.assert_array_equal(ctx.lattice_closed_loop_prev(), heads[k - 1], err_msg=f"{name}: headings in front of link {k}")
                out = plan(p, cfg)
                _same(out, want[k], f"{name}, link {k}")
        finally:
            ctx.lattice_set_closed_loop(False)
    step, out = _step(ctx, fresh_chain=False), None
    ctx.lattice_set_closed_loop(False)                             # a fresh step chain
    for k, p in enumerate(chain):
        if out is not None:
            _poison(out)
        out = step(p, cfg)
        _same(out, want[k], f"step, link {k}")
    np.testing.assert_array_equal(ctx.lattice_closed_loop_prev(), heads[2])
    ctx.lattice_set_closed_loop(False)
    sub = case["sub"]
    orc_last = orc.lattice_plan_batch(chain[2][sub], rl, cfg, grid=grid, prev_theta=heads[1][sub], nthreads=orc.max_threads())
    compare({k: v[sub] for k, v in want[2].items()}, orc_last)
    open_loop = ref_ctx.lattice_plan(chain[2], cfg)
    assert (open_loop["best_cost"] != want[2]["best_cost"]).any()    # the similarity term is live


def test_configs3_through_multicontext(ctxs, cfg, scene, orc):
    """BASELINE configs[3]: 32 768 egos x 256 candidates x 50 stations sharded over 8 contexts (8 GPUs when there are, else 8 contexts on
    GPU 0: one process, 8 host threads); bit-identical to one context planning the whole batch, open and closed loop; the oracle on the egos
    around every shard edge"""
    from f1tenth_planning_amd.runtime import MultiContext
    ctx, _ = ctxs
    rl, img, origin, grid = scene
    E, G = 32768, 8
    devices = list(range(G)) if _abi.load_library().f1p_device_count() >= G else [0] * G
    cuts = batch_cuts(E, chunks=(), shards=G)
    poses, planted = _make_poses(rl, E, cuts, seed=3)
    with MultiContext(devices) as mc:
        mc.set_waypoints(rl); mc.set_grid(img, RES, origin, 206)
        many = mc.lattice_plan(poses[0], cfg)
        one = ctx.lattice_plan(poses[0], cfg)
        assert sorted(many) == sorted(one)
        _same(many, one, "MultiContext vs one context")
        sub = _subset(E, cuts, planted, n_max=512)
        want = orc.lattice_plan_batch(poses[0][sub], rl, cfg, grid=grid, nthreads=orc.max_threads())
        compare({k: v[sub] for k, v in many.items()}, want)
        chain = [_drive(poses[k % 2], k) for k in range(3)]
        mc.lattice_set_closed_loop(True); ctx.lattice_set_closed_loop(True)
        try:
            for k, p in enumerate(chain):
                a, b = ctx.lattice_plan(p, cfg), mc.lattice_plan(p, cfg)
                _same(b, a, f"closed loop link {k}: MultiContext vs one context")
        finally:
            mc.lattice_set_closed_loop(False); ctx.lattice_set_closed_loop(False)
        open_loop = ctx.lattice_plan(chain[2], cfg)
        assert (open_loop["best_cost"] != a["best_cost"]).any()        # the similarity term is live in the chain
