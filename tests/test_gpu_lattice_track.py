"""Step 7 of a lattice plan on the device -- emit_and_track over wave_pursuit / wave_intersect / seg_hit / get_actuation -- at the edges of its verdict,
through every entry point that takes host goals.  The cases and the exact reference are tests/lattice_track_ref.py's (families a to f; the host test
ties the oracle to the reference on the same cases).

Forms: lattice_plan under lattice_set_mode 0 (the all-fp64 kernel), 1, 2 and 3 (the mixed schedule: k_lattice_select with the refinement's positions
handed over, and re-emitting; the cubic generator's closed form), lattice_plan_tracks on a one-track set, traj_dtype float32, lattice_plan_dev on
device buffers.  lattice_step / lattice_step_tracks take no goals (they sample from the raceline) and are not reached.

Per case: (1) the oracle's pure pursuit on the form's OWN fp64 rows gives the form's status and speed exactly and its steer within 1e-12, decided or
not; (2) where the exact reference decides on those rows: its status, and its steer within 1e-12 (0.0 exactly where it says 0.0); (3) every form
equals mode 0 bit for bit; (4) against the oracle's plan: indices equal, rows within 1e-9, status and target row equal where both row sets are
decided, the other disagreements counted and printed; (5) coverage read from the run.
"""
from collections import Counter

import numpy as np
import pytest

import lattice_track_ref as T
from f1tenth_planning_amd import _abi

pytestmark = pytest.mark.gpu
OUT = ("steer", "speed", "best_idx", "best_cost", "status", "near_idx", "best_traj")
# k_lattice_mixed.hip / lattice_mixed.h: ego e of an unpipelined plan appends its refinement entries, contiguous, to shard e % 8; the first
# ((ce + 7) / 8 + 1) * 4 entries of a shard (ce = E rounded up to 4, at most all ((ce + 7) / 8 + 1) * n_cand of them) have a position block, which
# k_lattice_select takes over (HAVE_INC); a winner further back is re-emitted
Q_SHARDS, INC_PER_EGO = 8, 4


@pytest.fixture(scope="module")
def ctx():
    from f1tenth_planning_amd.runtime import Context
    with Context(0) as c:
        yield c


def emitter_bounds(q, n_cand):
    """(egos whose winner surely came with positions, egos whose winner was surely re-emitted) from the entries per ego of one unpipelined
    mixed plan: whatever order the egos of a shard arrived in"""
    E = len(q)
    ce = max((E + 3) & ~3, 4)
    per = (ce + Q_SHARDS - 1) // Q_SHARDS + 1
    cap = min(per * INC_PER_EGO, per * n_cand)
    handed = emitted = 0
    for s in range(Q_SHARDS):
        qs = np.sort(q[s::Q_SHARDS][q[s::Q_SHARDS] > 0])
        if len(qs) == 0:
            continue
        handed += int((np.cumsum(qs[::-1]) <= cap).sum())                       # the first arrivals fit whole, even if they are the largest
        reach = 1 + int((np.cumsum(qs)[:-1] < cap).sum())                       # egos that can have an entry below the cap, if the smallest come first
        emitted += len(qs) - min(reach, len(qs))
    return handed, emitted


def plan_dev(c, p):
    E, S = len(p.idx), p.cases.S
    bufs = [c.to_device(p.poses), c.to_device(p.goals)] + [c.alloc(q * E) for q in (8, 8, 4, 8, 4, 4, 8 * S * 4)]
    try:
        c.lattice_plan_dev(bufs[0], E, p.cfg, *bufs[2:], d_goals=bufs[1])
        c.sync()
        kinds = ((np.float64, E), (np.float64, E), (np.int32, E), (np.float64, E), (np.int32, E), (np.int32, E), (np.float64, (E, S, 4)))
        return {k: b.download(*kd) for k, b, kd in zip(("steer", "speed", "best_idx", "best_cost", "status", "near_idx", "best_traj"), bufs[2:], kinds)}
    finally:
        for b in bufs:
            b.free()


class Run:
    def __init__(self, plan, base):
        self.plan, self.base, self.differ, self.queue = plan, base, [], {}


@pytest.fixture(scope="module")
def runs(ctx, orc):
    """every plan of both suites through every form, once: mode 0's outputs, what differs from them in any other form, the refinement queue's entries"""
    wp = T.raceline()
    ctx.set_waypoints(wp); ctx.set_grid(None, 0, (0, 0), 0); ctx.set_tracks([wp]); ctx.lattice_set_pipeline(1)
    out = {}
    try:
        for gen in ("clothoid", "cubic"):
            out[gen] = []
            for p in T.suite(orc, gen):
                E = len(p.idx)
                ctx.lattice_set_mode(0)
                r = Run(p, ctx.lattice_plan(p.poses, p.cfg, goals=p.goals))
                forms = {}
                for mode in (1, 2, 3):
                    ctx.lattice_set_mode(mode)
                    forms[f"mode {mode}"] = ctx.lattice_plan(p.poses, p.cfg, goals=p.goals)
                    r.queue[mode] = ctx.lattice_debug_queue(E)
                ctx.lattice_set_mode(1)
                forms["tracks"] = ctx.lattice_plan_tracks(p.poses, np.zeros(E, np.int32), p.cfg, goals=p.goals)
                forms["f32 rows"] = ctx.lattice_plan(p.poses, p.cfg, goals=p.goals, traj_dtype=np.float32)
                forms["dev"] = plan_dev(ctx, p)
                for name, g in forms.items():
                    for k in OUT:
                        want = r.base[k]
                        if name == "f32 rows" and k == "best_traj":
                            with np.errstate(over="ignore"):                     # (family e's rows beyond the f32 range round to inf, on the device too)
                                want = want.astype(np.float32)
                        eq = (g[k] == want) | ((g[k] != g[k]) & (want != want))
                        if g[k].dtype != want.dtype or not eq.all():
                            r.differ.append((name, k, np.nonzero(~eq.reshape(E, -1).all(1))[0][:8].tolist()))
                out[gen].append(r)
    finally:
        ctx.lattice_set_mode(1); ctx.lattice_set_pipeline(0); ctx.set_tracks([])
    return out


def cases_of(runs, gen, families):
    for r in runs[gen]:
        if r.plan.cases.family in families:
            for e in range(len(r.plan.idx)):
                yield r, e


@pytest.mark.parametrize("gen", ("clothoid", "cubic"))
def test_forms_agree_bit_for_bit_with_the_all_fp64_kernel(runs, gen):
    """(3) modes 1, 2, 3, the track-set plan, the f32-row plan and the device-buffer plan against mode 0: steer, speed, status, best_idx, best_cost,
    near_idx and the rows (the f32 rows: mode 0's rounded once)"""
    bad = [(r.plan.cases.family, r.plan.cases.S, r.plan.cases.L, r.plan.C, d) for r in runs[gen] for d in r.differ]
    assert not bad, bad[:10]


@pytest.mark.parametrize("gen,families", (("clothoid", "a"), ("clothoid", "bcd"), ("clothoid", "e"), ("cubic", "abcd")))
def test_tracker_on_the_emitted_rows(runs, orc, gen, families):
    """(1), (2) and family e's bar, on mode 0's rows (test (3) holds every other form to the same bits)"""
    wp = T.raceline()
    n = Counter()
    for r, e in cases_of(runs, gen, families):
        p, g = r.plan, r.base
        tag = (p.cases.tag[e], p.C)
        if p.cases.family == "e":                                                # no output non-finite where the oracle's is finite
            for k in ("steer", "speed", "best_cost"):
                assert np.isfinite(g[k][e]) or not np.isfinite(p.want[k][e]), (tag, k)
            assert np.isfinite(g["best_traj"][e]).all() or not np.isfinite(p.want["best_traj"][e]).all(), tag
        if g["status"][e] == _abi.ST_ALL_BLOCKED:
            assert g["steer"][e] == 0.0 and g["speed"][e] == 0.0 and not g["best_cost"][e] < np.inf, tag
            n["blocked"] += 1
            continue
        rows = g["best_traj"][e]
        v = wp[g["near_idx"][e], 2]
        pp = orc.pure_pursuit_batch(np.zeros((1, 3)), np.column_stack([rows[:, 0], rows[:, 1], np.full(len(rows), v)]), p.cases.L, p.cfg.wheelbase,
                                    p.cfg.max_reacquire)
        assert pp["status"][0] == g["status"][e] and pp["speed"][0] == g["speed"][e], (tag, pp, g["status"][e], g["speed"][e])
        assert abs(pp["steer"][0] - g["steer"][e]) <= 1e-12, (tag, pp["steer"][0], g["steer"][e])
        ref = T.reference_cached(rows[:, :2], p.cases.L, p.cfg.wheelbase, p.cfg.max_reacquire)
        if ref is None or not ref.decided or p.cases.family == "e":
            n["undecided"] += 1
            continue
        n["decided"] += 1
        n["closing"] += ref.la == -1
        n["seg64"] += ref.seg64
        assert g["status"][e] == ref.status, (tag, ref)
        if ref.status == T.ST_NO_LOOKAHEAD:
            assert g["steer"][e] == 0.0 and g["speed"][e] == 0.0, tag
        else:
            assert abs(g["steer"][e] - ref.steer[ref.la]) <= 1e-12 and g["speed"][e] == v, (tag, ref, g["steer"][e])
            if ref.steer[ref.la] == 0.0:
                assert g["steer"][e] == 0.0, (tag, g["steer"][e])
    print(gen, families, dict(n))
    if families != "e":
        assert n["decided"] >= 0.75 * (n["decided"] + n["undecided"])
    if "a" in families:
        assert n["closing"] >= 20                                                # (5) per form: the forms are bit-identical
    if gen == "clothoid" and families == "bcd":
        assert n["seg64"] >= 20


@pytest.mark.parametrize("gen", ("clothoid", "cubic"))
def test_against_the_oracles_plan(runs, gen):
    """(4) best_idx and near_idx equal, rows within 1e-9 (family e: of the row's magnitude); where the exact reference decides on BOTH row sets the
    status and the target row are equal and the steers differ by no more than the rows allow (2 wheelbase 1e-9 / L^2); elsewhere the two row sets may
    differ in the last ulps and fall on different sides: counted and printed"""
    n = Counter()
    for r in runs[gen]:
        p, g, w = r.plan, r.base, r.plan.want
        np.testing.assert_array_equal(g["best_idx"], w["best_idx"], err_msg=str((p.cases.family, p.cases.S, p.C)))
        np.testing.assert_array_equal(g["near_idx"], w["near_idx"])
        np.testing.assert_allclose(g["best_traj"], w["best_traj"], rtol=1e-9 if p.cases.family == "e" else 0, atol=1e-9)
        for e in range(len(p.idx)):
            same = g["status"][e] == w["status"][e] and abs(g["steer"][e] - w["steer"][e]) <= 1e-12 + 2.0 * p.cfg.wheelbase * 1e-9 / p.cases.L ** 2
            a = T.reference_cached(g["best_traj"][e, :, :2], p.cases.L, p.cfg.wheelbase, p.cfg.max_reacquire)
            b = T.reference_cached(w["best_traj"][e, :, :2], p.cases.L, p.cfg.wheelbase, p.cfg.max_reacquire)
            if p.cases.family != "e" and a is not None and b is not None and a.decided and b.decided:
                n["decided on both"] += 1
                assert same and (a.status, a.la) == (b.status, b.la), (p.cases.tag[e], p.C, a, b, g["steer"][e], w["steer"][e])
            else:
                n["undecided on one"] += 1
                n["disagreements"] += not same
            n["rows bit-identical"] += np.array_equal(g["best_traj"][e], w["best_traj"][e])
    print(gen, dict(n))
    assert n["decided on both"] > 1000


def test_both_emitters_of_the_mixed_schedule_are_reached(runs):
    """(5) read from the refinement queue of modes 1, 2 and 3: at least 10 clothoid winners that came with the refinement's station positions and at
    least 10 that k_lattice_select re-emitted (the near-twin decoys fill the queue past the position blocks)"""
    for mode in (1, 2, 3):
        handed = emitted = 0
        for r in runs["clothoid"]:
            if r.plan.cases.family != "e":
                h, m = emitter_bounds(r.queue[mode], r.plan.cfg.n_cand)
                handed += h; emitted += m
        print("mode", mode, "winners with positions handed over >=", handed, "re-emitted >=", emitted)
        assert handed >= 10 and emitted >= 10, (mode, handed, emitted)
