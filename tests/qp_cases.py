"""Seeded off-default cases for the two QP kernels (tests/test_qp_configs_host.py, tests/test_gpu_qp_configs.py, tools/gen_golden_qp_offdefault.py).
A helper module, not a conftest.

One spec -- a dict of plain numbers keyed by the mpc_config field names -- makes BOTH sides of every comparison: the device config
(_abi.kmpc_cfg / _abi.stmpc_cfg) and the yardstick's parameter dict (kmpc_qp_ref / stmpc_qp_ref), so the two cannot drift apart.

  * kmpc_spec / stmpc_spec (seed, T):   the spec, drawn from ranges the yardsticks were tried on
  * kmpc_case / stmpc_case (seed, T):   (cfg, params) of that spec
  * kmpc_inputs / stmpc_inputs:         states, references, previous solutions for E egos of a case; the reference comes from `ref_fn`
                                        (ctx.kmpc_ref / ctx.stmpc_ref on the GPU, host_ref_fn() without one)
  * the horizons and seeds of the sweeps, shared by the host and the GPU tests
"""
import numpy as np

import kmpc_qp_ref as Q
import stmpc_qp_ref as SQ

LDS_PER_BLOCK = 65536                       # sharedMemPerBlock of gfx950: above it a launch opts in to large LDS (qp_lds_opt_in)
DL = 0.03


def kmpc_lds_doubles(T):
    """qp_lds_doubles of k_kmpc_qp.hip"""
    n, Tp = 2 * T, T + 1
    return 4 * Tp * n + n * n + 3 * n + T + 4 + 8 * Tp + 6 * T


def stmpc_lds_doubles(T):
    """stqp_lds_doubles of k_stmpc_qp.hip (NJ = 20 Jacobian entries per step)"""
    n, Tp = 2 * T, T + 1
    return 2 * n * n + 8 + 14 * Tp + 20 * T + 7 * n + 3 * n + 8 * T


def _straddle(doubles):
    T = 2
    while 8 * doubles(T + 1) <= LDS_PER_BLOCK:
        T += 1
    return [T, T + 1]                       # the last horizon inside sharedMemPerBlock and the first above it


KMPC_LDS_EDGE = _straddle(kmpc_lds_doubles)      # [24, 25]: 8 * (12 T^2 + 29 T + 12) crosses 65536 between them
STMPC_LDS_EDGE = _straddle(stmpc_lds_doubles)    # [28, 29]: 8 * (8 T^2 + 62 T + 22)
KMPC_HORIZONS = sorted({2, 3, 7, 8, 9, 16, 31, 32, *KMPC_LDS_EDGE})
STMPC_HORIZONS = sorted({2, 3, 10, 43, 44, *STMPC_LDS_EDGE})
KMPC_SEEDS = list(range(24))
STMPC_SEEDS = list(range(16))
KMPC_LONG, STMPC_LONG = 31, 20               # from these horizons on the host-side exact solves run on LONG_SEEDS only
LONG_SEEDS = [0, 1, 2, 3]


# Configs replaced after the first run on the GPU.  In each of them some ego's Newton matrix stops being numerically
# positive definite, or the iteration runs into max_iter, before the stopping rule holds -- in the kernel and, iteration for iteration,
# in the same Mehrotra method in numpy (stmpc_qp_ref.ipm_hint's algorithm with the kernel's stopping rule): the problem, not the kernel.
#   * kinematic: 4 of 240 configs -- (T, seed) below; the replacement is the next draw of the same stream.  (24, 13) and (32, 22):
#     one ego each with status 2; (31, 8): one ego accepted through the broken-down-factorisation rule with a complementarity of
#     1.3e-9; (32, 8): one ego (H over 7 decades, |g| ~ 2e5) meets the stopping rule 1.3e-7 from the exact optimum -- numpy: 1.1e-7,
#     and 2.2e-7 from the device's point -- and the next Newton matrix cannot be factored, so no refinement step exists.
#   * dynamic, T >= 28: all 26 of 64 configs with DT = 0.05 (22 of them ended with status 2 for 1 to 32 of their egos, the other four
#     needed up to 50 iterations).  The reference's explicit Euler step of the slip-angle row has the factor 1 - DT A5 ~ 1 - 52 DT,
#     which is below -1 at DT = 0.05: the prediction matrices grow like 1.6^T and H spans 12 decades and more.  Their DT is drawn
#     again from {0.0125, 0.025}; at T <= 10 DT = 0.05 stays.
KMPC_REPLACED = {(24, 13), (32, 22), (31, 8), (32, 8)}
STMPC_DT_LIMIT_T = 28


def _loguniform(rng, lo, hi, size=None):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), size))


# ---- kinematic ---------------------------------------------------------------------------------------------------------------------------
def kmpc_spec(seed, T):
    rng = np.random.default_rng([int(seed), int(T), 16] + ([1] if (T, seed) in KMPC_REPLACED else []))
    s = dict(TK=int(T), DTK=float(rng.choice([0.05, 0.1, 0.2])), WB=float(rng.uniform(0.25, 0.4)), MAX_STEER=float(rng.uniform(0.2, 0.6)),
             MAX_DSTEER=float(rng.uniform(0.5, 4.0)), MAX_ACCEL=float(rng.uniform(1.0, 5.0)), MAX_SPEED=float(rng.uniform(3.0, 8.0)),
             MIN_SPEED=float(rng.choice([0.0, -1.0, 0.5])))
    qk, qfk = rng.uniform(0.5, 30.0, 4), rng.uniform(0.5, 60.0, 4)
    rk = np.array([_loguniform(rng, 0.005, 1.0), _loguniform(rng, 1.0, 150.0)])
    rdk = np.array([_loguniform(rng, 0.005, 1.0), _loguniform(rng, 1.0, 150.0)])
    iz, izf = int(rng.integers(0, 4)), int(rng.integers(0, 4))
    if seed % 4 == 3:                          # one case in four: a zero entry in each state weight
        qk[iz] = 0.0
        qfk[izf] = 0.0
    if seed % 8 == 5:                          # legal: rd >= 0
        rdk[:] = 0.0
    s.update(Qk=[float(x) for x in qk], Qfk=[float(x) for x in qfk], Rk=[float(x) for x in rk], Rdk=[float(x) for x in rdk])
    return s


def kmpc_params(s):
    """the yardstick's p (kmpc_qp_ref.default_params' keys)"""
    return dict(T=s["TK"], DTK=s["DTK"], WB=s["WB"], MAX_STEER=s["MAX_STEER"], MAX_DSTEER=s["MAX_DSTEER"], MAX_SPEED=s["MAX_SPEED"],
                MIN_SPEED=s["MIN_SPEED"], MAX_ACCEL=s["MAX_ACCEL"], Rk=np.diag(s["Rk"]), Rdk=np.diag(s["Rdk"]), Qk=np.diag(s["Qk"]),
                Qfk=np.diag(s["Qfk"]))


def kmpc_cfg(s):
    from f1tenth_planning_amd import _abi
    return _abi.kmpc_cfg(horizon=s["TK"], dt=s["DTK"], wheelbase=s["WB"], max_steer=s["MAX_STEER"], max_dsteer=s["MAX_DSTEER"],
                         max_speed=s["MAX_SPEED"], min_speed=s["MIN_SPEED"], max_accel=s["MAX_ACCEL"], q=s["Qk"], qf=s["Qfk"], r=s["Rk"],
                         rd=s["Rdk"])


def kmpc_case(seed, T):
    s = kmpc_spec(seed, T)
    return kmpc_cfg(s), kmpc_params(s)


def kmpc_config_fields(s):
    """the spec as mpc_config fields (the weights as the diagonal matrices mpc_config holds)"""
    f = {k: v for k, v in s.items() if k not in ("Qk", "Qfk", "Rk", "Rdk")}
    f.update({k: np.diag(s[k]) for k in ("Qk", "Qfk", "Rk", "Rdk")})
    return f


# ---- dynamic -----------------------------------------------------------------------------------------------------------------------------
def stmpc_spec(seed, T):
    rng = np.random.default_rng([int(seed), int(T), 17])
    s = dict(T=int(T), DT=float(rng.choice([0.0125, 0.025, 0.05])), WB=0.33, MAX_STEER=float(rng.uniform(0.3, 0.6)),
             MAX_STEER_V=float(rng.uniform(1.0, 4.0)), MAX_ACCEL=float(rng.uniform(1.0, 5.0)), MAX_SPEED=float(rng.uniform(5.0, 8.0)),
             MIN_SPEED=float(rng.choice([0.0, 0.5])))
    if T >= STMPC_DT_LIMIT_T and s["DT"] == 0.05:
        s["DT"] = float(np.random.default_rng([int(seed), int(T), 20]).choice([0.0125, 0.025]))
    s["Q"] = [float(x) for x in rng.uniform(0.1, 40.0, 7)]
    s["Qf"] = [float(x) for x in rng.uniform(0.1, 60.0, 7)]
    s["R"] = [float(_loguniform(rng, 0.05, 2.0)), float(_loguniform(rng, 0.002, 0.5))]          # [steering speed, accel]
    s["Rd"] = [float(_loguniform(rng, 0.05, 2.0)), float(_loguniform(rng, 0.002, 0.5))]
    vp = SQ.PARAMS.copy()
    vp[0] *= rng.uniform(0.9, 1.1)             # mass
    vp[7] *= rng.uniform(0.9, 1.1)             # friction
    s["vp"] = [float(x) for x in vp]
    return s


def stmpc_params(s):
    return dict(T=s["T"], DT=s["DT"], WB=s["WB"], MAX_STEER=s["MAX_STEER"], MAX_STEER_V=s["MAX_STEER_V"], MAX_SPEED=s["MAX_SPEED"],
                MIN_SPEED=s["MIN_SPEED"], MAX_ACCEL=s["MAX_ACCEL"], R=np.diag(s["R"]), Rd=np.diag(s["Rd"]), Q=np.diag(s["Q"]),
                Qf=np.diag(s["Qf"]), vp=np.array(s["vp"]))


def stmpc_cfg(s):
    from f1tenth_planning_amd import _abi
    return _abi.stmpc_cfg(horizon=s["T"], dt=s["DT"], wheelbase=s["WB"], max_steer=s["MAX_STEER"], max_steer_v=s["MAX_STEER_V"],
                          max_speed=s["MAX_SPEED"], min_speed=s["MIN_SPEED"], max_accel=s["MAX_ACCEL"], q=s["Q"], qf=s["Qf"], r=s["R"],
                          rd=s["Rd"], params=s["vp"])


def stmpc_case(seed, T):
    s = stmpc_spec(seed, T)
    return stmpc_cfg(s), stmpc_params(s)


def stmpc_config_fields(s):
    f = {k: v for k, v in s.items() if k not in ("Q", "Qf", "R", "Rd", "vp")}
    f.update({k: np.diag(s[k]) for k in ("Q", "Qf", "R", "Rd")})
    return f


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
_TRACK = {}


def track():
    """the synthetic centreline of the sweeps as waypoint rows [x, y, v, yaw, kappa] (Context.set_waypoints' default columns)"""
    if "rl" not in _TRACK:
        from f1tenth_planning_amd import synth
        cl = synth.make_centerline(seed=3)
        _TRACK["rl"] = np.ascontiguousarray(cl[:, [1, 2, 5, 3, 4]])
    return _TRACK["rl"]


def host_ref_fn(ncol):
    """references without a GPU: calc_ref_trajectory's gathers (kmpc_qp_ref.ref_trajectory) on track(); ncol 4 -> [E, 4, T+1] rows
    (x, y, v, yaw), ncol 7 -> [E, 7, T+1] rows (x, y, 0, v, yaw, 0, 0)"""
    rl = track()
    cx, cy, sp, cyaw = (np.ascontiguousarray(rl[:, k]) for k in range(4))

    def fn(x4, T, dt):
        out = np.zeros((len(x4), ncol, T + 1))
        for e, s in enumerate(x4):
            r = Q.ref_trajectory(s, cx, cy, cyaw.copy(), sp, dict(T=T, DTK=dt), dlk=DL)
            if ncol == 4:
                out[e] = r
            else:
                out[e, [0, 1, 3, 4]] = r
        return out
    return fn


def kmpc_inputs(seed, p, E, ref_fn):
    """E egos of one case, drawn like test_gpu_kmpc_qp._scale_inputs with the case's own bounds: speeds over [MIN_SPEED, MAX_SPEED] (a
    twentieth at each bound), heading errors up to +-1.2 rad, reference speeds scaled 0..2.8x, a non-zero previous solution for half the
    egos; a fifth slow, facing backwards, with a near-zero reference speed (the lower speed bound); a quarter of the rest fast, 2 m
    beside the line and heading back across it (the rate bound).  ref_fn(x0 [E, 4], T, dt) -> [E, 4, T+1]."""
    T, lo, hi = p["T"], p["MIN_SPEED"], p["MAX_SPEED"]
    rng = np.random.default_rng([int(seed), T, 18])
    rl = track()
    k = rng.integers(0, len(rl) - 1, E)
    v = rng.uniform(lo, hi, E)
    v[rng.random(E) < 0.05] = hi
    v[rng.random(E) < 0.05] = lo
    yaw = rl[k, 3] + rng.normal(0, 0.5, E).clip(-1.2, 1.2)
    rev = rng.random(E) < 0.2
    yaw[rev] += np.pi
    v[rev] = rng.uniform(lo, lo + 0.6, int(rev.sum()))
    lat = np.where(~rev & (rng.random(E) < 0.25), rng.choice([-2.0, 2.0], E), 0.0)
    yaw -= 1.2 * lat
    v[lat != 0] = rng.uniform(0.5 * hi, hi, int((lat != 0).sum()))
    nx, ny = -np.sin(rl[k, 3]), np.cos(rl[k, 3])
    x0 = np.column_stack([rl[k, 0] + lat * nx + rng.normal(0, 0.3, E), rl[k, 1] + lat * ny + rng.normal(0, 0.3, E), v, yaw])
    ref = np.array(ref_fn(x0, T, p["DTK"]), dtype=np.float64)
    ref[:, 2, :] *= np.where(rev, rng.uniform(0.0, 0.3, E), rng.uniform(0.0, 2.8, E))[:, None]
    warm = rng.random(E) < 0.5
    oa = np.where(warm[:, None], rng.normal(0, 0.5 * p["MAX_ACCEL"], (E, T)).clip(-p["MAX_ACCEL"], p["MAX_ACCEL"]), 0.0)
    od = np.where(warm[:, None], rng.normal(0, 0.6 * p["MAX_STEER"], (E, T)).clip(-p["MAX_STEER"], p["MAX_STEER"]), 0.0)
    return x0, ref, oa, od


def stmpc_inputs(seed, p, E, ref_fn):
    """E dynamic-branch egos of one case, drawn like test_gpu_stmpc_qp._scale_inputs with the case's own bounds: speeds 2.05..MAX_SPEED
    (a tenth at MAX_SPEED), steering inside 0.83 MAX_STEER (a twentieth exactly at a bound), heading errors up to +-0.9 rad, yaw rates
    and slip angles, reference speeds scaled 0.3..1.6x, a random previous solution for half the egos (accelerating on average, so the
    prediction keeps away from v = 0).  ref_fn(x0 [E, 4] = (x, y, v, yaw), T, dt) -> [E, 7, T+1]."""
    T, hi = p["T"], p["MAX_SPEED"]
    rng = np.random.default_rng([int(seed), T, 19])
    rl = track()
    k = rng.integers(0, len(rl) - 1, E)
    v = rng.uniform(2.05, hi, E)
    v[rng.random(E) < 0.1] = hi
    d = rng.uniform(-0.83, 0.83, E) * p["MAX_STEER"]
    at = rng.random(E) < 0.05
    d[at] = p["MAX_STEER"] * rng.choice([-1.0, 1.0])
    yaw = rl[k, 3] + rng.normal(0, 0.3, E).clip(-0.9, 0.9)
    x0 = np.column_stack([rl[k, 0] + rng.normal(0, 0.3, E), rl[k, 1] + rng.normal(0, 0.3, E), d, v, yaw, rng.normal(0, 0.5, E),
                          rng.normal(0, 0.03, E)])
    ref = np.array(ref_fn(x0[:, [0, 1, 3, 4]], T, p["DT"]), dtype=np.float64)
    ref[:, 3, :] *= rng.uniform(0.3, 1.6, E)[:, None]
    warm = rng.random(E) < 0.5
    A, SV = p["MAX_ACCEL"], p["MAX_STEER_V"]
    oa = np.where(warm[:, None], rng.normal(0.1 * A, 0.33 * A, (E, T)).clip(-0.66 * A, A), 0.0)
    odv = np.where(warm[:, None], rng.normal(0, 0.3 * SV, (E, T)).clip(-SV, SV), 0.0)
    return x0, ref, oa, odv


def n_egos(seed):
    """egos per case, 8 to 32: with sizes that leave the last workgroup of the four-ego packing partly filled"""
    return (8, 13, 32, 9)[seed % 4]
