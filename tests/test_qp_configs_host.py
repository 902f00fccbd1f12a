"""The two QP yardsticks (tests/kmpc_qp_ref.py, tests/stmpc_qp_ref.py) OFF the defaults of mpc_config, on the host: their problem data
against the reference's own (golden G18, recorded from the reference's code by tools/gen_golden_qp_offdefault.py with a different
off-default config per case), and the seeded sweep of tests/qp_cases.py that tests/test_gpu_qp_configs.py runs on the GPU: it has teeth
(the exact optimum moves when Q and Qf, or R and Rd, change places) and the helper's exact solver settles on it.  No GPU."""
import numpy as np
import pytest

import kmpc_qp_ref as KQ
import qp_cases as QC
import stmpc_qp_ref as SQ


def g18_cases(golden):
    g = golden("g18_qp_offdefault.npz")

    def dense(p, m):
        A = np.zeros(tuple(g[p + m + "_shape"]))
        A[g[p + m + "_rows"], g[p + m + "_cols"]] = g[p + m + "_vals"]
        return A
    out = []
    for k in range(int(g["n_cases"])):
        p = f"c{k:02d}_"
        rec = {m: dense(p, m) for m in ("P", "Aeq", "G")}
        rec.update({v: g[p + v] for v in ("q", "beq", "h")})
        rec["r"] = float(g[p + "r"])
        cfg = {key[len(p) + 4:]: g[key] for key in g.files if key.startswith(p + "cfg_")}
        out.append(dict(branch=str(g[p + "branch"]), T=int(g[p + "T"]), seed=int(g[p + "seed"]), x0=g[p + "x0"], ref=g[p + "ref"],
                        oa=g[p + "oa"], od=g[p + "od"], cfg=cfg, rec=rec))
    return out


def _params(c):
    """the yardstick's parameters of a G18 case: from qp_cases' spec of the recorded seed, which must be the recorded config"""
    spec = (QC.kmpc_spec if c["branch"] == "kin" else QC.stmpc_spec)(c["seed"], c["T"])
    assert set(spec) == set(c["cfg"])
    for k, v in spec.items():
        assert np.array_equal(np.asarray(v, dtype=np.float64), c["cfg"][k]), (c["branch"], c["T"], c["seed"], k)
    return QC.kmpc_params(spec) if c["branch"] == "kin" else QC.stmpc_params(spec)


def test_g18_covers_the_cases(golden):
    cases = g18_cases(golden)
    kin = [c for c in cases if c["branch"] == "kin"]
    dyn = [c for c in cases if c["branch"] == "dyn"]
    assert sorted({c["T"] for c in kin}) == [2, 3, 9] and len(kin) >= 12
    assert sorted({c["T"] for c in dyn}) == [2, 5] and len(dyn) >= 8
    for c in kin:                                                    # every case off the defaults, each with a config of its own
        assert not np.array_equal(c["cfg"]["Qk"], c["cfg"]["Qfk"]) and not np.array_equal(c["cfg"]["Rk"], c["cfg"]["Rdk"])
    for c in dyn:
        assert not np.array_equal(c["cfg"]["Q"], c["cfg"]["Qf"]) and not np.array_equal(c["cfg"]["R"], c["cfg"]["Rd"])
        assert (c["cfg"]["Q"][[2, 5, 6]] > 0).all() and c["cfg"]["vp"][0] != SQ.PARAMS[0] and c["cfg"]["vp"][7] != SQ.PARAMS[7]
    assert len({tuple(c["cfg"]["Qk"]) for c in kin}) == len(kin) and len({tuple(c["cfg"]["Q"]) for c in dyn}) == len(dyn)
    assert any((c["cfg"]["Rdk"] == 0).all() for c in kin) and any((c["cfg"]["Qk"] == 0).any() for c in kin)
    assert {float(c["cfg"]["MIN_SPEED"]) for c in kin} >= {0.0, -1.0} and len({float(c["cfg"]["DTK"]) for c in kin}) == 3
    assert len({float(c["cfg"]["DT"]) for c in dyn}) >= 2
    assert any(c["oa"].any() for c in cases) and any(not c["oa"].any() for c in cases)


def test_helper_qp_data_equals_the_references_off_default(golden):
    """every matrix and vector the reference builds from an off-default mpc_config: Qfk at t = T only, Rdk on the differences, the
    bounds' rows and right-hand sides (MAX_DSTEER x DTK, -MIN_SPEED), DTK / WB and the vehicle parameters in the model"""
    for k, c in enumerate(g18_cases(golden)):
        p = _params(c)
        d = (KQ if c["branch"] == "kin" else SQ).qp_data(c["x0"], c["ref"], c["oa"], c["od"], p)
        for m in ("P", "Aeq", "G", "q", "beq", "h"):
            a, b = c["rec"][m], d[m]
            assert a.shape == b.shape, (k, m)
            assert np.abs(a - b).max() <= 1e-12 * (1.0 + np.abs(a).max()), (k, m, np.abs(a - b).max())
        assert abs(c["rec"]["r"] - d["r"]) <= 1e-12 * (1.0 + abs(d["r"])), k


def test_fast_condense_equals_condense_off_default(golden):
    """stmpc_qp_ref.fast_condense (the GPU sweeps' certificates are taken on it) against condense(qp_data(...)).  The two sum the same
    <= 7 T products per entry in different orders: rounding of ~T 7 eps relative to the largest entry, T <= 5 here -- 1e-12 of
    (1 + max |a|) leaves a factor of a hundred"""
    n = 0
    for k, c in enumerate(g18_cases(golden)):
        if c["branch"] != "dyn":
            continue
        p = _params(c)
        full = SQ.condense(SQ.qp_data(c["x0"], c["ref"], c["oa"], c["od"], p), c["T"])
        fast = SQ.fast_condense(c["x0"], c["ref"], c["oa"], c["od"], p)
        for m in ("H", "g", "G", "h"):
            assert np.abs(full[m] - fast[m]).max() <= 1e-12 * (1.0 + np.abs(full[m]).max()), (k, m, np.abs(full[m] - fast[m]).max())
        assert abs(full["c"] - fast["c"]) <= 1e-12 * (1.0 + abs(full["c"])), k
        n += 1
    assert n >= 8


# ---- the sweep of the GPU tests: teeth and the helper's exact-settle rate ---------------------------------------------------------------
def _swapped(p, a, b):
    q = dict(p)
    q[a], q[b] = p[b], p[a]
    return q


def _cond(kind, x0, ref, oa, od, p):
    if kind == "kmpc":
        return KQ.condense(KQ.qp_data(x0, ref, oa, od, p), p["T"])
    return SQ.fast_condense(x0, ref, oa, od, p)


def _exact(c, polish_only):
    """the helper's exact optimum from its own guess, or None when it does not certify.  From T = 20 on the active-set polish from the
    numpy interior point's guess only (the SLSQP fallback costs seconds to tens of seconds per case there)."""
    if np.linalg.eigvalsh(c["H"]).min() <= 0:
        return None
    if polish_only:
        r = SQ.polish(c, SQ.ipm_hint(c))
        return None if r is None else r[0]
    u, lam, _ = SQ.exact(c)
    return u if SQ.exact_ok(c, u, lam) else None


SWEEP = [("kmpc", T) for T in QC.KMPC_HORIZONS] + [("stmpc", T) for T in QC.STMPC_HORIZONS]


@pytest.mark.parametrize("kind,T", SWEEP)
def test_sweep_has_teeth_and_the_helper_settles(kind, T):
    """On the first ego of every case of the GPU sweep: (a) the exact optimum of the case moves by more than 100 x the GPU tests' bar
    (1e-7) when Q and Qf change places, and when R and Rd do, in at least half of the cases -- a kernel that swaps them cannot pass
    test_gpu_qp_configs; (b) the helper's exact solver certifies its optimum in all but a quarter of the cases at most (the GPU tests
    compare u only where it does).  T = 44 of the dynamic QP is held to the certificate alone there, and is not counted here."""
    km = kind == "kmpc"
    long = T >= (QC.KMPC_LONG if km else QC.STMPC_LONG)
    seeds = QC.LONG_SEEDS if long else (QC.KMPC_SEEDS if km else QC.STMPC_SEEDS)
    ref_fn = QC.host_ref_fn(4 if km else 7)
    names = (("Qk", "Qfk"), ("Rk", "Rdk")) if km else (("Q", "Qf"), ("R", "Rd"))
    moved = {names[0]: 0, names[1]: 0}
    unsettled = 0
    for seed in seeds:
        p = (QC.kmpc_case if km else QC.stmpc_case)(seed, T)[1]
        x0, ref, oa, od = (a[0] for a in (QC.kmpc_inputs if km else QC.stmpc_inputs)(seed, p, QC.n_egos(seed), ref_fn))
        u = _exact(_cond(kind, x0, ref, oa, od, p), T >= 20)
        if u is None:
            unsettled += 1
            continue
        for pair in names:
            us = _exact(_cond(kind, x0, ref, oa, od, _swapped(p, *pair)), T >= 20)
            moved[pair] += us is not None and np.abs(us - u).max() > 100 * 1e-7
    print(kind, T, "cases", len(seeds), "unsettled", unsettled, "moved", moved)
    for pair, n in moved.items():
        assert 2 * n >= len(seeds), (pair, n, len(seeds))
    if not (kind == "stmpc" and T == 44):
        assert 4 * unsettled <= len(seeds), (unsettled, len(seeds))


def test_lds_edges_and_horizon_lists():
    """the horizons on either side of 8 * lds_doubles(T) == sharedMemPerBlock (64 KiB on gfx950), from the kernels' own formulas"""
    assert QC.KMPC_LDS_EDGE == [24, 25] and QC.STMPC_LDS_EDGE == [28, 29]
    assert 8 * QC.kmpc_lds_doubles(24) <= 65536 < 8 * QC.kmpc_lds_doubles(25)
    assert 8 * QC.stmpc_lds_doubles(28) <= 65536 < 8 * QC.stmpc_lds_doubles(29)
    assert set(QC.KMPC_HORIZONS) >= {2, 3, 7, 8, 9, 16, 31, 32} and set(QC.STMPC_HORIZONS) >= {2, 3, 10, 43, 44}
    assert len(QC.KMPC_SEEDS) == 24 and len(QC.STMPC_SEEDS) == 16
