"""The high-precision reference of the G1 clothoid fit (tests/clothoid_fit_ref.py), its fixture (tests/golden/g21_clothoid_fit.npz) and the
CPU restatements of the fit against it.  CPU only; needs mpmath."""
import os

import numpy as np
import pytest

mp = pytest.importorskip("mpmath")

import clothoid_fit_ref as F  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FAM = {n: i for i, n in enumerate(F.FAMILIES)}


@pytest.fixture(scope="module")
def fx():
    return F.load_fixture(GOLDEN)


def test_continuation_selects_the_min_abs_a_root_of_the_independent_solver(golden):
    """two criteria for the principal branch that share nothing: tools/gen_clothoid_g14.py scans ALL roots of g on [-60, 60] and takes the
    admissible one of smallest |A|; clothoid_fit_ref continues A = 0 from (0, 0).  On every 20th unambiguous G14 goal (behind the ego,
    |theta| up to pi, the seams) they are the same root to 1e-14 max(1, |A|), and L to 1e-14 relative"""
    g = golden("g14_clothoid_g1.npz")
    sel = np.nonzero((g["ok"] == 1) & (g["ambiguous"] == 0))[0][::20]
    assert len(sel) >= 80
    worst = 0.0
    for i in sel:
        s = F.solve(*g["goals"][i])
        assert s["expect_ok"] == 1 and s["ambiguous"] == 0
        worst = max(worst, abs(s["A"] - g["A"][i]) / max(1.0, abs(s["A"])), abs(s["L"] / g["L"][i] - 1.0))
    print(f"largest difference to the G14 fixture over {len(sel)} goals: {worst:.1e}")
    assert worst <= 1e-14
    for i in np.nonzero(g["ok"] == 0)[0]:
        assert F.solve(*g["goals"][i])["expect_ok"] == 0


def test_the_root_is_a_root_by_quadrature(fx):
    """g, h and g' of the closed form (Fresnel integrals, two integrations by parts; the central difference below |A| = 0.01; the series
    below 1e-6) against mpmath.quad of the defining integrals at the continued root: |g| < 1e-40, h and g' equal to 1e-40"""
    picks = [i for f in ("square", "worst-guess", "rule-switch", "heading", "class") for i in np.nonzero((fx["family"] == FAM[f]) & fx["expect_ok"] & (fx["mirror_of"] < 0))[0][::60]]
    picks += list(np.nonzero((fx["family"] == FAM["near-straight"]) & (fx["mirror_of"] < 0))[0])
    small = 0
    for i in picks:
        p0, p1 = (float(v) for v in fx["phi"][i])
        A = F.principal_root(p0, p1)
        assert float(A) == fx["A"][i]
        with mp.workdps(F.DPS):
            d = mp.mpf(p1) - mp.mpf(p0)
            g, h, dg = F.gh(A, p0, d)
            gq, hq, dq = F.gh_quad(A, p0, d)
            scale = min(mp.mpf(1), max(abs(mp.mpf(p0)), abs(mp.mpf(p1)), mp.mpf(10) ** -320))
            small += abs(A) < 0.01
            assert abs(gq) < mp.mpf(10) ** -40 * scale and abs(g) < mp.mpf(10) ** -45 * scale, fx["goals"][i]
            exact = abs(A) >= 0.01 or max(abs(A), abs(p0), abs(d)) < F.SMALL        # (else the central difference: step 1e-18 on 50 digits)
            assert abs(h - hq) < mp.mpf(10) ** -40 and abs(dg - dq) < mp.mpf(10) ** (-40 if exact else -27), fx["goals"][i]
            assert float(abs(dg)) == fx["dg"][i]
    assert len(picks) >= 25 and small >= 5


def test_fixture_equals_a_fresh_evaluation(fx):
    """every 45th original goal solved afresh gives the committed doubles bit for bit; every mirror holds its original's numbers negated;
    the normalisation is the literal one (phi from the stored goal)"""
    orig = np.nonzero(fx["mirror_of"] < 0)[0]
    for i in list(orig[::45]) + list(np.nonzero((fx["family"] >= FAM["small-r"]) & (fx["mirror_of"] < 0))[0][::9]):
        s = F.solve(*fx["goals"][i])
        for k in ("A", "k0", "dk", "L", "dg", "guess_err", "exc"):
            assert s[k] == fx[k][i], (k, fx["goals"][i])
        assert (s["phi0"], s["phi1"]) == tuple(fx["phi"][i]) and s["rule"] == fx["rule"][i]
        assert bool(s["expect_ok"]) == fx["expect_ok"][i] and bool(s["ambiguous"]) == fx["ambiguous"][i] and bool(s["singular"]) == fx["singular"][i]
    m = np.nonzero(fx["mirror_of"] >= 0)[0]
    o = fx["mirror_of"][m]
    np.testing.assert_array_equal(fx["goals"][m], fx["goals"][o] * [1.0, -1.0, -1.0])
    for k in ("A", "k0", "dk"):
        np.testing.assert_array_equal(fx[k][m], -fx[k][o])
    for k in ("L", "dg", "guess_err", "exc", "rule", "expect_ok", "family", "ambiguous", "singular"):
        np.testing.assert_array_equal(fx[k][m], fx[k][o])
    assert len(m) == len(orig) and (o == m - 1).all()


def test_the_fixture_reaches_what_it_was_built_for(fx):
    """the families and what each is there for: the grid with its edges and the corner, the worst guesses, 1e-6 either side of every rule
    threshold, 40 goals or more per rule, r from 1.1e-12 to 1e150 (a subnormal kappa' among them), rejected r down to 1e-300, headings up to
    1e300, the signed zeros, and the trust radius"""
    ok, fam, g = fx["expect_ok"], fx["family"], fx["goals"]
    assert (fam == FAM["square"]).sum() == 33 * 33 + 1
    edge = np.abs(np.abs(fx["phi"]) - F.PI_D) == 0.0
    assert (edge[fam == FAM["square"], 0]).sum() >= 60 and (edge[fam == FAM["square"], 1]).sum() >= 4 and fx["ambiguous"][fam == FAM["square"]].sum() >= 2
    assert fx["singular"][fam == FAM["square"]].sum() >= 2 and not (fx["singular"] & fx["ambiguous"]).any()
    assert fx["guess_err"][ok].max() < 0.05 and fx["guess_err"][fam == FAM["worst-guess"]].min() > 0.0371
    rs = fam == FAM["rule-switch"]
    for thr in F.RULE_EDGES:
        d = fx["exc"][rs] - thr
        assert ((d > 0) & (d < 1e-6)).sum() >= 40 and ((d < 0) & (d > -1e-6)).sum() >= 40
    assert (np.bincount(fx["rule"][ok], minlength=5) >= 40).all() and fx["exc"][ok].max() <= 36.0
    r = np.hypot(g[:, 0], g[:, 1])
    assert r[ok].min() < 1.2e-12 and r[ok].max() >= 1e150 and not ok[fam == FAM["small-r"]].any() and not ok[fam == FAM["reject"]].any()
    assert ((np.abs(fx["dk"]) < 2.0 ** -1022) & (fx["dk"] != 0.0) & ok).any()
    assert np.abs(g[fam == FAM["heading"], 2]).max() >= 1e300
    assert ((g[:, 0] < 0) & (g[:, 1] == 0.0) & np.signbit(g[:, 1])).any() and ((g[:, 0] < 0) & (g[:, 1] == 0.0) & ~np.signbit(g[:, 1])).any()
    assert fx["dg"][ok].min() > 0.05                                 # well conditioned everywhere: the backward bar is a bar on A


def _report(name, k0, dk, L, fx, sel):
    fwd, bwd, idx = F.fit_errors(k0, dk, L, fx, sel)
    print(f"{name}: k0 L {fwd[:, 0].max():.1e}, dk L^2 {fwd[:, 1].max():.1e}, L / L* {fwd[:, 2].max():.1e}, A {fwd[:, 3].max():.1e}, backward {bwd.max():.1e} "
          f"over {len(idx)} goals")
    return fwd, idx


def test_cpu_restatements_of_the_fit_at_1e_11(fx, orc):
    """orc_clothoid_g1, numpy_lattice.clothoid_g1_batch and opcount.clothoid_g1 (every 16th goal: it counts its operations in Python) on the
    fixture: the same ok set, and the forward figures within 1e-11 -- their Newton iteration stops at |g| <= 1e-13, the smallest |g'| is 0.05,
    kappa' L^2 = 2 A doubles it: 4e-12"""
    from oracle import numpy_lattice as nl
    from oracle import opcount
    G = fx["goals"]
    sel = fx["expect_ok"] & ~fx["ambiguous"] & ~fx["singular"]
    pinned = ~fx["singular"]                                         # (the full-circle corners: ok and L hang on the last bit)
    res = np.array([orc.clothoid_g1(*g) for g in G], dtype=np.float64)
    np.testing.assert_array_equal(res[pinned, 0] != 0, fx["expect_ok"][pinned])
    fwd, idx = _report("orc_clothoid_g1", res[:, 1], res[:, 2], res[:, 3], fx, sel)
    assert fwd.max() <= F.ORACLE_BAR, G[idx[np.argmax(fwd.max(axis=1))]]
    ok, k0, dk, L = nl.clothoid_g1_batch(G[:, 0].copy(), G[:, 1].copy(), G[:, 2].copy())
    np.testing.assert_array_equal(ok[pinned], fx["expect_ok"][pinned])
    fwd, idx = _report("numpy_lattice", k0, dk, L, fx, sel)
    assert fwd.max() <= F.ORACLE_BAR, G[idx[np.argmax(fwd.max(axis=1))]]
    sub = np.zeros(len(G), bool)
    sub[::16] = True
    res = np.zeros((len(G), 4))
    for i in np.nonzero(sub)[0]:
        res[i] = [float(v) for v in opcount.clothoid_g1(*(opcount.F(v) for v in G[i]))]
    np.testing.assert_array_equal(res[sub & pinned, 0] != 0, fx["expect_ok"][sub & pinned])
    fwd, idx = _report("opcount", res[:, 1], res[:, 2], res[:, 3], fx, sel & sub)
    assert fwd.max() <= F.ORACLE_BAR, G[idx[np.argmax(fwd.max(axis=1))]]
