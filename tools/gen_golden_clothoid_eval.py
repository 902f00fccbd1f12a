#!/usr/bin/env python3
"""tests/clothoid_ref.py evaluated into tests/golden/g19_clothoid_eval.npz: parameters as exact doubles, reference rows
rounded once to double, labels.  Of a clothoid's rows the file keeps (x, y); theta and |kappa| are clothoid_ref.theta_kappa's exact rationals.  Needs mpmath; the tests that read the file need numpy only.

  t_*   the regime table: clothoids aimed at the evaluator's switches -- pieces per station interval (nsub) 1, 2..15, 16, above 16; the
        16-piece re-anchoring inside a station interval and on a station; station counts 1 .. 1000; zero, tiny and subnormal kappa',
        an inflection, multi-turn spirals, L from 1e-3 to 20 -- each with its mirror image (-k0, -dk), whose rows are the original's
        with y negated and are not stored
  g_*   every 8th solvable, unambiguous goal of g14_clothoid_g1.npz (g_idx: its rows there) with that fixture's own (k0, dk, L): clothoid
        rows at S = 2, 3, 50
  c_*   the same goals' cubic rows at S = 2, 3, 50 with the conditioning terms of |kappa| (sp, cond; float32: they only size a tolerance)
"""
import os
import sys

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import clothoid_ref as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g19_clothoid_eval.npz")
G14 = os.path.join(ROOT, "tests", "golden", "g14_clothoid_g1.npz")
NSUB = (1, 2, 3, 5, 7, 15, 16, 17, 31, 54, 251, 300, 1667)
G_S = (2, 3, 50)
RULE_CURV, RULE_DK = 0, 1


def regime_cases():
    """(label, k0, dk, L, S, nsub wanted or 0, rule wanted or -1).  The curvature rule n1 = kmax ds / 0.3 decides every nsub above 3:
    kmax >= |dk| L / 2, so n2 = 2.5 ds sqrt|dk| > n1 needs |dk| < 2.25 / L^2 and then n2 < 3.75 / (S - 1).  So nsub 2 and 3 are
    reached once through each rule, and every nsub once with the curvature in k0 (kappa' small) and once with it in kappa' L."""
    shapes_k0 = {1: (200, 5.5), 2: (65, 2.0), 3: (64, 20.0), 5: (17, 1.0), 7: (65, 0.5), 15: (17, 3.0), 16: (3, 1e-3), 17: (17, 2.0),
                 31: (3, 4.0), 54: (5, 2.0), 251: (17, 2.0), 300: (2, 3.0), 1667: (2, 10.0)}
    shapes_dk = {1: (64, 3.0), 2: (64, 8.0), 3: (17, 0.7), 5: (65, 6.0), 7: (3, 0.05), 15: (64, 12.0), 16: (65, 4.0), 17: (2, 1.5),
                 31: (17, 5.0), 54: (3, 1.0), 251: (2, 2.0), 300: (5, 0.3), 1667: (3, 7.0)}
    out = []
    for j, n in enumerate(NSUB):
        S, L = shapes_k0[n]
        ds = L / max(S - 1, 1)
        sg = 1.0 if j % 2 == 0 else -1.0
        kmax = (n - 0.5) * 0.3 / ds
        out.append((f"nsub{n}/k0", sg * kmax, -sg * 0.05 * 0.3 / (ds * L), L, S, n, RULE_CURV))      # kappa' pulls |kappa| DOWN along the curve: kmax = |k0|
        S, L = shapes_dk[n]
        ds = L / max(S - 1, 1)
        kmax = (n - 0.5) * 0.3 / ds
        k0 = -sg * 0.1 * kmax                                                                        # starts the other way: an inflection at 1/11 of L
        out.append((f"nsub{n}/dkL", k0, (-sg * kmax - k0) / L, L, S, n, RULE_CURV))
    for n, q in ((2, 0.6), (3, 1.0)):      # S = 2, k0 = -0.45 dk L, q = L sqrt|dk|: n2 = ceil(2.5 q) above n1 = ceil(0.55 q^2 / 0.3)
        for L, sg in ((1.7, 1.0), (0.01, -1.0)):
            dk = sg * (q / L) ** 2
            out.append((f"nsub{n}/dk-rule", -0.45 * dk * L, dk, L, 2, n, RULE_DK))
    out += [
        ("k0=0", 0.0, 1.3, 2.5, 50, 0, -1), ("dk=0", 0.8, 0.0, 3.0, 50, 0, -1), ("both=0", 0.0, 0.0, 4.0, 17, 0, -1),
        ("dk=1e-9", 0.7, 1e-9, 3.0, 17, 0, -1), ("dk=-1e-9", 0.7, -1e-9, 3.0, 17, 0, -1), ("dk=5e-324", 0.7, 5e-324, 3.0, 17, 0, -1),
        ("k0=0,dk=5e-324", 0.0, 5e-324, 3.0, 3, 0, -1),
        ("inflection", 1.5, -1.3, 2.5, 65, 0, -1),                     # kappa changes sign at s = 1.154, between two stations
        ("spiral15.8", 0.4, 0.9, 5.5, 200, 0, -1), ("spiral60", 0.5, 1.2, 9.6, 200, 0, -1),
        ("S=1", 0.85, -0.4, 2.0, 1, 0, -1), ("S=1000", 0.3, 0.05, 10.0, 1000, 1, RULE_CURV),
        ("L=1e-3", 2.0, -30.0, 1e-3, 64, 0, -1), ("L=20", 0.05, 0.004, 20.0, 65, 0, -1),
        ("ex:3.1,-4.1,1.5,2", 3.1, -4.1, 1.5, 2, 16, RULE_CURV),
        ("ex:8,-20,2,5", 8.0, -20.0, 2.0, 5, 54, RULE_CURV), ("ex:30,-10,3,2", 30.0, -10.0, 3.0, 2, 300, RULE_CURV),
        ("ex:2,300,2,17", 2.0, 300.0, 2.0, 17, 251, RULE_CURV),
    ]
    return out


def anchors(n, S):
    """does a 16-piece anchor (piece index a positive multiple of 16) fall inside a station interval / on a station?"""
    hits = [a % n for a in range(16, (S - 1) * n, 16)]
    return any(h != 0 for h in hits), any(h == 0 for h in hits)


def f64(rws, cols=4):
    return np.array([[float(v) for v in r[:cols]] for r in rws], dtype=np.float64).reshape(-1, cols)


def main():
    cases = regime_cases()
    table = []
    for lab, k0, dk, L, S, n, rule in cases:
        table.append((lab, k0, dk, L, S, n, rule, -1))
    for i, (lab, k0, dk, L, S, n, rule) in enumerate(cases):
        if lab == "S=1000":                                           # a single S = 1000
            continue
        table.append((lab + "/mirror", -k0, -dk, L, S, n, rule, i))
    P = np.array([[c[1], c[2], c[3]] for c in table], dtype=np.float64)
    S_ = np.array([c[4] for c in table], np.int32)
    ns = np.array([R.nsub(*P[i], S_[i]) for i in range(len(table))], np.int64)
    rule = np.zeros(len(table), np.int32)
    for i, c in enumerate(table):
        n1, n2sq = R.nsub_rules(*P[i], S_[i])
        rule[i] = RULE_DK if n2sq > n1 * n1 else RULE_CURV
        if c[5]:
            assert ns[i] == c[5] and (ns[i] == 1 or rule[i] == c[6]), (c, ns[i], rule[i])
        k0, dk, L = P[i]                                              # no case sits on a ceil: the doubles' arithmetic agrees on nsub
        ds = L / max(int(S_[i]) - 1, 1)
        dbl = max(1.0, np.ceil(max(abs(k0), abs(dk * L + k0)) * ds * (1.0 / 0.3)), np.ceil(ds * np.sqrt(abs(dk) * 6.25)))
        assert dbl == ns[i], (c, dbl, ns[i])
    assert ns.max() < 4096
    inside, on = zip(*(anchors(int(ns[i]), int(S_[i])) for i in range(len(table))))
    n0 = len(cases)                                                   # a mirror's rows are its original's with y negated: not stored
    off = np.concatenate([[0], np.cumsum(S_[:n0])]).astype(np.int64)
    rows = np.concatenate([f64(R.rows(*P[i], S_[i]), 2) for i in range(n0)])
    assert rows.shape == (off[-1], 2)
    for i in range(n0, len(table)):
        assert np.array_equal(f64(R.rows(*P[i], S_[i]), 2), rows[off[table[i][7]]:off[table[i][7] + 1]] * [1.0, -1.0]), table[i]
    print(f"table: {len(table)} clothoids, {off[-1]} rows, nsub {sorted(set(ns.tolist()))}, anchor inside an interval on {sum(inside)}, on a station on {sum(on)}")

    g = np.load(G14)
    idx = np.nonzero((g["ok"] == 1) & (g["ambiguous"] == 0))[0][::8]
    goals = g["goals"][idx]
    gp = np.column_stack([g["k0"][idx], g["dk"][idx], g["L"][idx]])
    assert (goals[:, 0] < 0).sum() >= 25 and (np.abs(goals[:, 2]) > 1.3).sum() >= 25
    out = dict(t_label=np.array([c[0] for c in table]), t_params=P, t_S=S_, t_nsub=ns, t_rule=rule, t_want_nsub=np.array([c[5] for c in table], np.int32),
               t_mirror_of=np.array([c[7] for c in table], np.int32), t_anchor_inside=np.array(inside), t_anchor_on_station=np.array(on),
               t_off=off, t_xy=rows, g_idx=idx.astype(np.int32))
    for S in G_S:
        out[f"g_xy_S{S}"] = np.stack([f64(R.rows(*gp[i], S), 2) for i in range(len(idx))])
        cr, sp, cd = [], [], []
        for i in range(len(idx)):
            r, s, c, _ = R.cubic_rows(*goals[i], S)
            cr.append(f64(r)); sp.append([float(v) for v in s]); cd.append([float(v) for v in c])
        out[f"c_rows_S{S}"] = np.stack(cr)
        out[f"c_sp_S{S}"] = np.array(sp, np.float32)
        out[f"c_cond_S{S}"] = np.array(cd, np.float32)
    print(f"g14 subset: {len(idx)} goals, {(goals[:, 0] < 0).sum()} behind the ego, {(np.abs(goals[:, 2]) > 1.3).sum()} with |theta| > 1.3, "
          f"largest nsub at S = 2: {max(R.nsub(*gp[i], 2) for i in range(len(idx)))}")
    np.savez_compressed(OUT, **out)
    print("written", os.path.normpath(OUT), os.path.getsize(OUT))


if __name__ == "__main__":
    main()
