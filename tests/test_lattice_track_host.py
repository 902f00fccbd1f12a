"""Step 7 of a lattice plan on the CPU: the oracle's tracker against the exact reference of tests/lattice_track_ref.py on every family of verdict-edge
cases, the caps that say the cases sit where they were aimed, and negative controls that say the cases discriminate.

Families (all host goals, check_collision off, weights (1, 0, 0, 0), each once alone and once among 15 dearer decoys -- under the 1 / L length term
a dearer goal is a SHORTER one: eight near-twins shorter by 8 .. 64 ulps, six shorter by 3 .. 40 %, one NaN goal):
  a  end-radius ladders |goal| = L (1 + k 2^-52), 24 directions, 19 rungs, L in {0.3, 0.8, 2}, S in {2, 3, 50, 64, 65, 66, 100, 129}
  b  vertex ladders: station j in {1, 2, 31, 63, 64, 65, S - 2} of the emitted rows on the circle's rungs
  c  the target row's y at +-1e-6 (1 + k 2^-52), and the exactly straight goal
  d  the circle beyond the path's end; the circle inside the first segment (S = 2, 3); U-turns that leave the circle and come back (clothoid only:
     the cubic generator's paths never swing out beyond their goal's radius)
  e  |goal| at 1e-170 .. 1e160 and the zero goal: no exact verdict claimed
  f  a to d through the cubic generator, S in {50, 65}
"""
from collections import Counter

import numpy as np
import pytest

import lattice_track_ref as T

GENERATORS = ("clothoid", "cubic")


@pytest.fixture(scope="module")
def suites(orc):
    return {g: T.suite(orc, g) for g in GENERATORS}


def pursuit_on_rows(orc, rows, L, v, cfg):
    return orc.pure_pursuit_batch(np.zeros((1, 3)), np.column_stack([rows[:, 0], rows[:, 1], np.full(len(rows), v)]), L, cfg.wheelbase, cfg.max_reacquire)


def each_case(suites, generators=GENERATORS, C=None, families="abcde"):
    for g in generators:
        for p in suites[g]:
            if (C is None or p.C == C) and p.cases.family in families:
                for e in range(len(p.idx)):
                    yield p, e


@pytest.mark.parametrize("generator", GENERATORS)
def test_oracle_tracker_reproduces_its_plan_and_equals_the_exact_reference(orc, suites, generator):
    """on the oracle's own rows: pure_pursuit_batch from the origin is the plan's (status, steer, speed) bit for bit -- every case, family e included --
    and on every decided case the exact verdict: status equal, la_idx the admissible row, steer within 1e-12.  The constructed goal wins every plan."""
    wp = T.raceline()
    n = Counter()
    for p, e in each_case(suites, (generator,)):
        w = p.want
        if p.cases.family != "e":
            assert w["best_idx"][e] == p.idx[e], p.cases.tag[e]
        rows = w["best_traj"][e]
        if not np.isfinite(w["best_cost"][e]):
            assert w["status"][e] == T._abi.ST_ALL_BLOCKED and w["steer"][e] == 0.0 and w["speed"][e] == 0.0
            n["blocked"] += 1
            continue
        pp = pursuit_on_rows(orc, rows, p.cases.L, wp[w["near_idx"][e], 2], p.cfg)
        assert (pp["status"][0], pp["steer"][0], pp["speed"][0]) == (w["status"][e], w["steer"][e], w["speed"][e]), p.cases.tag[e]
        r = T.reference_cached(rows[:, :2], p.cases.L, p.cfg.wheelbase, p.cfg.max_reacquire)
        if r is None or not r.decided:
            n["undecided"] += 1
            continue
        n["decided"] += 1
        assert pp["status"][0] == r.status, (p.cases.tag[e], r)
        if r.status != T.ST_NO_LOOKAHEAD:
            assert pp["la_idx"][0] == r.la, (p.cases.tag[e], r)
            assert abs(pp["steer"][0] - r.steer[r.la]) <= 1e-12, (p.cases.tag[e], r, pp["steer"][0])
            if r.steer[r.la] == 0.0:
                assert pp["steer"][0] == 0.0
            assert pp["speed"][0] == wp[w["near_idx"][e], 2]
        else:
            assert pp["steer"][0] == 0.0 and pp["speed"][0] == 0.0
    print(generator, dict(n))
    assert n["decided"] > 1000


def ladder_verdicts(suites, generator):
    """{(plan's family, S, L, ladder id): [(decided, outcome)]} over the one-candidate plans"""
    out = {}
    for p, e in each_case(suites, (generator,), C=1, families="abc"):
        if p.cases.ladder[e] < 0:
            continue
        r = T.reference_cached(p.want["best_traj"][e, :, :2], p.cases.L)
        key = (p.cases.family, p.cases.S, p.cases.L, int(p.cases.ladder[e]))
        out.setdefault(key, []).append((p.cases.rung[e], r.decided, (r.status, r.la, r.steer.get(r.la) == 0.0)))
    return out


def test_the_cases_sit_where_they_were_aimed(suites):
    """conditions on the oracle's rows, not measurements: at most 25 % of families a to c undecided (and of a and of b alone; c's rungs 0 and +-1 lie
    inside the 4-ulp band of the 1e-6 test by construction, 6 of its 23 cases per size) and none of family d; every ladder has decided cases with
    different verdicts; at least 20 decided closing-segment answers in family a and 20 decided hits in a segment >= 64"""
    for g in GENERATORS:
        n = {f: Counter() for f in "abcd"}
        for p, e in each_case(suites, (g,), C=1, families="abcd"):
            r = T.reference_cached(p.want["best_traj"][e, :, :2], p.cases.L)
            c = n[p.cases.family]
            c["n"] += 1
            assert r is not None, p.cases.tag[e]
            c["undecided"] += not r.decided
            c["closing"] += r.decided and r.la == -1
            c["seg64"] += r.decided and r.seg64
            c["reenter"] += "d/iii" in p.cases.tag[e] and r.status == T.ST_INTERSECT and r.la < p.cases.S - 2
            c["origin"] += "d/ii" in p.cases.tag[e] and r.status == T.ST_INTERSECT and r.la == 0 and r.steer[0] == 0.0
            c["beyond"] += "d/i/" in p.cases.tag[e] and r.status == T.ST_NO_LOOKAHEAD
        print(g, {f: dict(c) for f, c in n.items()})
        abc = sum(n[f]["undecided"] for f in "abc") / sum(n[f]["n"] for f in "abc")
        assert abc <= 0.25 and n["a"]["undecided"] <= 0.25 * n["a"]["n"] and n["b"]["undecided"] <= 0.25 * n["b"]["n"]
        assert n["d"]["undecided"] == 0
        assert n["a"]["closing"] >= 20
        assert n["d"]["origin"] >= 10 and n["d"]["beyond"] >= 100
        if g == "clothoid":
            assert n["a"]["seg64"] + n["b"]["seg64"] + n["c"]["seg64"] >= 20 and n["b"]["seg64"] >= 20
            assert n["d"]["reenter"] >= 10
        for key, rungs in ladder_verdicts(suites, g).items():
            assert len({o for _, dec, o in rungs if dec}) >= 2, (g, key, sorted(rungs))


CONTROLS = (("no end-point shift", dict(shift=False)), ("no wrap loop", dict(wrap=False)), ("row i + 1 for row i", dict(row_off=1)),
            ("the hit point for the row", dict(use_hit=True)), ("only 64 segments scanned", dict(max_seg=64)), ("<= for < at 1e-6", dict(le=True)))


def test_negative_controls(orc, suites):
    """the fp64 transcription of the tracker passes every decided case; with one defect at a time it fails decided cases.  `<=` for `<` differs from
    the tracker only at |wy| == 1e-6 exactly, which the 4-ulp rule never calls decided: that control is held to the oracle's own bits on the cases
    whose target row has |y| == 1e-6 exactly (family c lands some there)."""
    fails = Counter()
    exact_1e6 = 0
    for p, e in each_case(suites, ("clothoid",), C=1, families="abcd"):
        rows = p.want["best_traj"][e, :, :2]
        r = T.reference_cached(rows, p.cases.L)
        if r.status == T.ST_INTERSECT and abs(rows[r.la, 1]) == T.WY_MIN:
            exact_1e6 += 1
            st, la, steer, _ = T.track_f64(rows, p.cases.L, le=True)
            fails["<= for < at 1e-6"] += (st, steer) != (p.want["status"][e], p.want["steer"][e]) and abs(steer - p.want["steer"][e]) > 1e-12
        if not r.decided:
            continue
        want = (r.status, r.la, r.steer.get(r.la, 0.0))
        for name, kw in (("none", {}),) + CONTROLS[:5]:
            st, la, steer, _ = T.track_f64(rows, p.cases.L, **kw)
            ok = (st, la) == want[:2] and abs(steer - want[2]) <= 1e-12 and (want[2] != 0.0 or steer == 0.0)
            fails[name] += not ok
    print(dict(fails), "cases at |wy| == 1e-6 exactly:", exact_1e6)
    assert fails["none"] == 0
    for name, _ in CONTROLS:
        assert fails[name] >= 1, name


def test_integer_decisions_against_mpmath(suites):
    """50 cases, the undecided ones first (they sit closest to a boundary): the verdict at L itself with 50-digit square roots"""
    pytest.importorskip("mpmath")
    picked = []
    cases = list(each_case(suites, GENERATORS, C=1, families="abcd"))
    refs = [T.reference_cached(p.want["best_traj"][e, :, :2], p.cases.L) for p, e in cases]
    near = [q for q, r in enumerate(refs) if not r.decided and p_family(cases[q]) in "ab"]
    rng = np.random.default_rng(7)
    picked = list(rng.choice(near, 30, replace=False)) + list(rng.choice(len(cases), 20, replace=False))
    for q in picked:
        p, e = cases[q]
        assert T.reference_mp(p.want["best_traj"][e, :, :2], p.cases.L) == (refs[q].status, refs[q].la), p.cases.tag[e]


def p_family(case):
    return case[0].cases.family


def test_exact_reference_off_the_origin(orc):
    """the rules a path that starts at the origin never uses -- a start parameter inside a segment, a wrap loop over more than the closing segment,
    re-acquisition -- on 400 random polylines that pass the origin at a distance: the oracle's pure pursuit equals the exact verdict wherever it is decided"""
    rng = np.random.default_rng(11)
    n = Counter()
    for _ in range(400):
        S = int(rng.integers(3, 14))
        rows = np.cumsum(rng.normal(0.0, 0.4, (S, 2)), axis=0)
        rows -= rows[rng.integers(0, S)] + rng.normal(0.0, 0.2, 2)                 # some vertex within a few decimetres of the origin
        L = float(rng.choice([0.15, 0.4, 0.8, 1.5]))
        r = T.reference(rows, L, v=2.5)
        pp = orc.pure_pursuit_batch(np.zeros((1, 3)), np.column_stack([rows, np.full(S, 2.5)]), L)
        if not r.decided:
            n["undecided"] += 1
            continue
        assert pp["status"][0] == r.status, (rows, L, r)
        n[("INTERSECT", "REACQUIRE", "NO_LOOKAHEAD")[r.status]] += 1
        if r.status != T.ST_NO_LOOKAHEAD:
            assert pp["la_idx"][0] == r.la or r.status == T.ST_REACQUIRE, (rows, L, r, pp)
            assert abs(pp["steer"][0] - r.steer[r.la]) <= 1e-12 and pp["speed"][0] == 2.5, (rows, L, r, pp)
            n["wrap"] += r.status == T.ST_INTERSECT and r.la < pp["near_idx"][0]
    print(dict(n))
    assert n["INTERSECT"] > 100 and n["REACQUIRE"] > 20 and n["wrap"] > 10 and n["undecided"] < 20
