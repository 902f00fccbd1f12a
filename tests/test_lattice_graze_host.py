"""The lattice grazing scenes of tests/lattice_graze_ref.py meet the conditions tests/test_gpu_lattice_graze.py relies on (CPU)."""
import numpy as np

import lattice_graze_ref as G
import lattice_obstacle_ref as O


def test_the_axis_scene_grazes_the_last_station_of_a_straight_candidate(orc):
    s = G.axis_scene(orc)
    E = s["E"]
    w = s["want_nomap"]
    ar = np.arange(E)
    pen = w["pen"][ar, s["star"]]                                       # the designated candidate's deepest penetration r - d
    want_pen = np.where(s["inside"], s["delta"], -s["delta"])
    np.testing.assert_allclose(pen, want_pen, rtol=1e-3, atol=1e-12)
    np.testing.assert_array_equal(w["blocked"][ar, s["star"]], s["inside"])
    assert (s["delta"] >= 1e-8 * (1 - 1e-12)).all() and (np.abs(pen) > 8 * O.DISC_EPS).all()
    for rung in range(G.N_RUNGS):
        for inside in (True, False):
            assert int(((s["rung"] == rung) & (s["inside"] == inside)).sum()) >= 3
    top = s["rung"] == G.N_RUNGS - 1
    assert (s["delta"][top] > 1e-5).all() and (s["delta"][top] < 3e-5).all()       # twice an eps of 1e-6 (|a| + |g| + L + 2 r) + 1e-6, operands of 1 .. 3 m
    straight = s["want"]["base"]["all_traj"][:, :G.N_STRAIGHT]
    assert np.abs(straight[..., 1]).max() < 1e-12 and np.abs(straight[..., 2]).max() < 1e-12    # the straight candidates are straight
    for k in ("want", "want_nomap"):
        m = ~s[k]["fragile"] & ~s[k]["all_blocked"]
        assert m.mean() >= 0.75, k


def test_the_random_scene_blocks_a_tenth_to_a_third(orc):
    s = G.random_scene(orc)
    assert 0.10 <= s["share"] <= 0.30, s["share"]
    assert (s["obs"][:, :, 4] >= 0).sum() >= 0.9 * s["obs"].shape[0] * O.M_SLOTS
    for k in ("want", "want_nomap"):
        m = ~s[k]["fragile"] & ~s[k]["all_blocked"]
        assert m.mean() >= 0.75, k
