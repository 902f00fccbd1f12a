"""The grazing scenes of tests/shoot_graze_ref.py meet the conditions that make tests/test_gpu_shoot_graze.py mean something (CPU)."""
import numpy as np
import pytest

import shoot_graze_ref as G


@pytest.mark.parametrize("name,T,n_sub", G.BATCHES)
def test_a_batch_is_decisive_where_it_has_to_be(orc, name, T, n_sub):
    b = G.build(orc, name, T, n_sub)
    d, inside = b["decisive"], b["inside"]
    assert d.mean() >= 0.75, int(d.sum())
    assert (b["gap0"][d] >= 10.0).all()                                 # rollout 0 wins by 10 margins without obstacles
    assert (b["win"][d & inside] > 0).all()                             # blocked: another rollout wins
    assert (b["win"][d & ~inside] == 0).all()                           # free: the warm start
    np.testing.assert_array_equal(b["win64"][d], b["win"][d])           # the float64 restatement of the rule agrees
    # the ladder: from max(1e-8, 64 x the point's fp64 deviation) to twice the allowance, the designated point's own slot
    assert (b["delta"][d] >= 64.0 * b["dev"][d]).all() and (b["delta"][d] >= 1e-8 * (1 - 1e-12)).all()
    top = d & (b["rung"] == G.N_RUNGS - 1)
    np.testing.assert_allclose(b["delta"][top], 2.0 * b["allow"][top], rtol=1e-3)
    assert (b["tstar"][d] >= T // 2).all() and (b["jstar"][d] >= 1).all() and (b["jstar"][d] <= n_sub).all()
    assert (b["jstar"][d] < n_sub).any() and (b["jstar"][d] == n_sub).any()          # interior sub-points and end points
    live = b["obs"][:, 0, 4] >= 0
    np.testing.assert_array_equal(live[d], True)
    assert len(set(b["obs"][d, 0, 4])) >= 2 and (np.hypot(b["obs"][d, 0, 2], b["obs"][d, 0, 3]) == 0).any()


@pytest.mark.parametrize("name", list(G.CONFIGS))
def test_every_rung_and_sign_has_three_decisive_egos_per_configuration(orc, name):
    batches = [G.build(orc, c, T, n_sub) for c, T, n_sub in G.BATCHES if c == name]
    for rung in range(G.N_RUNGS):
        for inside in (True, False):
            n = sum(int((b["decisive"] & (b["rung"] == rung) & (b["inside"] == inside)).sum()) for b in batches)
            assert n >= 3, (rung, inside, n)


def test_the_configurations_reach_the_three_instantiations():
    got = {(cfg.max_steer <= 0.45, G.is_iso(cfg)) for cfg in (G.make_cfg(n, 8) for n in G.CONFIGS)}
    assert got == {(True, True), (True, False), (False, False)}


def test_the_allowance_is_obs_compacts():
    """a hand case: ego at the origin heading +y at 3 m/s, T dt = 3 s, max_speed 6: reach 18; a disc at (1, 2) moving (0.5, 0) with r 0.3"""
    cfg = G.make_cfg("qxy", 30)
    S_ = (1.0 + 2.0) + 0.5 * 3.0 + 0.3 + 18.0
    assert G.allowance((0.0, 0.0, 3.0, np.pi / 2), (1.0, 2.0, 0.5, 0.0, 0.3), cfg) == pytest.approx(1e-4 * 18.0 + 1e-6 * S_, rel=1e-12)
    cfg = G.make_cfg("iso", 30)                                         # ego frame: the |.|_1 norms of the rotated vectors (here a quarter turn: the same)
    assert G.allowance((0.0, 0.0, 3.0, np.pi / 2), (1.0, 2.0, 0.5, 0.0, 0.3), cfg) == pytest.approx(1e-4 * 18.0 + 1e-6 * S_, rel=1e-9)


@pytest.mark.parametrize("name,T", G.GRID_BATCHES)
def test_a_grid_batch_is_decisive_where_it_has_to_be(orc, name, T):
    b = G.build_grid(orc, name, T)
    d, inside = b["decisive"], b["inside"]
    assert d.mean() >= 0.75, int(d.sum())
    assert (b["gap0"][d] >= 10.0).all()
    assert (b["win"][d & inside] > 0).all() and (b["win"][d & ~inside] == 0).all()
    np.testing.assert_array_equal(b["win64"][d], b["win"][d])
    assert (b["delta"][d] >= 64.0 * b["dev"][d]).all() and (b["delta"][d] >= 1e-8 * (1 - 1e-12)).all()
    assert (b["jstar"][d] >= 1).all() and (b["jstar"][d] < b["n_sub"]).all() and (b["tstar"][d] >= T // 2).all()     # interior sub-points only
    assert (b["spacing"][d] > 4.0 * G.GRID_RES).all()                   # the neighbours lie outside the 2-cell clearance zone
    img = b["grid"][0]
    assert int((img < b["grid"][4]).sum()) == int((b["cells"][:, 0] >= 0).sum()) >= int(d.sum())     # one occupied cell per placed ego
    assert b["decisive_both"].sum() >= 0.75 * G.E and not (b["decisive_both"] & ~d).any()
    assert (b["obs"][b["decisive_both"], 0, 4] > 0).all()


@pytest.mark.parametrize("name", list(G.CONFIGS))
def test_every_rung_and_sign_has_three_decisive_grid_egos_per_configuration(orc, name):
    batches = [G.build_grid(orc, c, T) for c, T in G.GRID_BATCHES if c == name]
    for rung in range(G.N_RUNGS):
        for inside in (True, False):
            n = sum(int((b["decisive"] & (b["rung"] == rung) & (b["inside"] == inside)).sum()) for b in batches)
            assert n >= 3, (rung, inside, n)


def test_the_cell_rule_restated():
    """grid_blocked on hand points: cell (3, 2) of a 10 x 10 image at res 0.5, origin (-1, -1)"""
    pts = np.array([[0.5 + 1e-9, 0.25], [0.5 - 1e-9, 0.25], [0.75, 0.0 + 1e-9], [0.75, 0.5 - 1e-9], [0.75, 0.5], [-1.0 - 1e-9, 0.0], [4.0, 0.0]], np.longdouble)
    blk, near = G.grid_blocked(pts, [(3, 2)], -1.0, -1.0, 0.5, 10)
    assert blk.tolist() == [True, False, True, True, False, True, True]
    np.testing.assert_allclose(near[:4], 1e-9, rtol=1e-6)


@pytest.mark.parametrize("name,T,n_sub", G.BATCHES)
def test_the_disc_batches_stay_inside_the_open_grid(orc, name, T, n_sub):
    b = G.build(orc, name, T, n_sub)
    assert b["decisive_grid"].mean() >= 0.75 and not (b["decisive_grid"] & ~b["decisive"]).any()
    assert int((b["grid"][0] < b["grid"][4]).sum()) == 0


@pytest.mark.parametrize("name,T,n_sub", G.STMPC_BATCHES)
def test_the_batches_for_the_dynamic_planners_kinematic_branch(orc, name, T, n_sub):
    b = G.build(orc, name, T, n_sub, stmpc=True)
    d, inside = b["decisive"], b["inside"]
    assert d.mean() >= 0.75 and (b["win"][d & inside] > 0).all() and (b["win"][d & ~inside] == 0).all()
    np.testing.assert_array_equal(b["win64"][d], b["win"][d])
    assert (b["x7"][:, 3] <= G.STMPC_V_KS).all() and (b["x7"][:, [2, 5, 6]] == 0).all()
