"""Rivals on the CPU: hand cases for the numpy reference of the rule (tests/rivals_ref.py), the reference against the examples' host
construction, and the planner classes' rejections -- on the stub library of tools/record_runtime_calls.py, where nothing may reach the
C-ABI before the ValueError."""
import importlib.util
import os

import numpy as np
import pytest

import rivals_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _st(xy, v=None, yaw=None):
    xy = np.asarray(xy, dtype=np.float64)
    E = xy.shape[0]
    return np.column_stack([xy, np.ones(E) if v is None else v, np.zeros(E) if yaw is None else yaw])


# ---- the reference, by hand --------------------------------------------------------------------------------------------------------
def test_two_vehicles():
    st = _st([[0.0, 0.0], [3.0, 4.0]], v=[2.0, -3.0], yaw=[0.0, np.pi / 2])
    r = ref.rivals(st, ref.XYVYAW, 2, 0.4)
    assert r["idx"].tolist() == [[1, -1], [0, -1]]
    assert r["obs"][0, 0, [0, 1, 4]].tolist() == [3.0, 4.0, 0.4] and abs(r["obs"][0, 0, 2]) < 1e-15 and r["obs"][0, 0, 3] == -3.0
    assert r["obs"][1, 0].tolist() == [0.0, 0.0, 2.0, 0.0, 0.4]
    assert r["obs"][0, 1].tolist() == list(ref.EMPTY) == r["obs"][1, 1].tolist()
    assert r["pace"].tolist() == [0.5, 1.0 / 3.0]
    # the other two layouts carry the same vehicles
    pose = st[:, [0, 1, 3, 2]]
    st7 = np.zeros((2, 7)); st7[:, [0, 1, 3]] = st[:, [0, 1, 2]]; st7[:, 4] = st[:, 3] - 0.25; st7[:, 6] = 0.25
    for lay, s in ((ref.POSE, pose), (ref.ST7, st7)):
        q = ref.rivals(s, lay, 2, 0.4)
        assert (q["idx"] == r["idx"]).all() and (q["pace"] == r["pace"]).all() and np.abs(q["obs"] - r["obs"]).max() < 1e-15


def test_tie_broken_by_index():
    st = _st([[0.0, 0.0], [0.0, 1.0], [1.0, 0.0], [-1.0, 0.0], [0.0, -1.0]])
    r = ref.rivals(st, ref.XYVYAW, 2, 0.3)
    assert r["idx"][0].tolist() == [1, 2]                       # four rivals at d2 == 1: the two lowest indices, in order
    assert ref.rivals(st, ref.XYVYAW, 4, 0.3)["idx"][0].tolist() == [1, 2, 3, 4]


def test_coincident_pair_is_ordinary():
    st = _st([[1.0, 1.0], [1.0, 1.0], [2.0, 1.0]])
    r = ref.rivals(st, ref.XYVYAW, 2, 0.3)
    assert r["idx"].tolist() == [[1, 2], [0, 2], [0, 1]]
    assert r["obs"][0, 0, :2].tolist() == [1.0, 1.0]


def test_nan_position_sorts_first():
    st = _st([[0.0, 0.0], [0.5, 0.0], [np.nan, 0.0], [9.0, 0.0]])
    r = ref.rivals(st, ref.XYVYAW, 2, 0.3, reach=1.0)           # (reach does not drop a NaN d2)
    assert r["idx"].tolist() == [[2, 1], [2, 0], [0, 1], [2, -1]]   # the NaN vehicle is everybody's slot 0; its own d2 are all NaN: by index
    assert np.isnan(r["obs"][0, 0, 0]) and np.isnan(r["obs"][3, 0, 0])
    v = np.array([1.0, np.nan, 0.1, -4.0])
    assert np.array_equal(ref.rivals(_st(np.zeros((4, 2)), v=v), ref.XYVYAW, 1, 0.3)["pace"], [1.0, np.nan, 2.0, 0.25], equal_nan=True)


REACH_CUT = [[0.0, 0.0], [1.25, 0.0], [-1.25, 2.0 ** -26]]       # from vehicle 0: d2 = 1.5625 = 1.25^2 exactly, and 1.5625 + 2^-52


def test_reach_cuts_above_the_square_not_at_it():
    reach = 1.25
    st = _st(REACH_CUT)
    assert 1.25 * 1.25 + 2.0 ** -52 == np.nextafter(reach * reach, np.inf)     # vehicle 2: d2 one ulp above reach^2, exactly
    r = ref.rivals(st, ref.XYVYAW, 2, 0.3, reach=reach)
    assert r["idx"][0].tolist() == [1, -1]                      # kept at d2 == reach^2, dropped one ulp above
    assert ref.rivals(st, ref.XYVYAW, 2, 0.3, reach=0.0)["idx"].tolist() == [[-1, -1]] * 3
    assert ref.rivals(_st([[0.0, 0.0], [0.0, 0.0]]), ref.XYVYAW, 1, 0.3, reach=0.0)["idx"].tolist() == [[1], [0]]


def test_negative_group_and_small_race():
    st = _st([[0.0, 0.0], [1.0, 0.0], [2.0, 0.0], [3.0, 0.0], [4.0, 0.0], [5.0, 0.0]])
    g = [7, -1, 7, 3, -5, 7]
    r = ref.rivals(st, ref.XYVYAW, 3, 0.3, groups=g)
    assert r["idx"].tolist() == [[2, 5, -1], [-1, -1, -1], [0, 5, -1], [-1, -1, -1], [-1, -1, -1], [2, 0, -1]]
    assert (r["obs"][1] == ref.EMPTY).all() and (r["obs"][3] == ref.EMPTY).all() and (r["obs"][0, 2] == ref.EMPTY).all()
    assert np.isfinite(r["pace"]).all()                         # the pace is every ego's, grouped or not


def test_reference_equals_the_examples_construction():
    rng = np.random.default_rng(5)
    E, M = 40, 4
    st = np.column_stack([rng.uniform(-20, 20, (E, 2)), rng.uniform(0.0, 6.0, E), rng.uniform(-3, 3, E)])
    obs, near = ref.example_obstacles(st, M, 0.45)
    d = np.hypot(st[:, None, 0] - st[None, :, 0], st[:, None, 1] - st[None, :, 1])
    assert all(len(np.unique(row)) == E for row in d)           # tie-free: hypot's order is d2's
    r = ref.rivals(st, ref.XYVYAW, M, 0.45)
    assert (r["idx"] == near).all() and np.array_equal(r["obs"], obs)


# ---- the classes' rejections: ValueError before anything touches the GPU ------------------------------------------------------------
@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("record_runtime_calls", os.path.join(ROOT, "tools", "record_runtime_calls.py"))
    t = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(t)
    return t


E = 3
WP = np.random.default_rng(2).normal(size=(6, 5))
COURSE = [WP[:, 0], WP[:, 1], WP[:, 3], WP[:, 2]]


def _planners(tool):
    """(name, factory(**config), plan args, plan_batch args, waypoints)"""
    from f1tenth_planning_amd.control.dynamic_mpc.dynamic_mpc import STMPCPlanner
    from f1tenth_planning_amd.control.dynamic_mpc.dynamic_mpc import mpc_config as stmpc_config
    from f1tenth_planning_amd.control.kinematic_mpc.kinematic_mpc import KMPCPlanner
    from f1tenth_planning_amd.control.kinematic_mpc.kinematic_mpc import mpc_config as kmpc_config
    from f1tenth_planning_amd.planning.lattice_planner.lattice_planner import LatticePlanner

    def make(cls, config):
        def f(**cfg):
            p = cls(config=config(**cfg)) if config is not None else cls()
            p._ctx = tool.stub_context()
            return p
        return f
    return [("KMPCPlanner", make(KMPCPlanner, kmpc_config), (np.zeros(7),), (np.zeros((E, 4)),), COURSE),
            ("STMPCPlanner", make(STMPCPlanner, stmpc_config), (np.zeros(7),), (np.zeros((E, 7)),), COURSE),
            ("LatticePlanner", make(LatticePlanner, None), (0.0, 0.0, 0.0, 1.0), (np.zeros((E, 4)),), WP)]


def _rejected(p, call, match):
    with pytest.raises(ValueError, match=match):
        call()
    assert p._ctx.lib.log == [], "the library was reached before the rejection"


@pytest.mark.parametrize("k", [0, 1, 2])
def test_class_rejections(tool, k):
    from f1tenth_planning_amd import Rivals
    name, make, plan_args, batch_args, wp = _planners(tool)[k]
    riv = Rivals(count=2, radius=0.45)
    assert riv.reach == np.inf and riv.groups is None
    with pytest.raises(Exception):                              # frozen
        riv.count = 3

    p = make(); p.rivals = riv
    _rejected(p, lambda: p.plan(*plan_args, waypoints=wp), "one ego")
    p = make(); p.rivals = riv; p.obstacles = np.zeros((E, 1, 5))
    _rejected(p, lambda: p.plan_batch(*batch_args, waypoints=wp), "rivals and planner.obstacles")
    assert p.obstacles is None and p.rivals is riv              # obstacles are taken, rivals persist
    for bad in (0, 17):
        p = make(); p.rivals = Rivals(count=bad, radius=0.45)
        _rejected(p, lambda: p.plan_batch(*batch_args, waypoints=wp), r"count must be in \[1, 16\]")
    for groups in (np.zeros(E - 1, int), np.zeros(E + 1, int)):
        p = make(); p.rivals = Rivals(count=2, radius=0.45, groups=groups)
        _rejected(p, lambda: p.plan_batch(*batch_args, waypoints=wp), "one id per ego")
    if name == "LatticePlanner":
        p = make(); p.rivals = riv
        _rejected(p, lambda: p.plan_batch(*batch_args, waypoints=wp, devices=[0]), "multi-GPU")
        p = make(); p.rivals = Rivals(count=2, radius=0.45, groups=np.zeros(E + 1, int))
        _rejected(p, lambda: p.step_batch(*batch_args, waypoints=wp), "one id per ego")
        p = make(); p.rivals = riv; p.obstacles = np.zeros((E, 1, 5))
        _rejected(p, lambda: p.step_batch(*batch_args, waypoints=wp), "rivals and planner.obstacles")
    else:
        p = make(SOLVER="qp"); p.rivals = riv
        _rejected(p, lambda: p.plan_batch(*batch_args, waypoints=wp), "SOLVER='qp'")


@pytest.mark.parametrize("k", [0, 1, 2])
def test_accepted_call_reaches_the_library_in_order(tool, k):
    """groups, state upload, f1p_rivals_dev with the planner's layout, the planner's *_set_obstacles_dev, then the plan; rivals = None
    afterwards clears the context's obstacles"""
    from f1tenth_planning_amd import Rivals
    name, make, _, batch_args, wp = _planners(tool)[k]
    p = make(); p.rivals = Rivals(count=2, radius=0.45, reach=7.0, groups=[0, 0, 1])
    p.plan_batch(*batch_args, waypoints=wp)
    names = [c[0] for c in p._ctx.lib.log]
    setter = {"KMPCPlanner": "f1p_kmpc_set_obstacles_dev", "STMPCPlanner": "f1p_stmpc_set_obstacles_dev", "LatticePlanner": "f1p_lattice_set_obstacles_dev"}[name]
    plan = {"KMPCPlanner": "f1p_kmpc_plan_batch", "STMPCPlanner": "f1p_stmpc_plan_batch", "LatticePlanner": "f1p_lattice_plan_batch"}[name]
    order = [names.index(n) for n in ("f1p_rivals_set_groups", "f1p_h2d", "f1p_rivals_dev", setter, plan)]
    assert order == sorted(order), names
    call = p._ctx.lib.log[names.index("f1p_rivals_dev")][1]
    layout = {"KMPCPlanner": 0, "STMPCPlanner": 2, "LatticePlanner": 1}[name]
    assert call[2:8] == [["i", layout], ["i", E], ["i", 2], ["f", 0.45], ["f", 7.0], ["f", 0.5]] and call[8] == "ptr"
    assert p._ctx.lib.log[names.index(setter)][1][-2:] == [["i", E], ["i", 2]]
    # a second call: same buffers, the groups are not uploaded again
    p._ctx.lib.log.clear()
    p.plan_batch(*batch_args, waypoints=wp)
    names = [c[0] for c in p._ctx.lib.log]
    assert "f1p_dev_alloc" not in names and "f1p_rivals_set_groups" not in names and "f1p_rivals_dev" in names
    # switched off: the obstacles are cleared once, then nothing
    p.rivals = None
    for want in (1, 0):
        p._ctx.lib.log.clear()
        p.plan_batch(*batch_args, waypoints=wp)
        names = [c[0] for c in p._ctx.lib.log]
        assert "f1p_rivals_dev" not in names and sum(n.endswith("_set_obstacles") for n in names) == want, names
