"""tests/session_script.py on the CPU: the generator (deterministic, every kind, every pattern a-j found by scans of the list that do not
use the generator's own tags or assertion), the witness's set-up against a hand-written table, the replay's comparison on fake contexts
-- a context that keeps a stale grid is reported at the right operation -- and a dry run of the real driver's calls against
runtime.Context's signatures."""
import inspect
import zlib

import numpy as np
import pytest

import session_script as ss
from session_script import MUTATORS, RESETS, Model, Op

SCRIPTS = {seed: ss.script(seed) for seed in ss.SEEDS}

GRID = {"set_grid", "inflate_grid", "set_footprint"}
LAT = GRID | {"lattice_set_clearance", "lattice_set_mode", "lattice_set_pipeline", "lattice_set_split", "lattice_set_order", "lattice_set_closed_loop",
              "lattice_set_obstacles"}
KSH = GRID | {"kmpc_set_mode", "kmpc_set_groups", "kmpc_set_collision", "kmpc_set_obstacles"}
SSH = GRID | {"stmpc_set_mode", "stmpc_set_collision", "stmpc_set_obstacles"}
SQP = GRID | {"kmpc_qp_set_pack", "stmpc_qp_set_avoid", "stmpc_qp_set_walls", "stmpc_set_obstacles"}
# query kind -> the mutators it reads, written out by hand from csrc/ (what each entry point and its launcher take from f1p_ctx)
TABLE = {
    "nearest_point": {"set_waypoints"}, "intersect_point": {"set_waypoints"}, "stanley": {"set_waypoints"}, "lqr": {"set_waypoints"},
    "pure_pursuit": {"set_waypoints", "pure_pursuit_set_form"},
    "nearest_point_tracks": {"set_tracks"}, "pure_pursuit_tracks": {"set_tracks"}, "stanley_tracks": {"set_tracks"}, "lqr_tracks": {"set_tracks"},
    "kmpc_ref": {"set_waypoints", "kmpc_set_yaw_fixup"}, "kmpc_ref_tracks": {"set_tracks", "kmpc_set_yaw_fixup"},
    "stmpc_ref": {"set_waypoints"}, "stmpc_ref_tracks": {"set_tracks"},
    "kmpc_predict": set(), "stmpc_predict": set(),
    "grid_occupied": GRID, "grid_distance": {"set_grid"},
    "lattice_plan": LAT | {"set_waypoints"}, "lattice_step": LAT | {"set_waypoints"}, "lattice_plan_tracks": LAT | {"set_tracks"},
    "kmpc_shoot": KSH, "kmpc_plan": KSH | {"set_waypoints", "kmpc_set_yaw_fixup"},
    "stmpc_shoot": SSH, "stmpc_plan": SSH | {"set_waypoints", "kmpc_set_mode", "kmpc_set_groups"},
    "kmpc_qp": {"kmpc_qp_set_pack"}, "kmpc_qp_avoid": {"kmpc_qp_set_pack"}, "kmpc_qp_walls": GRID | {"kmpc_qp_set_pack"},
    "stmpc_qp": set(), "stmpc_qp_avoid": set(), "stmpc_qp_walls": GRID,
    "kmpc_qp_plan": GRID | {"set_waypoints", "kmpc_set_yaw_fixup", "kmpc_qp_set_pack", "kmpc_qp_set_avoid", "kmpc_qp_set_walls", "kmpc_set_obstacles"},
    "stmpc_qp_plan": SQP | {"set_waypoints"}, "stmpc_qp_plan_tracks": SQP | {"set_tracks"},
    "rivals": {"rivals_set_groups"}, "rivals_predict": {"rivals_set_groups", "rivals_set_course", "set_waypoints", "set_tracks"},
}
MUTATOR_KINDS = ["set_waypoints", "set_tracks", "set_grid", "inflate_grid", "set_footprint", "lattice_set_clearance", "lattice_set_mode",
                 "lattice_set_pipeline", "lattice_set_split", "lattice_set_order", "lattice_set_closed_loop", "lattice_set_obstacles",
                 "pure_pursuit_set_form", "kmpc_set_mode", "stmpc_set_mode", "kmpc_set_groups", "kmpc_set_yaw_fixup", "kmpc_qp_set_pack",
                 "kmpc_set_collision", "stmpc_set_collision", "kmpc_set_obstacles", "stmpc_set_obstacles", "kmpc_qp_set_avoid", "kmpc_qp_set_walls",
                 "stmpc_qp_set_avoid", "stmpc_qp_set_walls", "rivals_set_groups", "rivals_set_course", "kmpc_warm_reset", "kmpc_qp_warm_reset",
                 "stmpc_warm_reset", "stmpc_qp_warm_reset"]
LINE_PTS = {0: 150, 1: 320, 2: 600}


def is_query(op):
    return op.kind in TABLE


def family(kind):
    if kind.startswith("lattice") or kind.startswith("grid"):
        return "lattice"
    if kind.startswith("rivals"):
        return "rivals"
    if kind.startswith(("kmpc", "stmpc")):
        return "mpc"
    return "trackers"


def walk(ops):
    """(index, op, the mutator values in force before it) for every op"""
    now = {k: dict(v) for k, v in MUTATORS.items()}
    for n, op in enumerate(ops):
        yield n, op, {k: dict(v) for k, v in now.items()}
        if op.kind in MUTATORS:
            now[op.kind] = dict(op.kw)
            if op.kind == "set_grid":
                now["inflate_grid"], now["set_footprint"] = dict(radius=0.0), dict(on=False)


# ---- the generator ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", ss.SEEDS)
def test_script_is_deterministic(seed):
    assert ss.script(seed) == SCRIPTS[seed]
    assert ss.script(seed + 1) != SCRIPTS[seed]


@pytest.mark.parametrize("seed", ss.SEEDS)
def test_every_mutator_and_query_kind_occurs(seed):
    kinds = {op.kind for op in SCRIPTS[seed]}
    assert set(MUTATOR_KINDS) <= kinds and set(TABLE) <= kinds
    assert kinds <= set(MUTATOR_KINDS) | set(TABLE)
    plans = [op.kw for op in SCRIPTS[seed] if op.kind == "lattice_plan"]
    for key, values in (("goals", {"host", None}), ("prev", {True, None}), ("f32", {True, None}), ("prune", {True, None}), ("gen", {"cubic", None}),
                        ("grid", {"4x7", "8x8"}), ("S", {20, 37})):
        assert values <= {kw.get(key) for kw in plans}, key
    pred = [(op.kw["speed"], op.kw["min_speed"]) for op in SCRIPTS[seed] if op.kind == "rivals_predict"]
    assert {s for s, _ in pred} == {"constant", "profile"} and len({m for s, m in pred if s == "profile"}) >= 2
    for kind, key, values in (("kmpc_shoot", "T", {8, 20}), ("stmpc_shoot", "T", {20, 21}), ("kmpc_shoot", "R", {64, 256}), ("kmpc_qp", "T", {8, 16}),
                              ("stmpc_qp", "T", {10, 20}), ("set_tracks", "K", {1, 3, 6}), ("set_grid", "map", {None, 0, 1, 2}),
                              ("inflate_grid", "radius", {0.0, 0.1, 0.3}), ("lattice_set_mode", "mixed", {0, 1, 2})):
        assert values <= {op.kw[key] for op in SCRIPTS[seed] if op.kind == kind}, (kind, key)
    assert {op.kw["E"] for op in SCRIPTS[seed] if is_query(op) and "E" in op.kw} == set(ss.E_SET)
    assert all(m["h"] <= 400 and m["w"] <= 400 for m in ss.MAPS) and any(m["w"] % 32 for m in ss.MAPS)
    assert len({m["h"] for m in ss.MAPS}) == len({m["w"] for m in ss.MAPS}) == len({m["res"] for m in ss.MAPS}) == 3


# ---- the patterns, each by its own scan ----------------------------------------------------------------------------------------------
def _triple(ops, kind, cond):
    """the largest E, the smallest, a middle one of `kind` under `cond`, another subsystem's query between each two"""
    want, stage, gap = [{300}, {1}, {33, 65, 130}], 0, True
    for n, op, now in walk(ops):
        if not is_query(op):
            continue
        if op.kind == kind and cond(op, now) and op.kw["E"] in want[stage] and gap:
            stage, gap = stage + 1, False
            if stage == 3:
                return True
        elif stage and family(op.kind) != family(kind):
            gap = True
    return False


@pytest.mark.parametrize("seed", ss.SEEDS)
def test_pattern_a_scratch_owners_see_large_small_middle(seed):
    ops = SCRIPTS[seed]
    owners = [("lattice_plan", lambda op, now: now["lattice_set_mode"]["mixed"] == 2 and not now["lattice_set_obstacles"]["E"]),
              ("lattice_plan", lambda op, now: now["lattice_set_mode"]["mixed"] == 2 and now["lattice_set_obstacles"]["E"] == op.kw["E"]),
              ("lattice_plan", lambda op, now: now["lattice_set_mode"]["mixed"] == 0 and op.kw.get("prune")),
              ("lattice_plan", lambda op, now: now["lattice_set_split"]["groups"] > 0),
              ("lattice_plan", lambda op, now: now["lattice_set_closed_loop"]["on"]),
              ("lattice_step", lambda op, now: True), ("lattice_plan_tracks", lambda op, now: True),
              ("kmpc_plan", lambda op, now: now["kmpc_set_groups"]["groups"] > 1 and op.kw["R"] >= 256),
              ("stmpc_shoot", lambda op, now: now["stmpc_set_mode"]["mixed"]), ("stmpc_plan", lambda op, now: True),
              ("kmpc_qp_plan", lambda op, now: True), ("stmpc_qp_plan", lambda op, now: True),
              ("rivals_predict", lambda op, now: True), ("rivals", lambda op, now: now["rivals_set_groups"]["E"] == op.kw["E"])]
    for k, (kind, cond) in enumerate(owners):
        assert _triple(ops, kind, cond), (k, kind)


def _clear_cells(kw, res, r, foot):
    la, wd = {"4x7": (1.0, 0.4), "8x8": (1.6, 0.45)}[kw["grid"]]
    ds = 1.2 * (la * la + wd * wd) ** 0.5 / (kw["S"] - 1)
    if kw.get("goals") == "host":
        ds = 1.2 * 4.0 / (kw["S"] - 1)
    if foot:
        ds *= 1.0 + 0.3
    return r * ds * 1.001 / res + 2.41422


@pytest.mark.parametrize("seed", ss.SEEDS)
def test_pattern_b_clearance_bitmap_after_every_grid_change(seed):
    ops = SCRIPTS[seed]
    mode2 = lambda op, now: op.kind == "lattice_plan" and now["lattice_set_mode"]["mixed"] == 2 and now["set_grid"]["map"] is not None   # noqa: E731
    steps = list(walk(ops))
    first = next(n for n, op, now in steps if mode2(op, now) and now["lattice_set_clearance"]["r"] > 0)
    seen = set()
    for n, op, now in steps[first + 1:]:
        if op.kind not in ("set_grid", "inflate_grid", "set_footprint", "lattice_set_clearance") or n + 1 >= len(ops):
            continue
        nxt = next((s for s in steps[n + 1:] if is_query(s[1])), None)
        if nxt is None or not mode2(nxt[1], nxt[2]):
            continue
        if op.kind == "set_grid" and op.kw["map"] is not None and now["set_grid"]["map"] is not None:
            a, b = ss.MAPS[op.kw["map"]], ss.MAPS[now["set_grid"]["map"]]
            if a["h"] != b["h"] and a["w"] != b["w"] and a["res"] != b["res"]:
                seen.add("set_grid")
        elif op.kind == "set_footprint":
            seen.add("footprint on" if op.kw["on"] else "footprint off")
        elif op.kind != "set_grid":
            seen.add(op.kind)
    assert seen == {"set_grid", "inflate_grid", "footprint on", "footprint off", "lattice_set_clearance"}
    # the reuse window of ensure_clear_map (k_grid.hip): a map built for `held` cells serves a plan that wants fewer, down to (held - 0.5) / 1.3
    held, hit = None, False
    for n, op, now in steps:
        if op.kind in ("set_grid", "inflate_grid", "set_footprint") or (is_query(op) and op.kind in ("kmpc_plan", "stmpc_plan", "kmpc_shoot")):
            held = None
        if not mode2(op, now) or now["lattice_set_clearance"]["r"] == 0:
            continue
        want = _clear_cells(op.kw, ss.MAPS[now["set_grid"]["map"]]["res"], now["lattice_set_clearance"]["r"], now["set_footprint"]["on"])
        if held is not None and held >= want and held <= 1.3 * want + 0.5:
            hit = hit or (want < held <= 8.0)             # (<= 8 cells: inside the clearance mode's own bound of a quarter of the >= 32-row tile)
        else:
            held = want
    assert hit
    small = [op.kw["radius"] for op in ops if op.kind == "inflate_grid" and 0.0 < op.kw["radius"] < 0.3]
    assert small


@pytest.mark.parametrize("seed", ss.SEEDS)
def test_pattern_c_shorter_then_longer_raceline(seed):
    ops = SCRIPTS[seed]
    sets = [n for n, op in enumerate(ops) if op.kind == "set_waypoints"]
    ok = {}
    for a, b in zip(sets, sets[1:] + [len(ops)]):
        prev = next((ops[p].kw["line"] for p in reversed(sets) if p < a), None)
        if prev is None:
            continue
        span = [op for op in ops[a + 1:b] if is_query(op)]
        kinds = {op.kind for op in span}
        ms = [op.kw["min_speed"] for op in span if op.kind == "rivals_predict" and op.kw["speed"] == "profile"]
        again = any(x == y and y != z for x, y, z in zip(ms, ms[1:], ms[2:]))
        if kinds & {"pure_pursuit", "stanley", "nearest_point", "lqr"} and {"kmpc_ref", "lattice_plan"} <= kinds and again:
            ok.setdefault("shorter" if LINE_PTS[ops[a].kw["line"]] < LINE_PTS[prev] else "longer", a)
    assert "shorter" in ok and "longer" in ok and any(ok["shorter"] < a for a in sets if a >= ok["longer"])


@pytest.mark.parametrize("seed", ss.SEEDS)
def test_pattern_d_another_track_set_between_tracks_queries(seed):
    ops = SCRIPTS[seed]
    for kind in [k for k in TABLE if k.endswith("_tracks")] + ["rivals_predict"]:
        at = [(n, now["set_tracks"]["K"]) for n, op, now in walk(ops)
              if op.kind == kind and (kind != "rivals_predict" or now["rivals_set_course"]["E"])]
        assert any(k0 != k1 for (_, k0), (_, k1) in zip(at, at[1:])), kind


@pytest.mark.parametrize("seed", ss.SEEDS)
def test_pattern_e_configuration_table_wraps_between_two_calls(seed):
    calls = []
    for op in SCRIPTS[seed]:
        if op.kind in ("kmpc_shoot", "kmpc_plan"):
            calls.append(("k", (op.kw["T"], op.kw["R"], op.kw.get("cfg", 0))))
        elif op.kind == "stmpc_plan":
            calls.append(("s", (op.kw["TK"], op.kw["R"], op.kw.get("cfg", 0))))
    assert len({c for _, c in calls}) >= 10
    for fam in "ks":
        wrapped = False
        for a, (fa, ca) in enumerate(calls):
            for b in range(a + 1, len(calls)):
                if calls[b] == (fa, ca) and fa == fam:
                    between = {c for f, c in calls[a + 1:b] if f != fam and c != ca}
                    wrapped = wrapped or len(between) >= 8
                    break
        assert wrapped, fam


@pytest.mark.parametrize("seed", ss.SEEDS)
def test_pattern_f_obstacles_of_one_batch_size_then_another(seed):
    ops = SCRIPTS[seed]
    for kind, plan in (("lattice_set_obstacles", "lattice_plan"), ("kmpc_set_obstacles", "kmpc_plan"), ("stmpc_set_obstacles", "stmpc_plan")):
        found = False
        for n, op, now in walk(ops):
            held = now[kind]["E"]
            if op.kind == plan and held and op.kw["E"] != held and op.expect == "error":
                rest = ops[n + 1:]
                clear = next((k for k, o in enumerate(rest) if o.kind == kind), None)
                if clear is not None and rest[clear].kw["E"] == 0:
                    nxt = next((o for o in rest[clear + 1:] if is_query(o)), None)
                    found = found or (nxt is not None and nxt.kind == plan and nxt.kw["E"] == op.kw["E"] and not nxt.expect)
        assert found, kind
    assert all(op.expect in ("", "error", "einval") for op in ops)


@pytest.mark.parametrize("seed", ss.SEEDS)
def test_pattern_g_argument_error_between_two_identical_queries(seed):
    ops = SCRIPTS[seed]
    q = [(n, op) for n, op in enumerate(ops) if is_query(op)]
    fams = set()
    for (a, first), (_, bad), (_, second) in zip(q, q[1:], q[2:]):
        if bad.expect == "einval" and bad.kw.get("bad") and not first.expect and (first.kind, first.kw, first.seed) == (second.kind, second.kw, second.seed) \
                and second.same_as == a and (first.kind == "lattice_plan" or not first.kind.endswith(("_plan", "_step"))):
            fams.add({"stanley": "trackers", "kmpc_ref": "references", "grid_occupied": "grid", "lattice_plan": "lattice", "kmpc_shoot": "shooting",
                      "kmpc_qp": "qp", "rivals": "rivals"}.get(first.kind, first.kind))
    assert fams >= {"trackers", "references", "grid", "lattice", "shooting", "qp", "rivals"}
    for n, op in q:
        if op.kind == "lattice_plan" and op.same_as >= 0:
            assert not next(now for k, o, now in walk(ops) if k == n)["lattice_set_closed_loop"]["on"]


@pytest.mark.parametrize("seed", ss.SEEDS)
def test_pattern_h_every_switch_away_and_back_with_a_reader(seed):
    ops = SCRIPTS[seed]
    switches = [k for k in MUTATOR_KINDS if k not in ("set_waypoints", "set_tracks") and not k.endswith("warm_reset")]
    readers = {k: {q for q, reads in TABLE.items() if k in reads} for k in switches}
    away, back = set(), set()
    for n, op in enumerate(ops[:-1]):
        if op.kind not in readers or ops[n + 1].kind not in readers[op.kind]:
            continue
        if op.kw != MUTATORS[op.kind]:
            away.add(op.kind)
        else:
            back.add(op.kind)
    assert away == set(switches) and back == set(switches), (set(switches) - away, set(switches) - back)
    for reset, plan in (("kmpc_warm_reset", "kmpc_plan"), ("kmpc_qp_warm_reset", "kmpc_qp_plan"), ("stmpc_warm_reset", "stmpc_plan"),
                        ("stmpc_qp_warm_reset", "stmpc_qp_plan")):
        assert any(a.kind == plan and b.kind == reset and c.kind == plan and (a.kw, b.kw) == (c.kw, {}) for a, b, c in zip(ops, ops[1:], ops[2:])), reset


@pytest.mark.parametrize("seed", ss.SEEDS)
def test_pattern_i_closed_loop_chain_interrupted_and_resumed(seed):
    ops = SCRIPTS[seed]

    def chain(kind, armed, need):
        """`need` calls of one shape, a lattice plan of another E, a kmpc_plan, the shape again -- with closed-loop mode `armed` throughout"""
        run, shape, stage = 0, None, 0
        for n, op, now in walk(ops):
            if op.kind == "lattice_set_closed_loop" or (is_query(op) and now["lattice_set_closed_loop"]["on"] != armed):
                run, shape, stage = 0, None, 0
                continue
            if not is_query(op):
                continue
            s = (op.kw.get("E"), op.kw.get("S"))
            if op.kind == kind and stage == 0:
                run, shape = (run + 1, s) if s == shape else (1, s)
                stage = 1 if run >= need else 0
            elif stage == 1 and op.kind == kind and s == shape:
                pass
            elif stage == 1 and op.kind == "lattice_plan" and s[0] != shape[0]:
                stage = 2
            elif stage == 2 and op.kind == "kmpc_plan":
                stage = 3
            elif stage == 3 and op.kind == kind and s == shape:
                return True
        return False

    assert chain("lattice_plan", True, 3)
    assert chain("lattice_step", False, 2)


@pytest.mark.parametrize("seed", ss.SEEDS)
def test_pattern_j_interleaved_warm_chains_change_shape_and_return(seed):
    ops = SCRIPTS[seed]
    four = ("kmpc_plan", "kmpc_qp_plan", "stmpc_plan", "stmpc_qp_plan")
    seq = [op for op in ops if op.kind in four]
    rounds = sum(1 for k in range(len(seq) - 3) if tuple(o.kind for o in seq[k:k + 4]) == four)
    assert rounds >= 6
    for kind in four:
        shapes = [(op.kw["E"], op.kw["T"]) for n, op in enumerate(seq) if op.kind == kind
                  and tuple(o.kind for o in seq[n - four.index(kind):n - four.index(kind) + 4]) == four]
        by_E = any(x == y and z[0] != y[0] and w == y for x, y, z, w in zip(shapes, shapes[1:], shapes[2:], shapes[3:]))
        by_T = any(z[1] != y[1] and z[0] == y[0] and w == y for y, z, w in zip(shapes, shapes[1:], shapes[2:]))
        assert by_E and by_T, kind


# ---- the witness's set-up ---------------------------------------------------------------------------------------------------------
def test_reads_table_matches_the_hand_written_one():
    assert set(ss.READS) == set(TABLE)
    for kind in TABLE:
        assert set(ss.READS[kind]) == TABLE[kind], kind
    assert list(MUTATORS) + list(RESETS) != [] and set(MUTATORS) | set(RESETS) == set(MUTATOR_KINDS)


def test_witness_setup_names_exactly_the_mutators_the_query_reads():
    away = dict(set_waypoints=dict(line=1), set_tracks=dict(K=3), set_grid=dict(map=1), inflate_grid=dict(radius=0.1), set_footprint=dict(on=True),
                lattice_set_clearance=dict(r=1), lattice_set_mode=dict(mixed=2), lattice_set_pipeline=dict(chunks=2), lattice_set_split=dict(groups=2),
                lattice_set_order=dict(heavy_first=0), lattice_set_closed_loop=dict(on=True), pure_pursuit_set_form=dict(egos_per_wave=4),
                kmpc_set_mode=dict(mixed=False), stmpc_set_mode=dict(mixed=False), kmpc_set_groups=dict(groups=2), kmpc_set_yaw_fixup=dict(on=False),
                kmpc_qp_set_pack=dict(egos_per_wave=1), kmpc_set_collision=dict(on=True, n_sub=2), stmpc_set_collision=dict(on=True, n_sub=2, n_sub_k=2),
                kmpc_qp_set_avoid=dict(on=True, margin=0.05), kmpc_qp_set_walls=dict(on=True, n_samples=24),
                stmpc_qp_set_avoid=dict(on=True, margin=0.05), stmpc_qp_set_walls=dict(on=True, n_samples=24),
                lattice_set_obstacles=dict(E=5, M=3, line=1), kmpc_set_obstacles=dict(E=5, M=3, line=1), stmpc_set_obstacles=dict(E=5, M=3, line=1),
                rivals_set_groups=dict(E=5, n=3), rivals_set_course=dict(E=5, K=3))
    assert set(away) == set(MUTATORS)
    model = Model()
    for n, (kind, kw) in enumerate(away.items()):                   # (set_grid first among the grid's three: it drops the other two)
        model.apply(n, Op(kind, kw, seed=100 + n))
    canonical = ["set_waypoints", "set_tracks", "set_grid", "inflate_grid", "set_footprint"]
    for query, reads in TABLE.items():
        setup = model.setup_for(query)
        kinds = [m.kind for m in setup]
        assert set(kinds) == reads and len(kinds) == len(reads), query
        assert kinds == sorted(kinds, key=list(MUTATORS).index), query
        scene = [k for k in kinds if k in canonical]
        assert scene == [k for k in canonical if k in reads], query
        held = [k for k in kinds if k.endswith("_obstacles") or k.startswith("rivals_set")]
        assert kinds[len(kinds) - len(held):] == held, query               # held obstacles / groups / courses come last
        assert all(m.kw == away[m.kind] and m.seed == 100 + list(away).index(m.kind) for m in setup), query
    assert Model().setup_for("lattice_plan") == []                       # a fresh context needs nothing
    model.apply(99, Op("set_grid", dict(map=2)))                         # a new grid drops the inflation and the footprint
    assert {"inflate_grid", "set_footprint"}.isdisjoint(m.kind for m in model.setup_for("grid_occupied"))


# ---- the replay on fakes ------------------------------------------------------------------------------------------------------------
class FakeDriver(ss.Driver):
    """contexts that are dicts: a query returns a digest of exactly what it may depend on -- its arguments, the mutators it reads, the data
    handed over -- so an honest context passes and one that keeps anything else fails"""

    def __init__(self, stale_grid=False, python_error=False):
        self.stale_grid, self.python_error, self.made = stale_grid, python_error, 0

    def library_code(self, exc):
        return {ValueError: -1, RuntimeError: -4}.get(type(exc))

    def create(self):
        self.made += 1
        return dict(first=self.made == 1, now={k: (dict(v), 0) for k, v in MUTATORS.items()}, carried={}, lag=None, open=True)

    def close(self, ctx):
        assert ctx["open"]
        ctx["open"] = False

    def mutate(self, ctx, kind, kw, seed):
        if kind in RESETS:
            ctx["carried"].pop(kind[:-len("_reset")], None)
            return
        if kind == "set_grid":
            ctx["lag"] = ctx["now"]["set_grid"]
            ctx["now"]["inflate_grid"], ctx["now"]["set_footprint"] = (dict(MUTATORS["inflate_grid"]), 0), (dict(MUTATORS["set_footprint"]), 0)
        if kind == "lattice_set_closed_loop":                            # (re)arming forgets the previous path
            ctx["carried"].pop("closed_loop", None)
        ctx["now"][kind] = (dict(kw), seed if kw != MUTATORS[kind] else 0)

    def _slot(self, op):
        what = ss.CARRIES.get(op.kind)
        return None if what is None else (what, op.kw["E"], op.kw.get("T", op.kw.get("S")), op.kw.get("TK"))

    def carried(self, ctx, op):
        slot = self._slot(op)
        if slot is None or (slot[0] == "closed_loop" and op.kind != "lattice_step" and not ctx["now"]["lattice_set_closed_loop"][0]["on"]):
            return None
        return ctx["carried"].get(slot[0], {}).get(slot)

    def hand_over(self, ctx, op, carried):
        if carried is not None:
            ctx["carried"][self._slot(op)[0]] = {self._slot(op): carried}

    def inputs(self, op):
        return {}

    def query(self, ctx, op, inputs, carried):
        kw = op.kw
        if kw.get("bad"):
            raise ValueError("bad argument")
        for held, kinds in (("lattice_set_obstacles", ("lattice_plan", "lattice_step", "lattice_plan_tracks")),
                            ("kmpc_set_obstacles", ("kmpc_plan", "kmpc_shoot")), ("stmpc_set_obstacles", ("stmpc_plan", "stmpc_shoot"))):
            E = ctx["now"][held][0]["E"]
            if op.kind in kinds and E and E != kw["E"] and self.python_error:
                raise KeyError("a mistake of the driver's own, the same on both contexts")
            if op.kind in kinds and E and E != kw["E"]:
                raise RuntimeError(f"{held}: held for {E} egos, this call has {kw['E']}")
        reads = {k: v for k, v in ctx["now"].items() if k in TABLE[op.kind]}
        if self.stale_grid and ctx["first"] and op.kind == "grid_occupied":
            reads["set_grid"] = ctx["lag"]                               # the bug: the grid before the last set_grid
        slot = self._slot(op)
        mine = self.carried(ctx, op) if slot else None
        digest = zlib.crc32(repr((op.kind, sorted(kw.items()), op.seed, sorted(reads.items()), mine)).encode())
        writes = slot and (slot[0] != "closed_loop" or op.kind == "lattice_step" or ctx["now"]["lattice_set_closed_loop"][0]["on"])
        if writes:                                                       # the call leaves data for the next one of its shape (another shape drops it)
            ctx["carried"][slot[0]] = {slot: digest}
        return dict(out=np.array([digest], np.int64), nan=np.array([np.nan, 1.0]))


@pytest.mark.parametrize("seed", ss.SEEDS)
def test_replay_passes_on_an_honest_context_and_closes_every_witness(seed):
    driver, stats = FakeDriver(), {}
    ss.replay(SCRIPTS[seed], driver, seed=seed, stats=stats)
    assert stats["queries"] == sum(1 for op in SCRIPTS[seed] if is_query(op)) == driver.made - 1


@pytest.mark.parametrize("seed", ss.SEEDS)
def test_replay_reports_a_stale_grid_at_the_right_operation(seed):
    ops = SCRIPTS[seed]
    expected = next(n for n, op in enumerate(ops) if op.kind == "grid_occupied")
    assert any(op.kind == "set_grid" for op in ops[:expected])
    with pytest.raises(AssertionError) as err:
        ss.replay(ops, FakeDriver(stale_grid=True), seed=seed)
    msg = str(err.value)
    assert msg.startswith(f"seed {seed}, op {expected} grid_occupied ")
    assert "out: 1 of 1 entries differ" in msg and "set_grid@" in msg and "nan:" not in msg


def test_replay_does_not_take_a_python_error_for_the_librarys():
    seed = ss.SEEDS[0]
    expected = next(n for n, op in enumerate(SCRIPTS[seed]) if op.expect == "error")
    with pytest.raises(AssertionError) as err:
        ss.replay(SCRIPTS[seed], FakeDriver(python_error=True), seed=seed)
    assert str(err.value).startswith(f"seed {seed}, op {expected} ") and "expected the library's error -4" in str(err.value)


def test_library_code_tells_the_runtimes_rejections_from_other_errors():
    from f1tenth_planning_amd.runtime import core
    d = ss.Driver()

    def raised(fn):
        try:
            fn()
        except Exception as e:  # noqa: BLE001
            return d.library_code(e)

    assert raised(lambda: core._raise(-1, "m")) == -1 and raised(lambda: core._raise(-4, "m")) == -4
    assert raised(lambda: np.zeros(3).reshape(2, 2)) is None and raised(lambda: {}["k"]) is None
    assert raised(lambda: (_ for _ in ()).throw(core.F1PError(-4, "raised by the runtime's own Python"))) is None


@pytest.mark.parametrize("phase", "abcdefghij")
def test_script_notices_a_lost_pattern(phase, monkeypatch):
    """script()'s own assertion: a session whose phase was emptied is refused, and for that pattern"""
    monkeypatch.setattr(ss._Gen, "phase_" + phase, lambda self: self.scene(0))
    with pytest.raises(AssertionError, match=("pattern " + phase) if phase != "b" else "pattern b|reuse window"):
        ss.script(ss.SEEDS[0])


def test_differences_sees_values_shapes_dtypes_nans_and_errors():
    a = ("ok", dict(x=np.array([1.0, np.nan, -0.0]), i=np.arange(3, dtype=np.int32)))
    same = ("ok", dict(x=np.array([1.0, np.nan, -0.0]), i=np.arange(3, dtype=np.int32)))
    assert ss.differences("q", a, same) == []
    assert ss.differences("q", a, ("ok", dict(x=np.array([1.0, np.nan, 1e-300]), i=a[1]["i"])))[0].startswith("x: 1 of 3 entries differ, first at (2,)")
    assert ss.differences("q", a, ("ok", dict(x=np.array([1.0, 2.0, -0.0]), i=a[1]["i"])))                # a NaN against a number
    assert ss.differences("q", a, ("ok", dict(x=a[1]["x"], i=np.arange(3, dtype=np.int64))))              # dtype
    assert ss.differences("q", a, ("ok", dict(x=a[1]["x"].reshape(3, 1), i=a[1]["i"])))                   # shape
    assert ss.differences("q", a, ("ok", dict(x=a[1]["x"])))                                              # a missing output
    assert ss.differences("q", a, ("error", "ValueError", "m"))
    assert ss.differences("q", ("error", "ValueError", "m"), ("error", "ValueError", "m")) == []
    assert ss.differences("q", ("error", "ValueError", "m"), ("error", "ValueError", "n"))
    assert ss.differences("q", ("error", "ValueError", "m"), ("error", "RuntimeError", "m"))
    assert len(ss.EXEMPT) <= 2


# ---- the real driver's calls, without a GPU --------------------------------------------------------------------------------------------
class _Lib:
    def __getattr__(self, name):
        return lambda *a: 0


class SignatureContext:
    """binds every call to runtime.Context's method of that name and returns arrays of zeros in the shapes the replay needs"""

    def __init__(self):
        from f1tenth_planning_amd import runtime
        self._cls, self.lib, self.h, self.calls = runtime.Context, _Lib(), None, []

    def _check(self, rc):
        assert rc == 0

    def __getattr__(self, name):
        fn = getattr(self._cls, name)

        def call(*a, **kw):
            inspect.signature(fn).bind(self, *a, **kw)
            self.calls.append(name)
            if name.endswith("warm_get"):
                raise ss.rt.F1PError(-4, "no warm start of this shape is held")
            if name == "lattice_fetch_traj":
                return np.zeros((a[0], a[1], 4))
            if name == "lattice_closed_loop_prev":
                return None
            return None if name.startswith(("set_", "inflate")) or "_set_" in name or name.endswith("_reset") else dict(out=np.zeros(1))
        return call

    def close(self):
        pass


class DryDriver(ss.Driver):
    def create(self):
        return SignatureContext()


def test_real_driver_calls_bind_to_the_runtime_signatures():
    seed = ss.SEEDS[0]
    stats = {}
    ss.replay(SCRIPTS[seed], DryDriver(), seed=seed, check=False, stats=stats)
    assert stats["queries"] > 100
