"""The Python runtime pinned call by call, on the CPU: tools/record_runtime_calls.py drives every public Context / MultiContext wrapper
and the planner classes' GPU-free rejections on a stub library and records what reaches the C-ABI (function, per-argument kind), what
comes back (keys, dtypes, shapes), the public signatures, and the exceptions' types and texts.  tests/golden/runtime_calls.json is that
record taken at the commit before the runtime was folded and split; the working tree must reproduce it exactly."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def records():
    spec = importlib.util.spec_from_file_location("record_runtime_calls", os.path.join(ROOT, "tools", "record_runtime_calls.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with open(os.path.join(ROOT, "tests", "golden", "runtime_calls.json")) as fh:
        return tool.record(), json.load(fh)


def _compare(got, want, key):
    assert [key(e) for e in got] == [key(e) for e in want]          # the same cases in the same order
    for g, w in zip(got, want):
        assert g == w, key(w)


@pytest.mark.parametrize("section", ["context", "multi"])
def test_runtime_calls_match_the_recorded_ones(records, section):
    got, want = records
    assert len(want[section]) > 30
    _compare(got[section], want[section], lambda e: e["call"])


def test_public_signatures_match_the_recorded_ones(records):
    got, want = records
    assert [e["class"] for e in want["signatures"]] == ["Context", "MultiContext", "PurePursuitPlanner", "StanleyPlanner", "LQRPlanner",
                                                        "LatticePlanner", "KMPCPlanner", "STMPCPlanner"]
    _compare(got["signatures"], want["signatures"], lambda e: e["class"])


def test_planner_rejections_match_the_recorded_ones(records):
    got, want = records
    assert sum("raises" in e for e in want["planners"]) > 60
    _compare(got["planners"], want["planners"], lambda e: (e["class"], e["case"]))
