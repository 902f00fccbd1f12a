"""Track sets without a GPU: the C-ABI declares and exports the track-set entry points, and the classes check their track
arguments before anything touches a device."""
import os
import re

import numpy as np
import pytest

from f1tenth_planning_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("f1p_set_track_set", "f1p_nearest_point_tracks_batch", "f1p_pure_pursuit_tracks_batch", "f1p_pure_pursuit_tracks_dev",
         "f1p_stanley_tracks_batch", "f1p_lqr_tracks_batch", "f1p_kmpc_ref_tracks_batch", "f1p_kmpc_ref_tracks_dev")


def test_header_declares_the_track_set_abi():
    hdr = open(os.path.join(ROOT, "include", "f1p.h")).read()
    for n in NAMES:
        assert re.search(r"\b" + n + r"\s*\(", hdr), n
        assert n in _abi.PROTOTYPES, n
    m = re.search(r"#define F1P_ST_BAD_TRACK (\d+)", hdr)
    assert m and int(m.group(1)) == _abi.ST_BAD_TRACK == _abi.ST_ALL_BLOCKED + 1


def test_library_exports_the_track_set_abi():
    if not os.path.exists(_abi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _abi.load_library()
    for n in NAMES:
        assert hasattr(lib, n), n


def test_class_track_arguments_are_checked_first():
    from f1tenth_planning_amd.control.lqr.lqr import LQRPlanner
    from f1tenth_planning_amd.control.pure_pursuit.pure_pursuit import PurePursuitPlanner
    from f1tenth_planning_amd.control.stanley.stanley import StanleyPlanner
    t = np.zeros((10, 4))
    with pytest.raises(ValueError):
        PurePursuitPlanner().plan_batch(np.zeros((2, 3)), 0.8, tracks=[t])                # no track_ids
    with pytest.raises(ValueError):
        PurePursuitPlanner().plan_batch(np.zeros((2, 3)), 0.8, tracks=[], track_ids=[])   # no track
    with pytest.raises(ValueError):
        StanleyPlanner().plan_batch(np.zeros((2, 4)), tracks=[t[:, :3]], track_ids=[0, 0])  # Stanley needs a heading column
    with pytest.raises(ValueError):
        LQRPlanner().plan_batch(np.zeros((2, 4)), tracks=[t], track_ids=[0, 0])           # LQR needs a curvature column
