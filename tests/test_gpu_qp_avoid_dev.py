"""f1p_kmpc_qp_avoid_dev and f1p_stmpc_qp_avoid_dev, the avoidance QPs on device buffers: every output, the three avoidance outputs included,
bit for bit what the tested *_batch entry points return for the same egos (the four share one body, csrc/f1p_host.h qp_call).  Shapes: the
smallest that reach each kernel instantiation and the row edge cases -- kinematic E = 3 at T = 3 (two egos per wave, the last wave half
filled) and T = 16 (one ego per wave), dynamic E = 2 at T = 2 (rate rows for tau = 0 only); M = 2: one live disc beside the path, one empty
slot."""
import ctypes as C

import numpy as np
import pytest

import kmpc_qp_avoid_scenes as KSC
import stmpc_qp_avoid_scenes as SSC
from f1tenth_planning_amd import _abi
from f1tenth_planning_amd.runtime import Context, kmpc_qp_avoid, stmpc_qp_avoid

pytestmark = pytest.mark.gpu

M = 2
KW = dict(want_duals=True, want_planes=True, want_avoid_duals=True)


@pytest.fixture(scope="module")
def ctx():
    with Context(0) as c:
        yield c


def _kinematic(ctx, T):
    x0, ref, oa, od, obs, fam = KSC.exact_scene(T, M)
    sel = [fam["inactive"][0], fam["active"][0], fam["inside"][0]]           # a disc in slot 0 (far, then touching), a disc in slot 1
    batch = kmpc_qp_avoid(ctx, x0[sel], ref[sel], obs[sel], _abi.kmpc_cfg(horizon=T), oa_prev=oa[sel], od_prev=od[sel], want_xk=True, **KW)
    return ctx.lib.f1p_kmpc_qp_avoid_dev, _abi.kmpc_cfg(horizon=T), "xk", (x0[sel], ref[sel], oa[sel], od[sel], obs[sel]), batch


def _dynamic(ctx, T):
    x0, ref, oa, odv, obs, fam = SSC.exact_scene(T, M)
    sel = [fam["inactive"][0], fam["inside"][0]]                             # a disc in slot 0, a disc in slot 1
    batch = stmpc_qp_avoid(ctx, x0[sel], ref[sel], obs[sel], _abi.stmpc_cfg(horizon=T), oa_prev=oa[sel], od_v_prev=odv[sel], want_x=True, **KW)
    return ctx.lib.f1p_stmpc_qp_avoid_dev, _abi.stmpc_cfg(horizon=T), "x", (x0[sel], ref[sel], oa[sel], odv[sel], obs[sel]), batch


@pytest.mark.parametrize("model,T", [(_kinematic, 3), (_kinematic, 16), (_dynamic, 2)])
def test_avoid_dev_equals_batch_bit_for_bit(ctx, model, T):
    fn, cfg, xname, inputs, batch = model(ctx, T)
    obs = inputs[4]
    E = len(obs)
    assert ((obs[:, :, 4] >= 0).sum(axis=1) == 1).all()                       # one live disc, one empty slot per ego
    assert np.isin(batch["status"], (0, 2)).all() and (batch["planes"][:, :, 0, 3] >= 0).all() and (batch["planes"][:, :, 1, 3] == -1).all()
    keys = ("steer", "speed", "status", "u", xname, "obj", "duals", "iters", "eps", "planes", "avoid_duals")      # the C signature's order
    d_in = [ctx.to_device(a) for a in inputs]
    d_out = {k: ctx.alloc(batch[k].nbytes) for k in keys}
    try:
        ctx._check(fn(ctx.h, *(d.ptr for d in d_in[:4]), E, C.byref(cfg), None, d_in[4].ptr, M, None, *(d_out[k].ptr for k in keys)))
        for k in keys:
            got = d_out[k].download(batch[k].dtype, batch[k].shape)
            assert got.tobytes() == batch[k].tobytes(), k
    finally:
        for d in d_in + list(d_out.values()):
            d.free()
