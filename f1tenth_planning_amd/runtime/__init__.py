"""Host-side runtime above the C-ABI (include/f1p.h): one `Context` per GPU.

Plumbing only -- numpy arrays in and out, ctypes calls into libf1p.so; no planning arithmetic happens in
Python.  There is no CPU fallback: constructing a Context without the HIP library or without a GPU raises.
"""
import os
import zlib

import numpy as np

from .._abi import F1PLibraryError, KmpcCfg, LatticeCfg  # noqa: F401

try:                      # xxh3 over the bytes: 6 us for a 1692 x 5 raceline
    import xxhash as _xxhash
except ImportError:       # numpy-only twin below (24 us)
    _xxhash = None

# (the fingerprint lives here, above the imports of the modules that use it: tests switch `runtime._xxhash` off to reach the numpy twin)
_SIG_WEIGHTS = {}


def _sig_weights(n):
    w = _SIG_WEIGHTS.get(n)
    if w is None:
        i = np.arange(1, n + 1, dtype=np.uint64)
        w = i * np.uint64(0x9E3779B97F4A7C15)
        w ^= w >> np.uint64(29)
        w |= np.uint64(1)
        _SIG_WEIGHTS[n] = w
    return w


def _content_signature(a):
    """Cheap ORDER-SENSITIVE fingerprint of an array's CONTENT for change detection on every plan() call (the reference keeps a
    live reference to the caller's waypoints, so in-place edits -- a reversed raceline, swapped columns, a mirrored track -- must
    be seen).  xxh3-64 of the bytes when xxhash is importable; otherwise a dot product of the 64-bit words, each folded with its
    own high half (so sign-bit flips do not cancel pairwise), with position-dependent odd weights, plus the XOR of the words.
    (Round 2's XOR + plain sum was invariant under permutations and under an even number of sign flips: ADVICE r2.)"""
    a = np.ascontiguousarray(a)
    if _xxhash is not None:
        return _xxhash.xxh3_64_intdigest(a.reshape(-1).view(np.uint8))
    if a.dtype.itemsize == 8 and a.size:
        w = a.reshape(-1).view(np.uint64)
        v = w ^ (w >> np.uint64(31))
        return (int(np.bitwise_xor.reduce(w)), int(np.dot(v, _sig_weights(w.size))))
    return zlib.crc32(a.view(np.uint8).reshape(-1))


from .core import DeviceBuffer, F1PError, _Core, _f64, _ptr  # noqa: E402, F401
from .comm import _Comm  # noqa: E402
from .lattice import _Lattice, lattice_set_obstacles, lattice_set_obstacles_dev  # noqa: E402, F401
from .mpc import (_Mpc, kmpc_qp_avoid, kmpc_qp_set_avoid, kmpc_qp_set_walls, kmpc_qp_walls, kmpc_set_obstacles,  # noqa: E402, F401
                  kmpc_set_obstacles_dev, stmpc_qp_avoid, stmpc_qp_set_avoid, stmpc_qp_set_walls, stmpc_qp_walls, stmpc_set_obstacles,
                  stmpc_set_obstacles_dev)
from .rivals import _Rivals, rivals, rivals_dev, rivals_predict, rivals_predict_dev, rivals_set_course, rivals_set_groups  # noqa: E402, F401
from .scene import _Scene  # noqa: E402
from .trackers import _Trackers  # noqa: E402


class Context(_Core, _Scene, _Trackers, _Lattice, _Mpc, _Rivals, _Comm):
    """One f1p_ctx: one device, one HIP stream.  Not thread-safe; use one Context per thread / rank."""


from .multi import MultiContext  # noqa: E402, F401  (needs Context)

_default_ctx = None


def default_context():
    """Process-wide Context on LOCAL_RANK (or device 0) used by the drop-in planner classes."""
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(int(os.environ.get("LOCAL_RANK", "0")))
    return _default_ctx
