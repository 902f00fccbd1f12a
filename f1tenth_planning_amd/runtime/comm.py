"""Context's multi-GPU exchange step: the RCCL communicator and the cross-rank argmin (csrc/f1p_comm.hip)."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np

from .. import _abi
from .core import _f64, _ptr


@contextlib.contextmanager
def _stdout_to_stderr():
    """RCCL prints a version banner to the C stdout when a communicator is created (flushed at process exit, i.e. AFTER a
    caller's own output -- bench.py must print exactly one JSON line): send fd 1 to stderr for the duration of the call."""
    libc = C.CDLL(None)
    sys.stdout.flush(); libc.fflush(None)
    saved = os.dup(1)
    os.dup2(2, 1)
    try:
        yield
    finally:
        sys.stdout.flush(); libc.fflush(None)
        os.dup2(saved, 1)
        os.close(saved)


class _Comm:
    # ---- multi-GPU exchange step -----------------------------------------------------------------------------
    def comm_unique_id(self):
        buf = (C.c_uint8 * _abi.COMM_ID_BYTES)()
        with _stdout_to_stderr():
            rc = self.lib.f1p_comm_unique_id(self.h, buf)
        self._check(rc)
        return bytes(buf)

    def comm_init(self, uid, nranks, rank):
        buf = (C.c_uint8 * _abi.COMM_ID_BYTES).from_buffer_copy(uid)
        with _stdout_to_stderr():
            rc = self.lib.f1p_comm_init(self.h, buf, int(nranks), int(rank))
        self._check(rc)

    def comm_info(self):
        """(nranks, rank) as the RCCL communicator reports them."""
        n = C.c_int32(); r = C.c_int32()
        self._check(self.lib.f1p_comm_info(self.h, C.byref(n), C.byref(r)))
        return n.value, r.value

    def comm_set_exchange(self, mode=0):
        """form of the cross-rank argmin: 0 = two RCCL all-reduces (default), 1 = one all-gather of (key, index) + a local minimum"""
        self._check(self.lib.f1p_comm_set_exchange(self.h, int(mode)))

    def argmin_gather_reduce(self, cost, idx):
        """the local kernels of exchange form 1 on N emulated ranks: cost / idx [N, E] -> (idx [E], cost [E])"""
        cost = _f64(cost); idx = np.ascontiguousarray(idx, np.int32)
        N, E = cost.shape
        io = np.empty(E, np.int32); co = np.empty(E)
        self._check(self.lib.f1p_argmin_gather_reduce_batch(self.h, _ptr(cost), _ptr(idx), N, E, _ptr(io), _ptr(co)))
        return io, co

    def comm_argmin_dev(self, d_cost, d_idx, E):
        self._check(self.lib.f1p_comm_argmin_dev(self.h, d_cost.ptr, d_idx.ptr, int(E)))

    def argmin_key(self, cost):
        """the cost -> u64 key map of the cross-rank argmin (np.argmin order, NaN first)"""
        cost = _f64(cost).reshape(-1); E = cost.shape[0]
        keys = np.empty(E, np.uint64)
        self._check(self.lib.f1p_argmin_key_batch(self.h, _ptr(cost), E, _ptr(keys)))
        return keys

    def argmin_mask(self, own_keys, min_keys, idx):
        own = np.ascontiguousarray(own_keys, np.uint64); mn = np.ascontiguousarray(min_keys, np.uint64)
        idx = np.ascontiguousarray(idx, np.int32); E = own.shape[0]
        masked = np.empty(E, np.int32); cost = np.empty(E)
        self._check(self.lib.f1p_argmin_mask_batch(self.h, _ptr(own), _ptr(mn), _ptr(idx), E, _ptr(masked), _ptr(cost)))
        return masked, cost
