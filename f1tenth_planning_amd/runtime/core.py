"""The runtime's core: error mapping, the pointer helpers every wrapper uses, DeviceBuffer, and the context's housekeeping -- creation and
destruction, page-locked and device memory, the timer (csrc/f1p_core.hip)."""
import ctypes as C

import numpy as np

from .. import _abi


class F1PError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libf1p error {code}: {msg}")
        self.code = code


def _raise(code, msg):
    if code == _abi.F1P_EINVAL:
        raise ValueError(msg)
    raise F1PError(code, msg)


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None:
        a = a.reshape(shape)
    return a


def _ptr(a):
    # (`a.ctypes.data` builds a ctypes helper object per call: 2.3 us; the array interface's address is 1.5 us -- nine of them per plan() call)
    return None if a is None else C.c_void_p(a.__array_interface__["data"][0])


def _dev(b):
    """the device pointer of an optional DeviceBuffer"""
    return None if b is None else b.ptr


def _ref(s):
    """an optional ctypes struct by reference"""
    return None if s is None else C.byref(s)


def _cut(a, lo, hi):
    """rows [lo, hi) of an optional array"""
    return None if a is None else a[lo:hi]


def _tid(track_ids):
    """what a *_tracks wrapper hands to the body it shares with the raceline form, where None means the raceline: the ids as an array"""
    return np.ascontiguousarray(track_ids, dtype=np.int32).reshape(-1)


def _pick(plain, tracks, ids):
    """A raceline / track-set pair of C entry points and the optional track ids -> (the function to call, the id pointer as the
    arguments to splice in: none for the raceline form)"""
    return (plain, ()) if ids is None else (tracks, (_ptr(ids),))


class DeviceBuffer:
    """A caller-visible HBM buffer (f1p_dev_alloc) for the *_dev entry points."""

    def __init__(self, ctx, nbytes):
        self.ctx = ctx
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        ctx._check(ctx.lib.f1p_dev_alloc(ctx.h, C.byref(p), C.c_size_t(self.nbytes)))
        self.ptr = p

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        self.ctx._check(self.ctx.lib.f1p_h2d(self.ctx.h, self.ptr, C.c_void_p(arr.ctypes.data), C.c_size_t(arr.nbytes)))
        self.ctx.sync()   # the host array may die right after the call
        return self

    def download(self, dtype, shape):
        out = np.empty(shape, dtype=dtype)
        assert out.nbytes <= self.nbytes
        self.ctx._check(self.ctx.lib.f1p_d2h(self.ctx.h, C.c_void_p(out.ctypes.data), self.ptr, C.c_size_t(out.nbytes)))
        self.ctx.sync()
        return out

    def free(self):
        if self.ptr is not None and self.ctx.h is not None:
            self.ctx.lib.f1p_dev_free(self.ctx.h, self.ptr)
        self.ptr = None


class _Core:
    def __init__(self, device=0):
        self.lib = _abi.load_library()
        h = C.c_void_p()
        rc = self.lib.f1p_create(C.byref(h), int(device))
        if rc != _abi.F1P_OK:
            msg = self.lib.f1p_last_error(None).decode()
            raise F1PError(rc, msg + " -- the HIP path is mandatory, there is no CPU fallback")
        self.h = h
        self.device = int(device)
        self.n_waypoints = 0
        self._wp_key = None
        self.n_tracks = 0
        self._tracks_key = None
        self.has_grid = False
        self._pinned = {}        # (tag, shape, dtype) -> numpy view of page-locked memory
        self._pinned_ptrs = []
        self._bundles = {}       # per batch shape: the page-locked arrays of lattice_plan(reuse_outputs=True) / lattice_step and their addresses

    # ---- housekeeping ------------------------------------------------------------------------------
    def _check(self, rc):
        if rc != _abi.F1P_OK:
            _raise(rc, self.lib.f1p_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None) is not None:
            for ptr in self._pinned_ptrs:
                self.lib.f1p_host_free(self.h, ptr)
            self._pinned_ptrs = []
            self._pinned = {}
            self._bundles = {}
            self.lib.f1p_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def sync(self):
        self._check(self.lib.f1p_sync(self.h))

    def device_info(self):
        name = C.create_string_buffer(256); arch = C.create_string_buffer(256); cu = C.c_int32()
        self._check(self.lib.f1p_device_info(self.h, name, 256, C.byref(cu), arch, 256))
        return dict(name=name.value.decode(), compute_units=cu.value, arch=arch.value.decode())

    def alloc(self, nbytes):
        return DeviceBuffer(self, nbytes)

    def pinned(self, tag, shape, dtype):
        """numpy array on page-locked host memory (f1p_host_alloc), cached per (tag, shape, dtype) and owned by the
        context: valid until close().  The *_batch calls DMA directly from / into such arrays."""
        dtype = np.dtype(dtype)
        shape = tuple(int(v) for v in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        key = (tag, shape, dtype.str)
        arr = self._pinned.get(key)
        if arr is None:
            nbytes = max(int(np.prod(shape)) * dtype.itemsize, 1)
            ptr = C.c_void_p()
            self._check(self.lib.f1p_host_alloc(self.h, C.byref(ptr), C.c_size_t(nbytes)))
            self._pinned_ptrs.append(ptr)
            buf = (C.c_char * nbytes).from_address(ptr.value)
            arr = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)
            self._pinned[key] = arr
        return arr

    def to_device(self, arr):
        arr = np.ascontiguousarray(arr)
        return DeviceBuffer(self, max(arr.nbytes, 1)).upload(arr)

    def timer_begin(self):
        self._check(self.lib.f1p_timer_begin(self.h))

    def timer_end(self):
        ms = C.c_float()
        self._check(self.lib.f1p_timer_end(self.h, C.byref(ms)))
        return ms.value

    @staticmethod
    def _ids(track_ids, E):
        """track ids as int32 [E]: ego e follows track track_ids[e] of set_tracks"""
        ids = np.ascontiguousarray(track_ids, dtype=np.int32).reshape(-1)
        if ids.shape[0] != E:
            raise ValueError(f"track_ids must hold one id per ego ({E}), not {ids.shape[0]}")
        return ids
