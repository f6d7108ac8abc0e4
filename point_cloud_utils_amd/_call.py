"""What the feature modules share when they call the library: how inputs are told apart and resolved (_is_torch, _shape2, _dtype_name, _Dev),
the call helpers (_fn, _call, _plain, _take, _record), the timing flags, the integer kinds, the allocation of integer outputs and _Handle, the
base of the objects that own an index on the GPU. It imports _lib only; the feature modules import from here and from _checks, once, at their
top, and not from each other ("The Python layer")."""
import ctypes
import os

import numpy as np

from . import _lib
from ._lib import Stats

_FACE_KINDS = {"int32": 0, "int64": 1, "uint32": 2, "uint64": 3}     # PCU_HIP_FACE_*: faces, cubes, grid coordinates

_last_stats = [None]      # the Stats struct of the most recent call (turned into a dict on demand)
# PCU_HIP_NO_TIE_ORDER=1: skip the kd-tree tie-order resolver (exact ties then ordered by (d2, row)); for experiments.
_ENV_FLAGS = _lib.NO_TIE_ORDER if os.environ.get("PCU_HIP_NO_TIE_ORDER", "0") not in ("", "0") else 0
_TIMING = [int(os.environ.get("PCU_HIP_TIMING", "0") or 0)]      # the level of set_timing


def _flags():
    return _ENV_FLAGS | (_lib.TIME_KERNELS if _TIMING[0] >= 1 else 0) | (_lib.TIME_PHASES if _TIMING[0] >= 2 else 0)


def _is_torch(a):
    return type(a).__module__.startswith("torch") and hasattr(a, "data_ptr")


def _shape2(a):
    sh = tuple(a.shape)
    if len(sh) == 2:
        return sh
    if len(sh) == 1:            # numpyeigen maps a 1-D array to a column vector
        return (sh[0], 1)
    raise ValueError(f"Invalid number of dimensions ({len(sh)}): expected a matrix of shape (n, 3).")


_DT_FAST = {np.dtype("float32"): "float32", np.dtype("float64"): "float64"}


def _dtype_name(a):
    dt = getattr(a, "dtype", None)
    try:
        name = _DT_FAST.get(dt)            # the two supported dtypes, numpy or torch, without string work
    except TypeError:
        name = None
    if name is not None:
        return name
    if _is_torch(a):
        name = str(a.dtype).replace("torch.", "")
        if name in ("float32", "float64"):
            _DT_FAST[a.dtype] = name
        return name
    return np.asarray(a).dtype.name


class _Dev:
    """Resolved inputs of one call: contiguous buffers, pointers, device, stream, flags."""

    def __init__(self, a, b):
        self.torch = _is_torch(a) or _is_torch(b)
        if self.torch:
            import torch
            if not (_is_torch(a) and _is_torch(b)) or not (a.is_cuda and b.is_cuda) or a.device != b.device:
                raise ValueError("torch inputs must both be CUDA/HIP tensors on the same device")
            self.a, self.b = a.contiguous(), b.contiguous()
            self.device = a.device.index if a.device.index is not None else torch.cuda.current_device()
            self.tdev = a.device
            # the library launches on torch's current stream, so its kernels are ordered after the producers of the input
            # tensors (torch's default stream is the legacy NULL stream, handle 0: STREAM_GIVEN makes NULL mean exactly that)
            raw = getattr(torch._C, "_cuda_getCurrentRawStream", None)       # (the handle without building a Stream object: ~2 us per call)
            self.stream = raw(self.device) if raw is not None else torch.cuda.current_stream(a.device).cuda_stream
            self.flags = _lib.PTRS_ON_DEVICE | _flags() | _lib.STREAM_GIVEN
            self.pa, self.pb = self.a.data_ptr(), self.b.data_ptr()
            self.np_dtype = np.float32 if a.dtype == torch.float32 else np.float64
            self.t_dtype = a.dtype
        else:
            self.a, self.b = np.ascontiguousarray(a), np.ascontiguousarray(b)
            self.device = _lib.default_device()
            self.stream = None
            self.flags = _flags()
            self.pa, self.pb = self.a.ctypes.data, self.b.ctypes.data
            self.np_dtype = self.a.dtype.type
        self.suffix = "f32" if self.np_dtype == np.float32 else "f64"
        self.ctx = _lib.ctx(self.device)

    def empty(self, shape, kind):
        """kind: 'T' (input dtype) or 'i64'."""
        if self.torch:
            import torch
            return torch.empty(shape, dtype=self.t_dtype if kind == "T" else torch.int64, device=self.tdev)
        return np.empty(shape, dtype=self.np_dtype if kind == "T" else np.int64)

    @staticmethod
    def ptr(x):
        if x is None:
            return None
        return x.data_ptr() if _is_torch(x) else x.ctypes.data


def _record(st):
    _last_stats[0] = st


_FN = {}


def _fn(op, suffix):
    """Entry point `pcu_hip_<op>_<suffix>` (looked up once)."""
    f = _FN.get((op, suffix))
    if f is None:
        f = _FN[(op, suffix)] = getattr(_lib.lib(), f"pcu_hip_{op}_{suffix}")
    return f


def _call(name, d, *args, suffix=True):
    """The library's `name` for the arrays `d` resolved (with their scalar suffix, or the one entry point that has none): raises what it
    refuses, records its statistics."""
    st = Stats()
    fn = _fn(name, d.suffix) if suffix else getattr(_lib.lib(), "pcu_hip_" + name)
    rc = fn(d.ctx, *args, d.flags, d.stream, ctypes.addressof(st))
    if rc:
        _lib.check(rc)
    _record(st)


def _plain(name, *args):
    """An entry point without a scalar suffix and without statistics."""
    rc = getattr(_lib.lib(), "pcu_hip_" + name)(*args)
    if rc:
        _lib.check(rc)


def _int_out(d, shape, np_dtype):
    """An uninitialised array of a numpy dtype beside the inputs `d` resolved: a tensor on their device, or numpy."""
    if d.torch:
        import torch
        return torch.empty(shape, dtype=getattr(torch, np.dtype(np_dtype).name), device=d.tdev)
    return np.empty(shape, dtype=np_dtype)


def _take(name, d, shapes_and_dtypes, *counts):
    """The second half of a call whose result the library parked (its size came back from the first half): allocates the two outputs beside
    the inputs and calls `<name>_take` with the counts the first half returned. shapes_and_dtypes: (shape, numpy dtype) per output."""
    outs = [_int_out(d, shape, dt) for shape, dt in shapes_and_dtypes]
    _plain(name + "_take", d.ctx, *counts, *[_Dev.ptr(o) for o in outs], d.flags, d.stream)
    return outs


class _Handle:
    """An index the library keeps on the GPU for its owner: made by _open, freed by the entry point `_destroy` on close(), at the end of a
    `with` block or with the object. A subclass states `_destroy` and its `_noun` for the two refusals."""
    _noun = _destroy = None
    _h = None

    def _open(self, name, d, *args, flags=None):
        """The create call `name` for the arrays `d` resolved; the handle's device is theirs."""
        h = ctypes.c_void_p()
        rc = _fn(name, d.suffix)(d.ctx, *args, d.flags if flags is None else flags, d.stream, ctypes.byref(h))
        if rc:
            _lib.check(rc)
        self._h, self._device = h, d.device

    def _check_open(self):
        if self._h is None:
            raise ValueError(f"the {self._noun} has been closed")

    def _same_device(self, d, what):
        if d.device != self._device:
            raise ValueError(f"{what} and {self._noun} live on different devices")

    def close(self):
        h, self._h = self._h, None
        if isinstance(h, ctypes.c_void_p):       # what _open made; anything else (a stand-in) is dropped, never handed to the library as a pointer
            getattr(_lib.lib(), self._destroy)(h)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
