"""What the feature modules share when they call the library: the call helpers, the integer kinds and the allocation of integer outputs.
Feature modules import these from here, not from each other."""
import ctypes

import numpy as np

_FACE_KINDS = {"int32": 0, "int64": 1, "uint32": 2, "uint64": 3}     # PCU_HIP_FACE_*: faces, cubes, grid coordinates


def _call(name, d, *args, suffix=True):
    """The library's `name` for the arrays `d` resolved (with their scalar suffix, or the one entry point that has none): raises what it
    refuses, records its statistics."""
    from . import _lib, _fn, _record, Stats
    st = Stats()
    fn = _fn(name, d.suffix) if suffix else getattr(_lib.lib(), "pcu_hip_" + name)
    rc = fn(d.ctx, *args, d.flags, d.stream, ctypes.addressof(st))
    if rc:
        _lib.check(rc)
    _record(st)


def _plain(name, *args):
    """An entry point without a scalar suffix and without statistics."""
    from . import _lib
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
    from . import _Dev
    outs = [_int_out(d, shape, dt) for shape, dt in shapes_and_dtypes]
    _plain(name + "_take", d.ctx, *counts, *[_Dev.ptr(o) for o in outs], d.flags, d.stream)
    return outs
