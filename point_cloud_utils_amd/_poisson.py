"""downsample_point_cloud_poisson_disk: the reference's binding (src/sample_point_cloud.cpp:253-333) over the HIP greedy of
csrc/poisson.h. Same arguments, defaults, error texts and return type; the sample set follows this library's deterministic contract
("Poisson-disk downsampling") instead of libigl's random one."""
import ctypes
import time

import numpy as np

from ._call import _Dev, _call, _dtype_name, _int_out
from ._checks import _check_finite


def downsample_point_cloud_poisson_disk(v, radius, target_num_samples=-1, random_seed=0, sample_num_tolerance=0.04):
    """
    Downsample a point set so that samples are approximately evenly spaced.

    Args:
        v: #v by 3 array of vertex positions (float32 or float64; numpy, or a CUDA/HIP torch tensor)
        radius: desired separation between points: no two samples are closer than radius, and every row of v lies closer than
                radius to some sample.
        target_num_samples: If set to a positive value, iterate to generate points as close to this target as possible (determined by
                            sample_num_tolerance), with the reference's radius search.
        random_seed: A random seed used to generate the samples. Passing in 0 will use the current time. (0 by default).
        sample_num_tolerance: If you requested a target number of samples, by passsing num_samples > 0, then this function will return
                              between (1 - sample_num_tolerance) * num_samples and (1 + sample_num_tolerance) * num_samples (if the
                              search converges within its 20 bisection steps). (0.04 by default).

    Returns:
        p_idx : A (m,) shaped int32 array of indices into v where m is the number of Poisson-disk samples (ascending). The samples are
                the rows the serial greedy takes when it visits the rows in an order drawn from random_seed; equal arguments give equal
                results.
    """
    dn = _dtype_name(v)
    if dn not in ("float32", "float64"):
        raise ValueError(f"Invalid scalar type ({dn}) for argument 'v'. Expected one of ['float32', 'float64'].")
    if len(v.shape) != 2 or int(v.shape[1]) != 3:
        sh = tuple(v.shape) + (1,) * (2 - len(v.shape))
        raise ValueError(f"Only 3D inputs are supported: v must have shape (n, 3) (n > 0). Got v.shape = ({sh[0]}, {sh[1]}).")
    target_num_samples = int(target_num_samples)
    radius = float(radius)
    if target_num_samples <= 0 and radius <= 0.0:
        raise ValueError("Cannot have both num_samples <= 0 and radius <= 0")
    tol = float(np.float32(sample_num_tolerance))          # (a float argument in the reference)
    if tol > 1.0 or tol <= 0.0 or tol != tol:
        raise ValueError("sample_num_tolerance must be in (0, 1]")
    if target_num_samples <= 0 and radius != radius:
        raise ValueError("radius must not be NaN")
    n = int(v.shape[0])
    if n == 0:
        raise ValueError("Invalid point set with zero elements: v must have shape (n, 3) with n > 0. Got v.shape = (0, 3).")
    # The reference has no stable behaviour for non-finite coordinates (README.md): refused before any work on the device.
    _check_finite(v, "v must not contain NaN or infinite coordinates")
    seed = int(random_seed)
    if seed < 0 or seed > 0xFFFFFFFF:
        raise ValueError(f"random_seed must be an unsigned 32-bit integer, got {seed}")
    if seed == 0:                                          # the reference's documented behaviour: a seed from the clock
        seed = (time.time_ns() & 0xFFFFFFFF) or 1
    d = _Dev(v, v)
    out = _int_out(d, (n,), np.int32)
    cnt = ctypes.c_int64(0)
    _call("poisson_disk", d, d.pa, n, radius, target_num_samples, seed, tol, _Dev.ptr(out), ctypes.byref(cnt))
    return out[:int(cnt.value)]
