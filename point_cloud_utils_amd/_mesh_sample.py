"""mesh_face_areas, sample_mesh_random and sample_mesh_poisson_disk: the reference's bindings (src/face_areas.cpp:17-79,
src/sample_mesh.cpp:34-115) over the HIP kernels of csrc/mesh_sample.h and the Poisson-disk greedy of csrc/poisson.h. Same arguments, defaults,
order of checks, error texts and return order; the sample sets follow this library's deterministic contract instead of
libigl's rand()-driven ones."""
import ctypes
import math

import numpy as np

from . import _lib
from ._call import Stats, _Dev, _call, _fn, _record
from ._checks import _MAX_ROWS, _check_mesh, _check_rows, _check_seed as _seed, _face_rows, _mesh_args, _resolve


def mesh_face_areas(v, f, num_threads=-1):
    """
    Compute the areas of each face of a triangle mesh

    Args:
        v : #v by 3 array of vertex positions (each row is a vertex; float32 or float64; numpy, or a CUDA/HIP torch tensor)
        f : #f by 3 Matrix of face (triangle) indices (int32, int64, uint32 or uint64; int32 / int64 for torch)
        num_threads : OpenMP knob of the reference; accepted and ignored.

    Returns:
        areas : an array of shape (#faces,) where areas[i] is the area of the face f[i], in v's dtype

    Notes:
        Heron's formula as the reference evaluates it, in v's dtype, every operation rounded on its own (no FMA): with a, b, c the edge lengths
        and p = 0.5 * ((a + b) + c), areas[i] = sqrt(((p * max(p - a, 0)) * max(p - b, 0)) * max(p - c, 0)). A face [i j j] has area exactly
        0; where a square overflows the result is what IEEE arithmetic gives (inf, or NaN). Non-finite coordinates, face indices outside
        [0, #v) and arrays of more than 2**27 - 16 rows raise ValueError.
    """
    _check_mesh(v, f)
    d, ff, nv, nf = _resolve(v, f)
    areas = d.empty((nf,), "T")
    _call("mesh_face_areas", d, *_mesh_args(d, ff, nv, nf), _Dev.ptr(areas))
    return areas.reshape(()) if nf == 1 else areas


def sample_mesh_random(v, f, num_samples, random_seed=0):
    """
    Generate uniformly distributed random point samples on a mesh

    Args:
        v : (#v, 3)-shaped array of mesh vertex positions (float32 or float64; numpy, or a CUDA/HIP torch tensor)
        f : (#f, 3)-shaped array of mesh face indices (int32, int64, uint32 or uint64; int32 / int64 for torch)
        num_samples : The number of samples to generate
        random_seed : A random seed used to generate the samples. Passing in 0 will use the current time. (0 by default).

    Returns:
        f_idx : (num_samples,) shaped array of face indices into f (f's dtype)
        bc : (num_samples, 3) shaped array of barycentric coordinates (v's dtype)

    Notes:
        The samples follow a deterministic contract instead of libigl's rand(): a face is drawn with probability
        proportional to floor(area / largest area * 2**36), by a 64-bit hash of (random_seed, row); two more hashes r, s give
        bc = (1 - sqrt(r), (1 - s) sqrt(r), s sqrt(r)). Equal arguments give equal bits; the first n rows of a longer call with the same
        seed are the call with n; no row depends on how the GPU was launched. A face smaller than 2**-36 of the largest one is never drawn.
        A mesh without area raises ValueError("Mesh has zero area"), one whose areas overflow v's dtype ValueError as well; so do
        non-finite coordinates, face indices outside [0, #v) and more than 2**27 - 16 rows or samples.
    """
    _check_mesh(v, f)
    num_samples = int(num_samples)
    if num_samples <= 0:
        raise ValueError("num_samples must be positive")
    _check_rows(num_samples)
    seed = _seed(random_seed)
    d, ff, nv, nf = _resolve(v, f)
    fi, bc = d.empty((num_samples,), "i64"), d.empty((num_samples, 3), "T")
    _call("sample_mesh_random", d, *_mesh_args(d, ff, nv, nf), num_samples, seed, _Dev.ptr(fi), _Dev.ptr(bc))
    return _face_rows(fi, bc, ff, num_samples)


def sample_mesh_poisson_disk(v, f, num_samples, radius=0.0, use_geodesic_distance=True, best_choice_sampling=True, random_seed=0,
                             sample_num_tolerance=0.04, oversampling_factor=40.0):
    """
    Downsample a point set (possibly on a mesh) so that samples are approximately evenly spaced.

    Args:
        v : #v by 3 array of mesh vertex positions (float32 or float64; numpy, or a CUDA/HIP torch tensor)
        f : #f by 3 array of mesh face indices (int32, int64, uint32 or uint64; int32 / int64 for torch)
        num_samples: desired number of Poisson Disk samples. The number returned lies within sample_num_tolerance of it (if the radius
                     search converges within its 20 bisection steps). If this value <= 0, then the parameter radius is used instead.
        radius : desired separation between points. If it is positive it decides the sampling, whatever num_samples is (0.0 by default).
        use_geodesic_distance : accepted and ignored (the reference's body never reads it).
        best_choice_sampling : accepted and ignored (the reference's body never reads it).
        random_seed : A random seed used to generate the samples. Passing in 0 will use the current time. (0 by default).
        sample_num_tolerance: with num_samples > 0 and no radius, the function returns between (1 - sample_num_tolerance) * num_samples
                              and (1 + sample_num_tolerance) * num_samples samples. (0.04 by default).
        oversampling_factor: the samples are pruned from a dense random sampling of oversampling_factor * num_samples candidates (with a
                             radius, num_samples is estimated as area / (0.7 pi radius^2)). Must be >= 1.0. (Default 40.0).

    Returns:
        f_idx : a (m,)-shaped array of face indices into f where m is the number of Poisson-disk samples (f's dtype)
        bc : a (m, 3)-shaped array of barycentric coordinates where m is the number of Poisson-disk samples (v's dtype)

    Notes:
        The candidates are the rows of sample_mesh_random(v, f, N_c, random_seed); the rows kept are those that
        downsample_point_cloud_poisson_disk keeps, with the same seed, for the candidates' positions
        interpolate_barycentric_coords(f, f_idx, bc, v): at `radius`, or with target_num_samples = num_samples and sample_num_tolerance.
        They come back in ascending candidate order; equal arguments give equal bits. This differs from the reference on purpose: its body
        runs once at the radius sqrt(area / (0.7 pi num_samples)) and never looks at sample_num_tolerance (about 1333 samples for a request
        of 1000); here the documented count is kept. Errors as for sample_mesh_random, and for more than 2**27 - 16 candidates.
    """
    _check_mesh(v, f)
    num_samples, radius = int(num_samples), float(radius)
    if num_samples <= 0 and radius <= 0.0:
        raise ValueError("Cannot have both num_samples <= 0 and radius <= 0")
    tol = float(np.float32(sample_num_tolerance))          # (float arguments in the reference)
    if not (0.0 < tol <= 1.0):
        raise ValueError("sample_num_tolerance must be in (0, 1]")
    of = float(np.float32(oversampling_factor))
    if not of >= 1.0:
        raise ValueError("oversampling_factor must be >= 1.0")
    if num_samples <= 0 and radius != radius:
        raise ValueError("radius must not be NaN")
    _check_rows(num_samples)
    n_c = None
    if not radius > 0.0:                                   # (with a radius the candidate count depends on the mesh's area: the library is asked)
        n_c = math.ceil(of * max(num_samples, 1))
        if n_c > _MAX_ROWS:
            raise ValueError(f"sample_mesh_poisson_disk needs {float(n_c):g} candidates: more than 2^27-16 rows are not supported")
    seed = _seed(random_seed)
    d, ff, nv, nf = _resolve(v, f)
    mesh = _mesh_args(d, ff, nv, nf)
    cnt = ctypes.c_int64(0)

    def call(capacity, fi, bc):
        st = Stats()
        rc = _fn("sample_mesh_poisson_disk", d.suffix)(d.ctx, *mesh, num_samples, radius, seed, tol, of, capacity, _Dev.ptr(fi), _Dev.ptr(bc),
                                                       ctypes.addressof(cnt), d.flags, d.stream, ctypes.addressof(st))
        if rc:
            _lib.check(rc)
        _record(st)

    if n_c is None:
        call(0, None, None)
        n_c = int(cnt.value)
    fi, bc = d.empty((n_c,), "i64"), d.empty((n_c, 3), "T")
    call(n_c, fi, bc)
    m = int(cnt.value)
    fi, bc = fi[:m], bc[:m]
    if n_c > 2 * m:                                        # (do not keep the candidates' room alive behind a small result)
        fi, bc = (fi.clone(), bc.clone()) if d.torch else (fi.copy(), bc.copy())
    return _face_rows(fi, bc, ff, m)
