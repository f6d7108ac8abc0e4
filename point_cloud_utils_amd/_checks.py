"""The argument checks that more than one feature module uses, one copy each: scalar types, the reference's shape checks with its texts
(src/common/common.h) and the k-NN family's pair checks (src/point_cloud_distance.cpp), this package's row limit, what the library checks on the device found on the host for host arrays, and the placing of
further arrays beside the resolved ones of a call. Order, texts and exception types are part of the contract (tests/test_check_texts.py).
It imports _call only."""
import math
import operator
import time

import numpy as np

from ._call import _FACE_KINDS, _Dev, _dtype_name, _is_torch, _shape2

_MAX_ROWS = 2 ** 27 - 16
_ROW_LIMIT = "meshes and point clouds with more than 2^27-16 rows are not supported"
_KNN_ROW_LIMIT = "point clouds with more than 2^27-16 rows are not supported"       # the k-NN family's text (csrc/pcu_hip.hip: validate_sizes)
_KNN_ZERO = ("Invalid input set with zero elements: query_points and dataset_points must have shape (n, 3) and (m, 3). "
             "Got query_points.shape = ({}, {}), dataset_points.shape = ({}, {}).")
_KNN_DIM = ("Only 3D inputs are supported: query_points and dataset_points must have shape (n, 3) and (m, 3). "
            "Got query_points.shape = ({}, {}), dataset_points.shape = ({}, {}).")
_HD_ZERO = ("Invalid input set with zero elements: source and targets must have shape (n, 3) and (m, 3). "
            "Got source.shape = ({}, {}), target.shape = ({}, {}).")
_HD_DIM = ("Only 3D inputs are supported: source and targets must have shape (n, 3) and (m, 3). "
           "Got source.shape = ({}, {}), target.shape = ({}, {}).")
_SAME_DEVICE = "torch inputs must all be CUDA/HIP tensors on the same device"
_RAY_ROWS = ("ray_o and ray_d must have the same number of rows (one ray origin per ray direction). "
             "(Note: ray_o can have one row to use the same origin for all directions)")
_ZERO_POINTS = "Invalid input point cloud with zero points: points must have shape (n, 3) (n > 0). Got points.shape =({}, {})."
_NOT_3D = "Only 3D inputs are supported: v must have shape (n, 3) (n > 0). Got points.shape =({}, {})."


# ------------------------------------------------------------------------------------------------ scalar types and counts
def _check_float(x, name):
    dx = _dtype_name(x)
    if dx not in ("float32", "float64"):
        raise ValueError(f"Invalid scalar type ({dx}) for argument '{name}'. Expected one of ['float32', 'float64'].")
    return dx


def _match(x, name, want, what):
    dx = _dtype_name(x)
    if dx != want:
        raise ValueError(f"Invalid scalar type ({dx}) for argument '{name}'. Expected it to match {what} which is of type {want}.")


def _check_rows(*counts, text=_ROW_LIMIT):
    if max(counts) > _MAX_ROWS:
        raise ValueError(text)


def _check_pair(a, b, aname, bname, zero_fmt, dim_fmt):
    """dtype / shape validation of two clouds in the order of src/point_cloud_distance.cpp:136-149 (and :195-208)."""
    da, db = _check_float(a, aname), _dtype_name(b)
    if db != da:
        raise ValueError(f"Invalid scalar type ({db}) for argument '{bname}'. Expected it to match argument "
                         f"'{aname}' which is of type {da}.")
    sa, sb = _shape2(a), _shape2(b)
    if sa[0] == 0 or sb[0] == 0:
        raise ValueError(zero_fmt.format(sa[0], sa[1], sb[0], sb[1]))
    if sa[1] != 3 or sb[1] != 3:
        raise ValueError(dim_fmt.format(sa[0], sa[1], sb[0], sb[1]))
    return da


def _check_finite(x, text):
    """For the calls that have no stable meaning for non-finite coordinates: numpy or torch, refused with the caller's text before any work."""
    if _is_torch(x):
        import torch
        finite = bool(torch.isfinite(x).all())
    else:
        finite = bool(np.isfinite(x).all())
    if not finite:
        raise ValueError(text)


def _check_finite_cloud(points):
    """The cloud of the calls that take one cloud and no non-finite coordinate (farthest-point sampling, plane segmentation): dtype, shape,
    zero rows, the row limit, then the Poisson-disk call's rule. Returns the number of rows."""
    _check_float(points, "points")
    sp = _shape2(points)
    if sp[1] != 3:
        raise ValueError(_NOT_3D.format(*sp))
    if sp[0] == 0:
        raise ValueError(_ZERO_POINTS.format(*sp))
    _check_rows(sp[0])
    # no stable meaning for non-finite coordinates: refused before any work on them
    _check_finite(points, "points must not contain NaN or infinite coordinates")
    return sp[0]


def _size(a):
    n = 1
    for x in a.shape:
        n *= int(x)
    return n


# ------------------------------------------------------------------------------------------------ points, normals, parameters
def _check_points_dtype(p, want=None):
    dp = _check_float(p, "p")
    if want is not None and dp != want:
        raise ValueError(f"Invalid scalar type ({dp}) for argument 'p'. Expected it to match the indexed mesh which is of type {want}.")
    return dp, _shape2(p)


def _check_points(p, want=None):
    """Scalar type, then validate_point_cloud (src/common/common.h:58-74; zero rows are allowed), then the row limit. Returns (dtype name, #p)."""
    dp, sp = _check_points_dtype(p, want)
    if sp[1] != 3:
        raise ValueError(_NOT_3D.format(*sp))
    _check_rows(sp[0])
    return dp, sp[0]


def _check_points_nonzero(p):
    """validate_point_cloud(p, allow_0=false) (src/common/common.h:58-74), then the row limit. Returns #p."""
    sp = _shape2(p)
    if sp[0] == 0:
        raise ValueError(_ZERO_POINTS.format(*sp))
    if sp[1] != 3:
        raise ValueError(_NOT_3D.format(*sp))
    _check_rows(sp[0])
    return sp[0]


def _check_normals(p, n, allow_zero, **more):
    """Scalar types (p's; n and the arrays of `more`, by argument name, must match it), then validate_point_cloud_normals(p, n, allow_0)
    (src/common/common.h:78-110). Returns (dtype name, #p); the row limit is the caller's."""
    dp = _check_float(p, "p")
    for name, x in (("n", n),) + tuple(more.items()):
        _match(x, name, dp, "argument 'p'")
    sp, sn = _shape2(p), _shape2(n)
    if sp[0] == 0 and not allow_zero:
        raise ValueError(_ZERO_POINTS.format(*sp))
    if sp[1] != 3:
        raise ValueError(_NOT_3D.format(*sp))
    if sn[1] != 3:
        raise ValueError(f"Invalid shape for normals: must have shape (n, 3) (n > 0). Got normals.shape =({sn[0]}, {sn[1]}).")
    if sn[0] != sp[0]:
        raise ValueError("Invalid input point cloud. Number of normals must match number of points. "
                         f"Got points.shape =({sp[0]}, {sp[1]}) and normals.shape = {sn[0]}, {sn[1]}")
    return dp, sp[0]


def _check_beta(beta, noun):
    beta = float(beta)
    if not beta > 0.0:
        raise ValueError(f"beta must be greater than 0 (finite, or +inf for the plain sum over all {noun})")
    return beta


def _check_radius(radius):
    """The radius of the fixed-radius calls, and eps of the clustering built on them."""
    radius = float(radius)
    if not (radius >= 0.0) or math.isinf(radius):
        raise ValueError(f"Invalid radius ({radius}): must be finite and not negative.")
    return radius


_FEATURE_DIM_TOP = 128             # match_point_features (csrc/feature_match.h: kFmMaxD)
_FEATURE_ZERO = ("Invalid input set with zero elements: query_features and dataset_features must have shape (n, D) and (m, D). "
                 "Got query_features.shape = ({}, {}), dataset_features.shape = ({}, {}).")
_FEATURE_DIM_PAIR = ("Invalid feature dimension: query_features and dataset_features must have the same number of columns. "
                     "Got query_features.shape = ({}, {}), dataset_features.shape = ({}, {}).")


def _check_features(query_features, dataset_features):
    """The two feature arrays of match_point_features: scalar types as _check_pair states them, zero rows, one D for both, D in [1, 128],
    the k-NN row limit. Returns (n, m, D)."""
    dq, dd = _check_float(query_features, "query_features"), _dtype_name(dataset_features)
    if dd != dq:
        raise ValueError(f"Invalid scalar type ({dd}) for argument 'dataset_features'. Expected it to match argument "
                         f"'query_features' which is of type {dq}.")
    sq, sd = _shape2(query_features), _shape2(dataset_features)
    if sq[0] == 0 or sd[0] == 0:
        raise ValueError(_FEATURE_ZERO.format(sq[0], sq[1], sd[0], sd[1]))
    if sq[1] != sd[1]:
        raise ValueError(_FEATURE_DIM_PAIR.format(sq[0], sq[1], sd[0], sd[1]))
    if sq[1] < 1 or sq[1] > _FEATURE_DIM_TOP:
        raise ValueError(f"Invalid feature dimension ({sq[1]}): must be in [1, 128].")
    _check_rows(sq[0], sd[0], text=_KNN_ROW_LIMIT)
    return sq[0], sd[0], sq[1]


def _check_target_normals(target_normals, dtype_name, m):
    """The normals of register_point_clouds_icp's target: an (m, 3) array of the clouds' dtype (their kind is _beside's business)."""
    dn = _dtype_name(target_normals)
    if dn != dtype_name:
        raise ValueError(f"Invalid scalar type ({dn}) for argument 'target_normals'. Expected it to match argument "
                         f"'target_points' which is of type {dtype_name}.")
    sn = tuple(target_normals.shape)
    if sn != (m, 3):
        raise ValueError(f"Invalid shape for target_normals: must have shape ({m}, 3), one normal per target point. "
                         f"Got target_normals.shape = {sn}.")


def _check_max_correspondence_distance(distance):
    """Not _check_radius: +inf is allowed (and the default) -- every source row with a finite nearest distance then is an inlier."""
    distance = float(distance)
    if not distance >= 0.0:
        raise ValueError(f"Invalid max_correspondence_distance ({distance}): must not be NaN or negative.")
    return distance


def _check_tolerance(value, name):
    value = float(value)
    if not (value >= 0.0) or math.isinf(value):
        raise ValueError(f"Invalid {name} ({value}): must be finite and not negative.")
    return value


def _check_init_transform(init_transform):
    """None (identity), or anything numpy turns into a finite (4, 4) float64 matrix with last row [0, 0, 0, 1]. Returns a C-contiguous copy."""
    text = "Invalid init_transform: must be a finite (4, 4) matrix with last row [0, 0, 0, 1]."
    if init_transform is None:
        return np.eye(4, dtype=np.float64)
    if _is_torch(init_transform):
        init_transform = init_transform.detach().cpu().numpy()
    try:
        m = np.array(init_transform, dtype=np.float64, order="C")
    except (TypeError, ValueError):
        raise ValueError(text) from None
    if m.shape != (4, 4) or not bool(np.isfinite(m).all()) or m[3].tolist() != [0.0, 0.0, 0.0, 1.0]:
        raise ValueError(text)
    return m


_NUM_ITERATIONS_TOP = 2 ** 20      # hypotheses of segment_point_cloud_plane (csrc/plane_host.h)


def _check_plane_rows(n):
    if n < 3:
        raise ValueError(f"Invalid number of points ({n}): a plane needs at least 3.")
    return n


def _check_distance_threshold(distance_threshold):
    distance_threshold = float(distance_threshold)
    if not (distance_threshold >= 0.0) or math.isinf(distance_threshold):
        raise ValueError(f"Invalid distance_threshold ({distance_threshold}): must be finite and not negative.")
    return distance_threshold


def _check_num_iterations(num_iterations):
    try:
        m = operator.index(num_iterations)
    except TypeError:
        m = 0
    if m < 1 or m > _NUM_ITERATIONS_TOP:
        raise ValueError(f"Invalid num_iterations ({num_iterations}): must be an integer in [1, 2**20].")
    return m


def _check_seed(random_seed):
    """The seed rule of the sampling calls: an unsigned 32-bit integer, 0 means "from the clock". Returns the seed actually used, never 0."""
    seed = int(random_seed)
    if seed < 0 or seed > 0xFFFFFFFF:
        raise ValueError(f"random_seed must be an unsigned 32-bit integer, got {seed}")
    if seed == 0:
        seed = (time.time_ns() & 0xFFFFFFFF) or 1
    return seed


_CORRESPONDENCE_LIMIT = "correspondences with more than 2^27-16 rows are not supported"       # (csrc/ransac_host.h)


def _check_ransac_clouds(source_points, target_points):
    """The two clouds of register_point_clouds_ransac: each by _check_finite_cloud, then one dtype for both. Returns (n, m)."""
    n = _check_finite_cloud(source_points)
    m = _check_finite_cloud(target_points)
    _match(target_points, "target_points", _dtype_name(source_points), "argument 'source_points'")
    return n, m


def _check_correspondences(correspondences):
    """A (c, 2) int64 array with 3 <= c <= 2**27 - 16 (what its entries name is the library's to check, on the device). Returns c."""
    dc = _face_dtype_name(correspondences)
    if dc != "int64":
        raise ValueError(f"Invalid scalar type ({dc}) for argument 'correspondences'. Expected one of ['int64'].")
    sc = tuple(correspondences.shape)
    if len(sc) != 2 or sc[1] != 2:
        raise ValueError("Invalid shape for correspondences: must have shape (c, 2), one [source row, target row] per row. "
                         f"Got correspondences.shape = {sc}.")
    if sc[0] < 3:
        raise ValueError(f"Invalid number of correspondences ({sc[0]}): a rigid transform needs at least 3.")
    _check_rows(sc[0], text=_CORRESPONDENCE_LIMIT)
    return sc[0]


def _check_edge_length_ratio(edge_length_ratio):
    ratio = float(edge_length_ratio)
    if not (0.0 <= ratio <= 1.0):
        raise ValueError(f"Invalid edge_length_ratio ({ratio}): must be in [0, 1].")
    return ratio


def _check_bounds(lower_bound, upper_bound):
    lower_bound, upper_bound = float(lower_bound), float(upper_bound)
    if lower_bound != lower_bound or upper_bound != upper_bound:
        raise ValueError("lower_bound and upper_bound must not be NaN")
    if lower_bound > upper_bound:
        raise ValueError("lower_bound must not be greater than upper_bound")
    return lower_bound, upper_bound


# ------------------------------------------------------------------------------------------------ rays
def _check_rays(ray_o, ray_d, want, match):
    """Scalar types (both must be `want`; `match` names what that is), then the reference's shape checks in its order
    (src/ray_mesh_intersection.cpp:117-134). Returns (#rays, single origin?)."""
    _match(ray_o, "ray_o", want, match)
    _match(ray_d, "ray_d", want, match)
    so, sd = _shape2(ray_o), _shape2(ray_d)
    single = _size(ray_o) == 3
    if not single and so[0] != sd[0]:
        raise ValueError(_RAY_ROWS)
    if so[1] != 3 and not single:
        raise ValueError(f"Invalid shape for ray_o must have shape (N, 3) but got ({so[0]}, {so[1]}).")
    if sd[1] != 3:
        raise ValueError(f"Invalid shape for ray_d must have shape (N, 3) but got ({sd[0]}, {sd[1]}).")
    return sd[0], single


def _check_ray_limits(n, ray_near, ray_far):
    _check_rows(n)
    ray_near, ray_far = float(ray_near), float(ray_far)
    if ray_near != ray_near or ray_far != ray_far:
        raise ValueError("ray_near and ray_far must not be NaN")
    return ray_near, ray_far


def _origins_for(d, ray_o, single):
    """ray_o next to the resolved arrays of a call (_beside), as (1, 3) or (n, 3). Returns (array, rows)."""
    oo = _beside(d, ray_o)
    if single:
        oo = oo.reshape(1, 3)
    return oo, int(oo.shape[0])


# ------------------------------------------------------------------------------------------------ host arrays: what the device would find
def _host_finite(**arrays):
    """What the library checks on the device for device-resident input, found on the host for host arrays (before any device work)."""
    for name, x in arrays.items():
        if not bool(np.isfinite(x).all()):
            raise ValueError(f"{name} must not contain NaN or infinite " + ("values" if name == "a" else "coordinates"))


_KNN_NONFINITE = ("Invalid input: dataset_points contains NaN coordinates, or both +inf and -inf along one axis. The reference builds its kd-tree over "
                  "NaN bounds for such data and returns rows that depend on the traversal; not supported (non-finite query points and single-signed "
                  "infinities in the dataset are handled as the reference handles them).")       # (csrc/pcu_hip.hip: nonfinite_error)


def _host_searched_cloud(points):
    """The rule of every searched cloud, which the search checks on the device, found on the host for a host array: with the search's text."""
    if bool(np.isnan(points).any()) or bool(((points == np.inf).any(axis=0) & (points == -np.inf).any(axis=0)).any()):
        raise ValueError(_KNN_NONFINITE)


def _host_ray_checks(ray_o, ray_d):
    _host_finite(ray_o=ray_o, ray_d=ray_d)


def _host_mesh_checks(v, f):
    _host_finite(v=v)
    nv = int(v.shape[0])
    if (f.dtype.kind == "i" and int(f.min()) < 0) or int(f.max()) >= nv:
        raise ValueError(f"f must hold row indices of v: found a face index outside [0, {nv})")


# ------------------------------------------------------------------------------------------------ meshes
def _beside(d, x):
    """`x` next to the resolved arrays of a call: same kind (torch on that device / numpy), contiguous."""
    if d.torch:
        if not _is_torch(x) or not x.is_cuda or x.device != d.tdev:
            raise ValueError(_SAME_DEVICE)
        return x.contiguous()
    if _is_torch(x):
        raise ValueError(_SAME_DEVICE)
    return np.ascontiguousarray(x)


def _face_dtype_name(f):
    if _is_torch(f):
        return str(f.dtype).replace("torch.", "")
    return np.asarray(f).dtype.name


def _check_face_dtype(f):
    df = _face_dtype_name(f)
    kinds = ["int32", "int64"] if _is_torch(f) else list(_FACE_KINDS)
    if df not in kinds:
        raise ValueError(f"Invalid scalar type ({df}) for argument 'f'. Expected one of {kinds}.")


def _check_mesh(v, f, want=None):
    """Scalar types, then validate_mesh (src/common/common.h:133-147), then this package's row limit. Returns (dtype name, #v, #f)."""
    dv = _check_float(v, "v") if want is None else _dtype_name(v)
    if want is not None and dv != want:
        raise ValueError(f"Invalid scalar type ({dv}) for argument 'v'. Expected it to match argument 'p' which is of type {want}.")
    _check_face_dtype(f)
    sv, sf = _shape2(v), _shape2(f)
    got = f"Got v.shape =({sv[0]}, {sv[1]}), f.shape = ({sf[0]}, {sf[1]})."
    if sv[0] == 0 or sf[0] == 0:
        raise ValueError("Invalid input mesh with zero elements: v and f must have shape (n, 3) and (m, 3) (n, m > 0). " + got)
    if sv[1] != 3 or sf[1] != 3:
        raise ValueError("Only 3D inputs are supported: v and f must have shape (n, 3) and (m, 3) (n, m > 0). " + got)
    _check_rows(sv[0], sf[0])
    return dv, sv[0], sf[0]


def _resolve(v, f):
    """The arrays of a call whose mesh passed _check_mesh: host checks for host arrays, then (_Dev, faces, #v, #f)."""
    if not (_is_torch(v) or _is_torch(f)):
        _host_mesh_checks(np.asarray(v), np.asarray(f))
    d = _Dev(v, v)
    ff = _beside(d, f)
    return d, ff, _shape2(v)[0], _shape2(f)[0]


def _mesh_args(d, ff, nv, nf):
    return d.pa, nv, _Dev.ptr(ff), nf, _FACE_KINDS[_face_dtype_name(ff)]


# ------------------------------------------------------------------------------------------------ results
def _scalar_rows(w, n):
    return w.reshape(()) if n == 1 else w


def _face_rows(fi, bc, like, n):
    """(f_idx, bc) as returned: the face in the dtype of `like`, f's (-1 wraps for an unsigned one, as the reference's assignment does);
    singleton dimensions squeezed as the package's other calls do (numpyeigen's squeeze)."""
    fi = fi.to(like.dtype) if _is_torch(fi) else fi.astype(like.dtype, copy=False)
    if n == 1:
        fi, bc = fi.reshape(()), bc.reshape(3)
    return fi, bc
