"""mesh_face_areas, sample_mesh_random and sample_mesh_poisson_disk on the GPU (-m gpu), bit for bit against the numpy restatement of the
contract (tests/sampling_contract.py): the bits of the areas, the face indices, the bits of the barycentric coordinates,
the rows the Poisson-disk greedy keeps."""
import functools

import numpy as np
import pytest

import sampling_contract as sc
from test_gpu_poisson_disk import check_properties, greedy

pytestmark = pytest.mark.gpu

SEED = 1234567
DTYPES = [np.float32, np.float64]
FACE_DTYPES = [np.int32, np.int64, np.uint32, np.uint64]
TILE = sc.SC_TILE             # 4096: the tile of the library's 64-bit inclusive scan (csrc/radix.h: kScTile)
TABLE = sc.TABLE              # 1024: the entries of k_mesh_sample's LDS table; its stride is ceil(#f / 1024)


@pytest.fixture(scope="module")
def pcu():
    import point_cloud_utils_amd as m
    from point_cloud_utils_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: the gfx950 path has no CPU fallback"
    return m


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_rows(got, want, what=""):
    fi, bc = got
    wfi, wbc = want
    assert fi.shape == wfi.shape and bc.shape == wbc.shape, (what, fi.shape, wfi.shape)
    assert np.array_equal(np.asarray(fi).astype(np.int64), wfi), what
    assert bc.dtype == wbc.dtype and np.array_equal(bits(bc), bits(wbc)), what


def to_torch(*arrays):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


def to_numpy(*tensors):
    return tuple(t.cpu().numpy() for t in tensors)


@functools.lru_cache(maxsize=None)
def mesh(name, dtype):
    return sc.golden_mesh(name, dtype)


def soup(nf, dtype, seed=5):
    """nf faces over 600 random vertices, areas spread over three decades."""
    rng = np.random.default_rng(seed)
    v = rng.random((600, 3)) * np.array([1.0, 1.0, 0.001])
    v[:300] *= 0.03
    f = rng.integers(0, 600, (nf, 3))
    return np.ascontiguousarray(v.astype(dtype)), f.astype(np.int64)


# ---------------------------------------------------------------------------------------------------- areas
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["bunny", "cube_twist"])
def test_areas_equal_the_restatement(pcu, name, dtype):
    v, f = mesh(name, dtype)
    a = pcu.mesh_face_areas(v, f)
    assert a.dtype == dtype and a.shape == (len(f),)
    assert np.array_equal(bits(a), bits(sc.face_areas(v, f)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_areas_at_block_and_wave_edges(pcu, dtype):
    v, f = mesh("bunny", dtype)
    want = sc.face_areas(v, f)
    for nf in (2, 63, 64, 65, 255, 256, 257):
        assert np.array_equal(bits(pcu.mesh_face_areas(v, f[:nf])), bits(want[:nf])), nf
    a1 = pcu.mesh_face_areas(v, f[:1])
    assert a1.shape == () and bits(a1.reshape(1))[0] == bits(want[:1])[0]


@pytest.mark.parametrize("dtype", DTYPES)
def test_degenerate_faces_have_area_zero(pcu, dtype):
    v, f = mesh("bunny", dtype)
    i, j = int(f[10, 0]), int(f[10, 1])
    fd = np.concatenate([f[:5], [[i, j, j], [i, i, i], [j, i, i]], f[5:9]]).astype(np.int64)
    a = pcu.mesh_face_areas(v, fd)
    assert np.array_equal(bits(a), bits(sc.face_areas(v, fd)))
    assert np.all(a[5:8] == 0) and not np.any(np.signbit(a[5:8])) and np.all(a[:5] > 0)


@pytest.mark.parametrize("scale", [2.0 ** 40, 2.0 ** -40, 2.0 ** 70])
def test_areas_where_squares_overflow_or_vanish_are_what_ieee_gives(pcu, scale):
    v, f = mesh("bunny", np.float32)
    vs = np.ascontiguousarray((v * np.float32(scale)).astype(np.float32))
    assert np.all(np.isfinite(vs))
    want = sc.face_areas(vs, f)
    a = pcu.mesh_face_areas(vs, f)
    assert np.array_equal(np.isnan(a), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.array_equal(bits(a[ok]), bits(want[ok]))
    print("scale", scale, "inf", int(np.isinf(want).sum()), "nan", int(np.isnan(want).sum()), "zero", int((want == 0).sum()))


def test_areas_reference_test_body(pcu):
    v = np.array([[0., 0., 0.], [0., 1., 0.], [1., 0., 0.]])
    f = np.array([[0, 1, 2]])
    a = pcu.mesh_face_areas(v, f)
    assert abs(float(a) - 0.5) < 1e-7
    v, f = mesh("bunny", np.float64)
    a = pcu.mesh_face_areas(v, f)
    a2 = pcu.mesh_face_areas(v, f[::2])
    assert np.all(a2 == a[::2])
    with pytest.raises(ValueError):
        pcu.mesh_face_areas(v, np.zeros([0, 3], dtype=int))
    with pytest.raises(ValueError):
        pcu.mesh_face_areas(v, np.random.randint(0, v.shape[0] - 1, size=[100, 2], dtype=int))


@pytest.mark.parametrize("dtype", DTYPES)
def test_areas_face_dtypes_and_torch(pcu, dtype):
    import torch
    v, f = mesh("cube_twist", dtype)
    want = bits(sc.face_areas(v, f))
    for fdt in FACE_DTYPES:
        assert np.array_equal(bits(pcu.mesh_face_areas(v, f.astype(fdt))), want), fdt
    for fdt in (np.int32, np.int64):
        a = pcu.mesh_face_areas(*to_torch(v, f.astype(fdt)))
        assert isinstance(a, torch.Tensor) and a.is_cuda and a.dtype == to_torch(v)[0].dtype
        assert np.array_equal(bits(a.cpu().numpy()), want), fdt


def test_areas_device_resident_input_is_checked_by_the_kernels(pcu):
    v, f = mesh("bunny", np.float32)
    bad_v = v.copy(); bad_v[17, 1] = np.nan
    bad_f = f.copy(); bad_f[100, 2] = len(v)
    for call in (lambda v, f: pcu.mesh_face_areas(v, f), lambda v, f: pcu.sample_mesh_random(v, f, 100, SEED),
                 lambda v, f: pcu.sample_mesh_poisson_disk(v, f, 100, random_seed=SEED)):
        with pytest.raises(ValueError, match="v must not contain NaN or infinite coordinates"):
            call(*to_torch(bad_v, f))
        with pytest.raises(ValueError, match=r"found a face index outside \[0, %d\)" % len(v)):
            call(*to_torch(v, bad_f))


# ---------------------------------------------------------------------------------------------------- scan and search edges
# The face counts at which a tiled 64-bit scan or a two-level search can go wrong: below, at and above the scan's tile (4096 faces) and the
# strides of the 1024-entry table (stride 1 up to 1024 faces, 2 up to 2048, 38 at 37,889 ...), one and two tiles, many tiles.
EDGE_COUNTS = [1, 2, 3, 64, 65, TABLE - 1, TABLE, TABLE + 1, 2 * TABLE - 1, 2 * TABLE + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 37 * TABLE - 1, 37 * TABLE + 1]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nf", EDGE_COUNTS)
def test_samples_at_scan_and_search_edges(pcu, nf, dtype):
    v, f = soup(nf, dtype)
    same_rows(pcu.sample_mesh_random(v, f, 1000, SEED), sc.sample_mesh_random(v, f, 1000, SEED), nf)


def test_sum_of_weights_beyond_2_to_54(pcu):
    """2^18 + 1 copies of one face: W = (2^18 + 1) 2^36 > 2^54. A sum kept in a double or in 32 bits, or a hi64 done in floating point, fails."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=np.float32)
    f = np.tile(np.array([[0, 1, 2]], dtype=np.int32), (2 ** 18 + 1, 1))
    want = sc.sample_mesh_random(v, f, 1000, SEED)
    assert len(np.unique(want[0])) > 990 and want[0].max() > 2 ** 18 - 2 ** 10
    same_rows(pcu.sample_mesh_random(v, f, 1000, SEED), want)
    same_rows(pcu.sample_mesh_random(v, f, 65_537, SEED + 1), sc.sample_mesh_random(v, f, 65_537, SEED + 1))


def test_scan_beyond_1024_tiles(pcu):
    """More than 1024 scan tiles: the second trip of the carry loop of k_sc_sums in its 64-bit instance (W = 4,198,404 x 2^36 > 2^58)."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=np.float32)
    f = np.tile(np.array([[0, 1, 2]], dtype=np.int32), (TILE * 1024 + TILE + 4, 1))
    want = sc.sample_mesh_random(v, f, 1000, SEED)
    assert (want[0] >= TILE * 1024).sum() >= 1 and (want[0] < TILE * 1024).sum() >= 1          # (rows on both sides of the 1024th tile)
    same_rows(pcu.sample_mesh_random(v, f, 1000, SEED), want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_equal_faces_are_chosen_by_the_top_bit(pcu, dtype):
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=dtype)
    f = np.array([[0, 1, 2], [2, 0, 1]], dtype=np.int64)
    fi, _ = pcu.sample_mesh_random(v, f, 1000, SEED)
    h0, _, _ = sc.draws(SEED, 1000)
    assert np.array_equal(fi, (h0 >> np.uint64(63)).astype(np.int64))


@pytest.mark.parametrize("dtype", DTYPES)
def test_tiny_and_degenerate_faces_are_never_drawn(pcu, dtype):
    """One face of area 1/2 beside faces of about 2^-40 of it (weight 0) and degenerate ones, interleaved."""
    t = 2.0 ** -20
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, t, 0], [t, 0, 0]], dtype=dtype)
    unit = np.array([[0, 3, 4], [0, 1, 1], [2, 2, 2], [0, 4, 3]], dtype=np.int64)
    f = np.concatenate([np.tile(unit, (40, 1)), [[0, 1, 2]], np.tile(unit, (40, 1))])
    w = sc.weights(sc.face_areas(v, f))[0]
    assert w[160] == 2 ** 36 and w.sum() == 2 ** 36
    fi, bc = pcu.sample_mesh_random(v, f, 1000, SEED)
    assert np.all(fi == 160)
    same_rows((fi, bc), sc.sample_mesh_random(v, f, 1000, SEED))


# ---------------------------------------------------------------------------------------------------- sample counts and call forms
@functools.lru_cache(maxsize=None)
def reference_rows(name, dtype, seed, n=65_537):
    v, f = mesh(name, dtype)
    return sc.sample_mesh_random(v, f, n, seed)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [63, 64, 65, 4095, 4097, 65_537])
def test_sample_counts(pcu, n, dtype):
    v, f = mesh("bunny", dtype)
    wfi, wbc = reference_rows("bunny", dtype, SEED)
    fi, bc = pcu.sample_mesh_random(v, f, n, SEED)
    assert fi.dtype == f.dtype and bc.dtype == dtype
    same_rows((fi, bc), (wfi[:n], wbc[:n]), n)


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_sample_squeezes(pcu, dtype):
    v, f = mesh("cube_twist", dtype)
    wfi, wbc = reference_rows("cube_twist", dtype, SEED)
    fi, bc = pcu.sample_mesh_random(v, f, 1, SEED)
    assert fi.shape == () and bc.shape == (3,)
    assert int(fi) == wfi[0] and np.array_equal(bits(bc), bits(wbc[0]))


@pytest.mark.parametrize("dtype", DTYPES)
def test_prefix_repeat_and_seeds(pcu, dtype):
    v, f = mesh("cube_twist", dtype)
    long_ = pcu.sample_mesh_random(v, f, 10_000, SEED)
    short = pcu.sample_mesh_random(v, f, 1_237, SEED)
    same_rows(short, (long_[0][:1_237], long_[1][:1_237]), "prefix")
    same_rows(pcu.sample_mesh_random(v, f, 10_000, SEED), long_, "repeat")
    other = pcu.sample_mesh_random(v, f, 10_000, 7654321)
    assert not np.array_equal(other[0], long_[0]) and not np.array_equal(other[1], long_[1])
    same_rows(other, tuple(a[:10_000] for a in reference_rows("cube_twist", dtype, 7654321)), "other seed")


def test_seed_zero_draws_from_the_clock(pcu):
    v, f = mesh("bunny", np.float32)
    a = pcu.sample_mesh_random(v, f, 2_000, 0)
    b = pcu.sample_mesh_random(v, f, 2_000, 0)          # (the clock has nanoseconds: two calls never see the same value)
    assert not np.array_equal(a[0], b[0])
    p = pcu.sample_mesh_poisson_disk(v, f, 200, random_seed=0, oversampling_factor=5.0)
    q = pcu.sample_mesh_poisson_disk(v, f, 200, random_seed=0, oversampling_factor=5.0)
    assert p[0].shape != q[0].shape or not np.array_equal(p[0], q[0])


@pytest.mark.parametrize("dtype", DTYPES)
def test_face_dtypes_numpy_and_torch_give_equal_bits(pcu, dtype):
    import torch
    v, f = mesh("bunny", dtype)
    want = tuple(a[:5_000] for a in reference_rows("bunny", dtype, SEED))
    for fdt in FACE_DTYPES:
        fi, bc = pcu.sample_mesh_random(v, f.astype(fdt), 5_000, SEED)
        assert fi.dtype == fdt
        same_rows((fi, bc), want, fdt)
    for fdt, tdt in ((np.int32, torch.int32), (np.int64, torch.int64)):
        fi, bc = pcu.sample_mesh_random(*to_torch(v, f.astype(fdt)), 5_000, random_seed=SEED)
        assert fi.is_cuda and bc.is_cuda and fi.dtype == tdt and fi.shape == (5_000,) and bc.shape == (5_000, 3)
        same_rows(to_numpy(fi, bc), want, ("torch", fdt))


@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_area_and_overflowing_areas_raise(pcu, dtype):
    v, f = mesh("bunny", dtype)
    flat = np.ascontiguousarray(np.repeat(v[:1], len(v), axis=0))
    calls = (lambda v, f: pcu.sample_mesh_random(v, f, 100, SEED), lambda v, f: pcu.sample_mesh_poisson_disk(v, f, 100, random_seed=SEED))
    for call in calls:
        with pytest.raises(ValueError, match="^Mesh has zero area$"):
            call(flat, f)
        with pytest.raises(ValueError, match="^Mesh has zero area$"):
            call(v, np.array([[0, 1, 1], [2, 2, 2]]))
        with pytest.raises(ValueError, match="^Mesh has zero area$"):
            call(*to_torch(flat, f))
    big = np.ascontiguousarray((v * dtype(2.0 ** 40 if dtype is np.float32 else 2.0 ** 300)).astype(dtype))
    assert np.all(np.isfinite(big)) and not np.all(np.isfinite(sc.face_areas(big, f)))
    for call in calls:
        with pytest.raises(ValueError, match="^face areas overflow the scalar type of v$"):
            call(big, f)
        with pytest.raises(ValueError, match="^face areas overflow the scalar type of v$"):
            call(*to_torch(big, f))


# ---------------------------------------------------------------------------------------------------- Poisson disk
@functools.lru_cache(maxsize=None)
def poisson_reference(name, dtype, num_samples, of, radius_rel=0.0, seed=SEED):
    v, f = mesh(name, dtype)
    diag = float(np.linalg.norm(v.max(0).astype(np.float64) - v.min(0).astype(np.float64)))
    radius = radius_rel * diag
    return (radius,) + sc.sample_mesh_poisson_disk(v, f, num_samples, seed, greedy, radius=radius, oversampling_factor=of)


POISSON_CASES = [(1000, 5.0, 0.0), (200, 40.0, 0.0), (-1, 5.0, 0.05)]          # (num_samples, oversampling_factor, radius / bbox diagonal)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("num_samples,of,radius_rel", POISSON_CASES)
@pytest.mark.parametrize("name", ["bunny", "cube_twist"])
def test_poisson_equals_the_restatement_and_the_packages_own_composition(pcu, name, num_samples, of, radius_rel, dtype):
    v, f = mesh(name, dtype)
    radius, wfi, wbc, P, keep, n_c, r_last = poisson_reference(name, dtype, num_samples, of, radius_rel)
    fi, bc = pcu.sample_mesh_poisson_disk(v, f, num_samples, radius=radius, random_seed=SEED, oversampling_factor=of)
    st = pcu.last_stats()
    print(name, np.dtype(dtype).name, (num_samples, of, radius_rel), "candidates", n_c, "kept", len(fi), "stats", st["n_queries"], st["n_passes"], st["n_grid_builds"])
    assert fi.dtype == f.dtype and bc.dtype == dtype
    same_rows((fi, bc), (wfi, wbc), "restatement")
    assert st["n_queries"] == n_c and st["n_grid_builds"] >= 1 and st["n_passes"] >= 1
    # the package's own composition: sample_mesh_random -> interpolate_barycentric_coords in numpy -> downsample_point_cloud_poisson_disk
    cfi, cbc = pcu.sample_mesh_random(v, f, n_c, SEED)
    cP = pcu.interpolate_barycentric_coords(f, cfi, cbc, v)
    assert cP.dtype == dtype and np.array_equal(bits(cP), bits(P))
    if radius > 0:
        idx = pcu.downsample_point_cloud_poisson_disk(cP, radius, random_seed=SEED)
    else:
        idx = pcu.downsample_point_cloud_poisson_disk(cP, 0.0, target_num_samples=num_samples, random_seed=SEED)
    assert np.array_equal(idx, keep)
    same_rows((fi, bc), (cfi[idx], cbc[idx]), "composition")
    check_properties(P, keep, r_last)
    if num_samples > 0:
        lo, hi = sc.count_limits(num_samples, 0.04, dtype)
        assert lo <= len(fi) <= hi
    # device-resident in and out: equal bits
    tfi, tbc = pcu.sample_mesh_poisson_disk(*to_torch(v, f), num_samples, radius=radius, random_seed=SEED, oversampling_factor=of)
    assert tfi.is_cuda and tbc.is_cuda
    same_rows(to_numpy(tfi, tbc), (wfi, wbc), "torch")


@pytest.mark.parametrize("dtype", DTYPES)
def test_poisson_oversampling_one_returns_every_candidate(pcu, dtype):
    v, f = mesh("bunny", dtype)
    fi, bc = pcu.sample_mesh_poisson_disk(v, f, 64, random_seed=SEED, oversampling_factor=1.0)
    wfi, wbc = reference_rows("bunny", dtype, SEED)
    same_rows((fi, bc), (wfi[:64], wbc[:64]))
    fi1, bc1 = pcu.sample_mesh_poisson_disk(v, f, 1, random_seed=SEED, oversampling_factor=1.0)
    assert fi1.shape == () and bc1.shape == (3,) and int(fi1) == wfi[0]


@pytest.mark.parametrize("dtype", DTYPES)
def test_poisson_radius_wins_over_num_samples(pcu, dtype):
    """Both given: the greedy runs at the radius; N_c = ceil(oversampling * max(num_samples, n_est, 1)), whichever of the two is larger."""
    name, of = "cube_twist", 5.0
    v, f = mesh(name, dtype)
    radius, wfi, wbc, _, _, n_c, _ = poisson_reference(name, dtype, -1, of, 0.05)
    n_est = n_c // 5
    got = pcu.sample_mesh_poisson_disk(v, f, n_est // 2, radius=radius, random_seed=SEED, oversampling_factor=of)      # n_est decides
    assert pcu.last_stats()["n_queries"] == n_c and pcu.last_stats()["n_grid_builds"] == 1
    same_rows(got, (wfi, wbc))
    many = 2 * n_est + 3                                                                                              # num_samples decides
    want = sc.sample_mesh_poisson_disk(v, f, many, SEED, greedy, radius=radius, oversampling_factor=of)
    assert want[4] == 5 * many
    got = pcu.sample_mesh_poisson_disk(v, f, many, radius=radius, random_seed=SEED, oversampling_factor=of)
    assert pcu.last_stats()["n_queries"] == 5 * many and pcu.last_stats()["n_grid_builds"] == 1
    same_rows(got, want[:2])


def test_poisson_radius_that_needs_too_many_candidates_raises(pcu):
    v, f = mesh("bunny", np.float32)
    for args in ((v, f), to_torch(v, f)):
        with pytest.raises(ValueError, match=r"candidates: more than 2\^27-16 rows are not supported"):
            pcu.sample_mesh_poisson_disk(*args, -1, radius=1e-6, random_seed=SEED)
        with pytest.raises(ValueError, match=r"candidates: more than 2\^27-16 rows are not supported"):
            pcu.sample_mesh_poisson_disk(*args, -1, radius=1e-30, random_seed=SEED)


def test_poisson_reference_test_body(pcu):
    v, f = mesh("cube_twist", np.float64)
    bbox_diag = np.linalg.norm(np.max(v, axis=0) - np.min(v, axis=0))
    f_idx1, bc1 = pcu.sample_mesh_random(v, f, num_samples=1000, random_seed=1234567)
    f_idx2, bc2 = pcu.sample_mesh_random(v, f, num_samples=1000, random_seed=1234567)
    f_idx3, bc3 = pcu.sample_mesh_random(v, f, num_samples=1000, random_seed=7654321)
    assert np.all(f_idx1 == f_idx2) and np.all(bc1 == bc2)
    assert not np.all(f_idx1 == f_idx3) and not np.all(bc1 == bc3)
    for kw in (dict(num_samples=1000, use_geodesic_distance=True), dict(num_samples=-1, radius=0.01 * bbox_diag)):
        f_idx1, bc1 = pcu.sample_mesh_poisson_disk(v, f, random_seed=1234567, oversampling_factor=5.0, **kw)
        f_idx2, bc2 = pcu.sample_mesh_poisson_disk(v, f, random_seed=1234567, oversampling_factor=5.0, **kw)
        f_idx3, bc3 = pcu.sample_mesh_poisson_disk(v, f, random_seed=7654321, oversampling_factor=5.0, **kw)
        assert np.all(f_idx1 == f_idx2) and np.all(bc1 == bc2)
        if f_idx1.shape == f_idx3.shape:
            assert not np.all(f_idx1 == f_idx3)
        if bc1.shape == bc3.shape:
            assert not np.all(bc1 == bc3)


# ---------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("dtype", DTYPES)
def test_mesh_to_samples_to_chamfer_without_leaving_the_device(pcu, dtype):
    """The pipeline the feature exists for: 100k samples on the bunny as tensors, interpolated, Chamfer distance to a second sampling."""
    import torch
    v, f = mesh("bunny", dtype)
    tv, tf = to_torch(v, f)
    clouds, host = [], []
    for seed in (SEED, 7654321):
        fi, bc = pcu.sample_mesh_random(tv, tf, 100_000, random_seed=seed)
        p = pcu.interpolate_barycentric_coords(tf, fi, bc, tv)
        assert isinstance(p, torch.Tensor) and p.is_cuda and p.shape == (100_000, 3)
        nfi, nbc = pcu.sample_mesh_random(v, f, 100_000, random_seed=seed)
        same_rows(to_numpy(fi, bc), (nfi, nbc), seed)
        clouds.append(p.contiguous())
        host.append(np.ascontiguousarray(p.cpu().numpy()))
    d_dev = pcu.chamfer_distance(clouds[0], clouds[1])
    d_host = pcu.chamfer_distance(host[0], host[1])
    print(np.dtype(dtype).name, "chamfer", float(d_dev))
    assert np.isfinite(float(d_dev)) and float(d_dev) > 0
    assert bits(np.asarray(d_dev, dtype=dtype).reshape(1))[0] == bits(np.asarray(d_host, dtype=dtype).reshape(1))[0]
