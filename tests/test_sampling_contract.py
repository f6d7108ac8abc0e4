"""CPU tests of the sampling contract's restatement (tests/sampling_contract.py) and of the host-side checks of
mesh_face_areas, sample_mesh_random and sample_mesh_poisson_disk. The limits are derived, not measured: a chi-square statistic with k degrees
of freedom has mean k and variance 2k, and the test allows mean plus six standard deviations; the figures measured with seed 1234567 and
200,000 samples stand next to them."""
import functools
import math

import numpy as np
import pytest

import sampling_contract as sc
from test_gpu_poisson_disk import greedy, greedy_target

SEED = 1234567
N = 200_000
MESHES = ["bunny", "cube_twist"]
DTYPES = [np.float32, np.float64]


@functools.lru_cache(maxsize=None)
def sampled(name, dtype):
    v, f = sc.golden_mesh(name, dtype)
    areas = sc.face_areas(v, f)
    w, C, W, amax = sc.weights(areas)
    fi, bc = sc.sample_rows(C, W, SEED, N, dtype)
    return v, f, areas, w, C, W, fi, bc


@pytest.mark.parametrize("name,smallest", [("bunny", 799_462), ("cube_twist", 50_378_772_577)])
def test_no_face_has_weight_zero(name, smallest):
    _, _, _, w, C, W, _, _ = sampled(name, np.float64)
    assert w.min() == smallest and w.min() > 0
    assert w.max() == 2 ** sc.WEIGHT_BITS
    assert W == sum(int(x) for x in w) and W <= 2 ** 63


def test_hi64_is_the_high_half_of_the_product():
    rng = np.random.default_rng(3)
    h = rng.integers(0, 2 ** 64, 2000, dtype=np.uint64)
    h[:4] = [0, 1, 2 ** 64 - 1, 2 ** 63]
    for W in (1, 2, 2 ** 32 - 1, 2 ** 32, 2 ** 36 * 262145, 2 ** 63, 160535517573796):
        assert [int(x) for x in sc.hi64(h, W)] == [(int(x) * W) >> 64 for x in h]


def test_draws_are_the_stated_hashes():
    def mix(z):
        z ^= z >> 30; z = (z * 0xBF58476D1CE4E5B9) & sc.M64
        z ^= z >> 27; z = (z * 0x94D049BB133111EB) & sc.M64
        return z ^ (z >> 31)
    h = sc.draws(SEED, 50)
    for i in (0, 1, 7, 49):
        p = mix((SEED << 32) ^ i)
        assert [int(h[j][i]) for j in range(3)] == [mix((p + (j + 1) * sc.GOLDEN_GAMMA) & sc.M64) for j in range(3)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", MESHES)
def test_face_choice_follows_the_areas(name, dtype):
    """Chi-square of the face counts over 64 groups of consecutive faces against float64 areas: 53.2 (bunny) and 68.6 (cube_twist)."""
    v, f, _, _, _, _, fi, _ = sampled(name, dtype)
    a64 = sc.face_areas(v.astype(np.float64), f)
    group = np.minimum(np.arange(len(f)) * 64 // len(f), 63)
    expected = np.bincount(group, weights=a64, minlength=64) / a64.sum() * N
    observed = np.bincount(group[fi], minlength=64)
    chi2 = float(((observed - expected) ** 2 / expected).sum())
    print(name, np.dtype(dtype).name, "chi2 over 64 face groups:", chi2)
    assert chi2 <= 63 + 6 * math.sqrt(126)                      # 130.3
    assert fi.min() >= 0 and fi.max() < len(f)


@pytest.mark.parametrize("dtype", DTYPES)
def test_barycentrics_are_uniform(dtype):
    """Chi-square over the 16 congruent sub-triangles floor(4 bc): 20.5; means within 2.4 sigma of 1/3."""
    *_, bc = sampled("bunny", dtype)
    b = bc.astype(np.float64)
    cell = np.minimum(np.floor(4 * b).astype(np.int64), 3)
    _, counts = np.unique(cell[:, 0] * 16 + cell[:, 1] * 4 + cell[:, 2], return_counts=True)
    assert len(counts) == 16
    chi2 = float(((counts - N / 16) ** 2 / (N / 16)).sum())
    z = (b.mean(0) - 1 / 3) / math.sqrt(1 / (18 * N))
    print(np.dtype(dtype).name, "chi2 over 16 sub-triangles:", chi2, "means, in sigma:", z)
    assert chi2 <= 15 + 6 * math.sqrt(30)                       # 47.9
    assert np.all(np.abs(z) <= 6)
    assert np.abs(bc.sum(1, dtype=dtype) - dtype(1)).max() <= np.finfo(dtype).eps
    assert bc.min() >= 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_prefix_property(dtype):
    _, _, _, _, C, W, fi, bc = sampled("cube_twist", dtype)
    for n in (1, 63, 4097):
        fi_n, bc_n = sc.sample_rows(C, W, SEED, n, dtype)
        assert np.array_equal(fi_n, fi[:n]) and np.array_equal(bc_n.view(np.uint8), bc[:n].view(np.uint8))
    fi_o, _ = sc.sample_rows(C, W, SEED + 1, 1000, dtype)
    assert not np.array_equal(fi_o, fi[:1000])


def test_degenerate_and_tiny_faces_are_never_drawn():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 2.0 ** -20, 0], [2.0 ** -20, 0, 0]], dtype=np.float64)
    f = np.array([[0, 1, 1], [0, 3, 4], [0, 1, 2], [2, 2, 2], [0, 4, 3]], dtype=np.int64)     # areas 0, about 2^-41, 1/2, 0, about 2^-41
    areas = sc.face_areas(v, f)
    assert areas[0] == 0 and areas[3] == 0 and 0 < areas[1] < 2.0 ** -40 and 0 < areas[4] < 2.0 ** -40
    w, C, W, _ = sc.weights(areas)
    assert list(w) == [0, 0, 2 ** 36, 0, 0]
    fi, _ = sc.sample_rows(C, W, SEED, 5000, np.float64)
    assert np.all(fi == 2)


# ---- the composition with the restated greedy and radius search of f5
POISSON = [  # mesh, request, oversampling, kept in float32, kept in float64
    ("bunny", 1000, 5.0, 984, 983), ("cube_twist", 1000, 5.0, 995, 995), ("bunny", 1000, 40.0, 974, 974), ("cube_twist", 1000, 40.0, 970, 970),
    ("bunny", 200, 40.0, 194, 194), ("cube_twist", 200, 40.0, 194, 194), ("bunny", 64, 1.5, 61, 61), ("cube_twist", 64, 1.5, 62, 62),
    ("bunny", 64, 1.0, 64, 64), ("cube_twist", 64, 1.0, 64, 64)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,request_n,of,kept32,kept64", POISSON)
def test_poisson_composition_keeps_the_promised_count(name, request_n, of, kept32, kept64, dtype):
    """The count lies within f5's limits (int)((T)target * (T)(1 -/+ tol)). The counts listed are what the restatement gives with this seed,
    row for row what greedy_target of tests/test_gpu_poisson_disk.py keeps: for the request of 64 at oversampling 1.5 (96 candidates) that
    is 61 on the bunny and 62 on cube_twist, inside [61, 66]."""
    v, f = sc.golden_mesh(name, dtype)
    fi, bc, P, keep, n_c, _ = sc.sample_mesh_poisson_disk(v, f, request_n, SEED, greedy, oversampling_factor=of)
    if (of == 5.0 or n_c < 1000) and request_n < n_c:            # the radius search restated here is the one f5's tests restate
        assert np.array_equal(keep, greedy_target(P, request_n, SEED, 0.04))
    print(name, np.dtype(dtype).name, "request", request_n, "oversampling", of, "candidates", n_c, "kept", len(keep))
    assert n_c == math.ceil(of * request_n)
    lo, hi = sc.count_limits(request_n, 0.04, dtype)
    if dtype is np.float32:
        assert (lo, hi) == {1000: (960, 1040), 200: (192, 208), 64: (61, 66)}[request_n]
    assert lo <= len(keep) <= hi
    assert len(keep) == (kept32 if dtype is np.float32 else kept64)
    assert np.all(np.diff(keep) > 0) and len(fi) == len(bc) == len(keep)
    if of == 1.0:
        assert np.array_equal(keep, np.arange(n_c))


def test_candidate_count_follows_the_max_rule():
    assert sc.candidate_count(40.0, 1000, 0.0, 2 ** 40, 1.0) == 40_000
    assert sc.candidate_count(1.5, -1, 0.0, 2 ** 40, 1.0) == 2
    total = (2.0 ** 40 * 2.0 ** -36) * 0.5                       # 8
    n_est = math.ceil(total / (0.7 * math.pi * 0.1 * 0.1))
    assert sc.candidate_count(5.0, 10, 0.1, 2 ** 40, 0.5) == math.ceil(5.0 * n_est) and n_est > 10
    assert sc.candidate_count(5.0, 10 * n_est, 0.1, 2 ** 40, 0.5) == 50 * n_est
    with pytest.raises(ValueError, match="2\\^27-16"):
        sc.candidate_count(40.0, 10, 1e-6, 2 ** 40, 0.5)


# ---- host-side checks of the package: no GPU is touched
@pytest.fixture(scope="module")
def pcu():
    import point_cloud_utils_amd as m
    return m


def tri():
    return np.array([[0.0, 0, 0], [0, 1, 0], [1, 0, 0]]), np.array([[0, 1, 2]])


def test_names_are_public(pcu):
    for name in ("mesh_face_areas", "sample_mesh_random", "sample_mesh_poisson_disk"):
        assert name in pcu.__all__ and callable(getattr(pcu, name))


def test_dtype_and_shape_errors(pcu):
    v, f = tri()
    calls = [lambda v, f: pcu.mesh_face_areas(v, f), lambda v, f: pcu.sample_mesh_random(v, f, 10, 1), lambda v, f: pcu.sample_mesh_poisson_disk(v, f, 10, random_seed=1)]
    for call in calls:
        with pytest.raises(ValueError, match=r"Invalid scalar type \(int64\) for argument 'v'"):
            call(v.astype(np.int64), f)
        with pytest.raises(ValueError, match=r"Invalid scalar type \(float64\) for argument 'f'"):
            call(v, f.astype(np.float64))
        with pytest.raises(ValueError, match=r"Invalid scalar type \(int16\) for argument 'f'"):
            call(v, f.astype(np.int16))
        with pytest.raises(ValueError, match="Invalid input mesh with zero elements"):
            call(v, np.zeros((0, 3), dtype=np.int64))
        with pytest.raises(ValueError, match="Invalid input mesh with zero elements"):
            call(np.zeros((0, 3)), f)
        with pytest.raises(ValueError, match=r"Only 3D inputs are supported.*f.shape = \(100, 2\)"):
            call(v, np.zeros((100, 2), dtype=np.int64))
        with pytest.raises(ValueError, match="v must not contain NaN or infinite coordinates"):
            call(np.array([[0.0, 0, 0], [0, np.inf, 0], [1, 0, 0]]), f)
        with pytest.raises(ValueError, match=r"found a face index outside \[0, 3\)"):
            call(v, np.array([[0, 1, 3]]))
        with pytest.raises(ValueError, match=r"found a face index outside \[0, 3\)"):
            call(v, np.array([[0, -1, 2]]))


def test_random_checks_and_their_order(pcu):
    v, f = tri()
    for n in (0, -5):
        with pytest.raises(ValueError, match="^num_samples must be positive$"):
            pcu.sample_mesh_random(v, f, n)
    with pytest.raises(ValueError, match="Invalid scalar type"):                       # scalar types before num_samples
        pcu.sample_mesh_random(v.astype(np.int32), f, 0)
    with pytest.raises(ValueError, match="zero elements"):                             # the mesh before num_samples
        pcu.sample_mesh_random(v, np.zeros((0, 3), dtype=np.int64), 0)
    with pytest.raises(ValueError, match="num_samples must be positive"):              # num_samples before the host checks of the values
        pcu.sample_mesh_random(v, np.array([[0, 1, 7]]), 0)
    with pytest.raises(ValueError, match="2\\^27-16"):
        pcu.sample_mesh_random(v, f, 2 ** 27)
    for seed in (-1, 2 ** 32):
        with pytest.raises(ValueError, match="random_seed must be an unsigned 32-bit integer"):
            pcu.sample_mesh_random(v, f, 10, random_seed=seed)


def test_poisson_checks_and_their_order(pcu):
    v, f = tri()
    with pytest.raises(ValueError, match="^Cannot have both num_samples <= 0 and radius <= 0$"):
        pcu.sample_mesh_poisson_disk(v, f, 0)
    with pytest.raises(ValueError, match="Cannot have both"):                          # 1 before 2 and 3
        pcu.sample_mesh_poisson_disk(v, f, -1, radius=-1.0, sample_num_tolerance=0.0, oversampling_factor=0.5)
    for tol in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match=r"^sample_num_tolerance must be in \(0, 1\]$"):
            pcu.sample_mesh_poisson_disk(v, f, 10, sample_num_tolerance=tol, oversampling_factor=0.5)      # 2 before 3
    with pytest.raises(ValueError, match=r"sample_num_tolerance must be in \(0, 1\]"):
        pcu.sample_mesh_poisson_disk(v, f, 10, sample_num_tolerance=1e-60)             # 0 as a float32
    for of in (0.999, 0.0, -3.0, float("nan")):
        with pytest.raises(ValueError, match="^oversampling_factor must be >= 1.0$"):
            pcu.sample_mesh_poisson_disk(v, f, 10, oversampling_factor=of)
    with pytest.raises(ValueError, match="zero elements"):                             # the mesh before the function's own checks
        pcu.sample_mesh_poisson_disk(v, np.zeros((0, 3), dtype=np.int64), 0)
    with pytest.raises(ValueError, match="Cannot have both"):                          # ... which come before the host checks of the values
        pcu.sample_mesh_poisson_disk(v, np.array([[0, 1, 7]]), 0)
    with pytest.raises(ValueError, match="candidates: more than 2\\^27-16 rows"):
        pcu.sample_mesh_poisson_disk(v, f, 2 ** 23, random_seed=1)                     # 40 x 2^23 candidates
    with pytest.raises(ValueError, match="2\\^27-16"):
        pcu.sample_mesh_poisson_disk(v, f, 2 ** 27, random_seed=1)


def test_no_cpu_fallback_without_gpu(pcu):
    from point_cloud_utils_amd import _lib
    if _lib.device_count() > 0:
        pytest.skip("GPU present")
    v, f = tri()
    for call in (lambda: pcu.mesh_face_areas(v, f), lambda: pcu.sample_mesh_random(v, f, 10, 1), lambda: pcu.sample_mesh_poisson_disk(v, f, 10, random_seed=1)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
