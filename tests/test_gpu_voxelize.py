"""voxelize_triangle_mesh on the GPU (-m gpu), row for row against the numpy restatement of the contract (tests/voxelize_contract.py;
DESIGN.md, row f12): the same rows, dtype and order. The shapes sit on the edges of the library's slices of candidate ranks (SLICE), of its
scan tile (TILE) and of its ballot words (64 ranks)."""
import functools

import numpy as np
import pytest

import voxelize_contract as vc
from test_voxelize_contract import grid_for

pytestmark = pytest.mark.gpu

FACE_DTYPES = [np.int32, np.int64, np.uint32, np.uint64]
SLICE = vc.SLICE              # 2048: candidate ranks per block of the test pass (csrc/voxelize.h: kVxSlice)
TILE = vc.SC_TILE             # 4096: the tile of the library's 64-bit inclusive scan (csrc/radix.h: kScTile)


@pytest.fixture(scope="module")
def pcu():
    import point_cloud_utils_amd as m
    from point_cloud_utils_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: the gfx950 path has no CPU fallback"
    return m


def to_torch(*arrays):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


def same(got, want, what=""):
    got = np.asarray(got)
    assert got.dtype == np.int32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    assert np.array_equal(got, want), (what, np.nonzero((got != want).any(axis=1))[0][:5])


def check(pcu, v, f, size, origin, what=""):
    want = vc.voxelize(v, f, size, origin)
    assert len(want) > 0
    same(pcu.voxelize_triangle_mesh(v, f, size, origin), want, what)
    return want


@functools.lru_cache(maxsize=None)
def mesh(name, dtype):
    return vc.golden_mesh(name, dtype)


def words_of(v, f, size, origin):
    """The verdicts of all candidates in rank order, as rows of 64 (the library's ballot words)."""
    _, _, yes = vc.kept_pairs(v, f, size, origin)
    pad = (-len(yes)) % 64
    return np.concatenate([yes, np.zeros(pad, dtype=bool)]).reshape(-1, 64)


def small_faces(cells, rng):
    """One tiny triangle strictly inside each unit cell: with size 1 and origin 0 it has exactly 2 x 2 x 2 candidates."""
    cells = np.asarray(cells, dtype=np.float64)
    v = (cells[:, None, :] + 0.3 + 0.4 * rng.random((len(cells), 3, 3))).reshape(-1, 3)
    return v, np.arange(3 * len(cells)).reshape(-1, 3)


def join(parts):
    vs, fs, base = [], [], 0
    for v, f in parts:
        vs.append(v); fs.append(f + base); base += len(v)
    return np.concatenate(vs), np.concatenate(fs)


# ---------------------------------------------------------------------------------------------------- 1. golden meshes
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("across", [16, 64])
@pytest.mark.parametrize("name", ["bunny", "cube_twist"])
def test_golden_meshes_equal_the_restatement(pcu, name, across, dtype):
    v, f = mesh(name, dtype)
    size, origin = grid_for(v, across)                     # anisotropic: (1, 0.7, 1.3)
    n_cand = vc.candidate_count(v, f, size, origin)
    assert 70_000 < n_cand < 450_000
    check(pcu, v, f, size, origin, (name, across, dtype))


@pytest.mark.parametrize("fdt", FACE_DTYPES)
def test_face_dtypes(pcu, fdt):
    v, f = mesh("bunny", np.float32)
    size, origin = grid_for(v, 16)
    same(pcu.voxelize_triangle_mesh(v, f.astype(fdt), size, origin), vc.voxelize(v, f, size, origin), fdt)


def test_origin_above_the_mesh_gives_negative_indices(pcu):
    v, f = mesh("bunny", np.float64)
    size, _ = grid_for(v, 16)
    origin = v.max(axis=0) + 3.25 * size
    want = check(pcu, v, f, size, origin)
    assert want.max() < 0
    same(pcu.voxelize_triangle_mesh(v, f, float(size[0]), tuple(origin)), vc.voxelize(v, f, size[0], origin), "a scalar size")


# ---------------------------------------------------------------------------------------------------- 2. slice edges
BIG_TRI = np.array([[0.1, 0.2, 0.3], [47.3, 5.1, 31.7], [3.3, 39.2, 12.9]])


def test_one_face_across_many_slices(pcu):
    """49 x 41 x 33 = 66,297 candidates of one face: every slice boundary falls inside it; most ballot words are empty."""
    f = np.array([[0, 1, 2]])
    lo, hi = vc.candidates(BIG_TRI, f, 1.0, (0, 0, 0))
    assert (hi - lo + 1).tolist() == [[49, 41, 33]]
    w = words_of(BIG_TRI, f, 1.0, (0.0, 0.0, 0.0))
    assert (~w.any(axis=1)).sum() > 100 and w.any()
    check(pcu, BIG_TRI, f, 1.0, (0.0, 0.0, 0.0))
    check(pcu, BIG_TRI.astype(np.float32), f, (1.0, 0.7, 1.3), (0.25, -0.5, 0.125))


@pytest.mark.parametrize("k", [SLICE // 8 - 1, SLICE // 8, SLICE // 8 + 1, TILE - 1, TILE, TILE + 1])
def test_faces_of_eight_candidates(pcu, k):
    """8k candidates at SLICE - 8, SLICE, SLICE + 8; k at the scan tile and one face to either side."""
    rng = np.random.default_rng(k)
    v, f = small_faces(rng.integers(-20, 20, (k, 3)), rng)
    lo, hi = vc.candidates(v, f, 1.0, (0, 0, 0))
    assert bool(((hi - lo + 1) == 2).all())
    check(pcu, v, f, 1.0, (0.0, 0.0, 0.0), k)


@pytest.mark.parametrize("before", [SLICE // 8, (SLICE - 64) // 8])
def test_slice_boundary_on_a_face_boundary(pcu, before):
    """`before` faces of 8 candidates, one of 4 x 4 x 4, ten more of 8: the large face starts on a slice's first candidate (before = 256) or
    ends on a slice's last (before = 248)."""
    rng = np.random.default_rng(before)
    a = small_faces(rng.integers(-9, 9, (before, 3)), rng)
    big = (np.array([[0.5, 0.4, 0.6], [2.5, 0.6, 2.4], [0.7, 2.6, 2.5]]), np.array([[0, 1, 2]]))
    b = small_faces(rng.integers(-9, 9, (10, 3)), rng)
    v, f = join([a, big, b])
    lo, hi = vc.candidates(v, f, 1.0, (0, 0, 0))
    C = np.cumsum((hi - lo + 1).prod(axis=1))
    assert C[before] - C[before - 1] == 64 and (C[before - 1] % SLICE == 0 or C[before] % SLICE == 0)
    check(pcu, v, f, 1.0, (0.0, 0.0, 0.0))


# ---------------------------------------------------------------------------------------------------- 3. ballot and emit edges
def test_full_and_empty_ballot_words(pcu):
    """A large triangle in the plane z = a voxel centre: one layer of candidates, whole words of 64 survivors next to whole words of none."""
    v = np.array([[0.0, 0.0, 0.0], [200.0, 0.0, 0.0], [0.0, 200.0, 0.0]])
    f = np.array([[0, 1, 2]])
    lo, hi = vc.candidates(v, f, 1.0, (0, 0, 0))
    assert (hi - lo + 1).tolist() == [[201, 201, 1]]
    w = words_of(v, f, 1.0, (0.0, 0.0, 0.0))
    assert w.all(axis=1).any() and (~w.any(axis=1)).any()
    want = check(pcu, v, f, 1.0, (0.0, 0.0, 0.0))
    assert bool((want[:, 2] == 0).all())


# ---------------------------------------------------------------------------------------------------- 4. touching and degenerate faces
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_lattice_aligned_mesh(pcu, dtype):
    """Vertices on multiples of size / 2 relative to the origin: nearly every verdict is decided by an equality."""
    rng = np.random.default_rng(11)
    size, origin = np.array([0.5, 0.25, 1.0]), np.array([0.25, -1.0, 3.0])
    v = (origin + rng.integers(-12, 13, (300, 3)) * (size / 2)).astype(dtype)
    f = rng.integers(0, 300, (700, 3))
    check(pcu, v, f, size, origin, dtype)


def test_degenerate_faces(pcu):
    rng = np.random.default_rng(12)
    v = rng.random((40, 3)) * 6.0
    v[30], v[31], v[32] = (1.0, 1.0, 1.0), (2.0, 2.0, 2.0), (4.0, 4.0, 4.0)            # collinear
    f = np.array([[0, 1, 1], [2, 2, 3], [4, 5, 4], [6, 6, 6], [30, 31, 32], [32, 30, 31], [7, 8, 9]])
    for size, origin in ((0.5, (0.0, 0.0, 0.0)), ((1.0, 0.5, 0.25), (0.5, 0.25, 0.125))):
        check(pcu, v, f, size, origin)
        for i in range(len(f)):
            check(pcu, v, f[i:i + 1], size, origin, i)


# ---------------------------------------------------------------------------------------------------- 5. range
def test_candidates_up_to_the_ends_of_the_range_are_accepted(pcu):
    top, bottom = float(vc.RANGE), -float(vc.RANGE)
    v = np.array([[top - 2.5, 0.2, 0.3], [top - 1.5, 0.4, 0.1], [top - 2.0, 0.7, 0.6],
                  [bottom + 0.5, 0.2, 0.3], [bottom + 1.5, 0.4, 0.1], [bottom + 0.75, 0.7, 0.6]])
    f = np.array([[0, 1, 2], [3, 4, 5]])
    lo, hi = vc.candidates(v, f, 1.0, (0, 0, 0))
    assert hi[0, 0] == vc.RANGE - 1 and lo[1, 0] == -vc.RANGE
    want = check(pcu, v, f, 1.0, (0.0, 0.0, 0.0))
    assert want[:, 0].min() <= -vc.RANGE + 1 and want[:, 0].max() >= vc.RANGE - 3


def test_a_candidate_beyond_the_range_is_refused(pcu):
    top = float(vc.RANGE)
    f = np.array([[0, 1, 2]])
    for v in (np.array([[top - 2.5, 0.2, 0.3], [top - 0.5, 0.4, 0.1], [top - 2.0, 0.7, 0.6]]),
              np.array([[0.2, -top - 0.5, 0.3], [0.1, -top + 0.5, 0.1], [0.3, -top + 0.75, 0.6]]),
              np.array([[0.0, 0.0, 0.0], [1e300, 0.0, 0.0], [0.0, 1.0, 0.0]])):
        with pytest.raises(ValueError, match=r"outside \[-2\^20, 2\^20\)"):
            pcu.voxelize_triangle_mesh(v, f, 1.0, (0.0, 0.0, 0.0))
    with pytest.raises(ValueError, match=r"outside \[-2\^20, 2\^20\)"):
        pcu.voxelize_triangle_mesh(np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]]), f, 1e-9, (0.0, 0.0, 0.0))


def test_too_many_candidates_are_refused_before_any_is_enumerated(pcu):
    """One face whose box holds 2001^3 > 2^32 candidates: refused from the extent pass's total."""
    v = np.array([[0.5, 0.5, 0.5], [1999.5, 1999.5, 0.5], [0.5, 1999.5, 1999.5]])
    f = np.array([[0, 1, 2]])
    with pytest.raises(ValueError, match=r"more than 2\^32 candidate voxels"):
        pcu.voxelize_triangle_mesh(v, f, 1.0, (0.0, 0.0, 0.0))
    check(pcu, v, f, 100.0, (0.0, 0.0, 0.0))             # (the context is as good as before)


# ---------------------------------------------------------------------------------------------------- 6. paths and errors
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_torch_on_device_equals_numpy(pcu, dtype):
    import torch
    v, f = mesh("bunny", dtype)
    size, origin = grid_for(v, 16)
    want = vc.voxelize(v, f, size, origin)
    for fdt in (np.int32, np.int64):
        got = pcu.voxelize_triangle_mesh(*to_torch(v, f.astype(fdt)), size, origin)
        assert got.is_cuda and got.dtype == torch.int32
        same(got.cpu().numpy(), want, fdt)


def test_equal_arguments_give_equal_bytes_and_other_calls_do_not_disturb(pcu):
    v, f = mesh("cube_twist", np.float32)
    size, origin = grid_for(v, 16)
    a = pcu.voxelize_triangle_mesh(v, f, size, origin)
    b = pcu.voxelize_triangle_mesh(v, f, size, origin)
    assert a.tobytes() == b.tobytes()
    pcu.estimate_point_cloud_normals_knn(v, 8)             # (uses the context's workspace and its auxiliary block)
    pcu.mesh_face_areas(v, f)
    c = pcu.voxelize_triangle_mesh(v, f, size, origin)
    assert a.tobytes() == c.tobytes()
    same(a, vc.voxelize(v, f, size, origin))


def test_bad_values_are_refused_on_the_device(pcu):
    v, f = mesh("bunny", np.float64)
    size, origin = grid_for(v, 16)
    bad_v = v.copy(); bad_v[17, 1] = np.inf
    bad_f = f.copy(); bad_f[100, 2] = len(v)
    with pytest.raises(ValueError, match="v must not contain NaN or infinite coordinates"):
        pcu.voxelize_triangle_mesh(*to_torch(bad_v, f), size, origin)
    with pytest.raises(ValueError, match=r"found a face index outside \[0, %d\)" % len(v)):
        pcu.voxelize_triangle_mesh(*to_torch(v, bad_f), size, origin)
    with pytest.raises(ValueError, match="v must not contain NaN or infinite coordinates"):
        pcu.voxelize_triangle_mesh(bad_v, f, size, origin)
    with pytest.raises(ValueError, match="found a face index outside"):
        pcu.voxelize_triangle_mesh(v, bad_f, size, origin)
