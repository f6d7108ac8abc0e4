"""sparse_voxel_grid_to_hex_mesh on the GPU (-m gpu) against the set / dict restatement of tests/marching_cubes_contract.py:
cubes equal row for row, vertices bit for bit."""
import numpy as np
import pytest

import marching_cubes_contract as mc

pytestmark = pytest.mark.gpu

INT_DTYPES = [np.int32, np.int64, np.uint32, np.uint64]
OVERFLOW = "Invalid vertex leads to an overflow integer"


@pytest.fixture(scope="module")
def pcu():
    import point_cloud_utils_amd as m
    from point_cloud_utils_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: the gfx950 path has no CPU fallback"
    return m


def to_torch(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check(pcu, ijk, size=1.0, origin=(0.0, 0.0, 0.0), dtype=np.float64, what=""):
    want_v, want_c = mc.hex_mesh(ijk, size, origin, dtype)
    v, c = pcu.sparse_voxel_grid_to_hex_mesh(ijk, size, origin, dtype)
    assert c.dtype == np.int64 and c.shape == want_c.shape and np.array_equal(c, want_c), what
    assert v.dtype == np.dtype(dtype) and v.shape == want_v.shape and v.tobytes() == want_v.tobytes(), what
    st = pcu.last_stats()
    assert st["n_queries"] == len(ijk) and st["n_escalated"] == len(v), (what, st)
    return v, c


def draw(n, side, seed):
    """n rows drawn with repetition from a box of side^3 cells around the origin."""
    rng = np.random.default_rng(seed)
    return rng.integers(-(side // 2), side - side // 2, (n, 3))


def test_rows_drawn_with_repetition_from_a_small_box(pcu):
    ijk = draw(5000, 12, 1).astype(np.int64)
    assert len(np.unique(ijk, axis=0)) < len(ijk)
    v, c = check(pcu, ijk, 0.25, (1.0, -2.0, 0.5))
    # every cube's eight vertices are the voxel's corners in the stated order: voxel ijk is centred on origin + ijk * size
    want = np.array([1.0, -2.0, 0.5]) + (ijk[:, None, :] + mc.CORNERS[None] - 0.5) * 0.25
    assert np.array_equal(v[c], want)


def test_forty_thousand_rows(pcu):
    ijk = draw(40000, 40, 2).astype(np.int32)
    v, c = check(pcu, ijk, (0.3, 0.7, 1.1), (0.1, 0.2, -0.3))
    want = np.array([0.1, 0.2, -0.3]) + (ijk[:, None, :].astype(np.float64) + mc.CORNERS[None] - 0.5) * np.array([0.3, 0.7, 1.1])
    assert np.abs(v[c] - want).max() < 1e-12              # (each axis uses its own size; the bits are the restatement's, checked above)
    tv, tc = pcu.sparse_voxel_grid_to_hex_mesh(to_torch(ijk), (0.3, 0.7, 1.1), (0.1, 0.2, -0.3))
    assert tv.is_cuda and tc.is_cuda and tv.cpu().numpy().tobytes() == v.tobytes() and np.array_equal(tc.cpu().numpy(), c)


def test_the_ends_of_the_range(pcu):
    lo, hi = -mc.RANGE, mc.RANGE - 2
    ijk = np.array([[lo, lo, lo], [hi, hi, hi], [lo, 0, hi], [hi, lo, 0], [0, 0, 0], [lo, lo, lo]])
    check(pcu, ijk.astype(np.int32), 0.5)
    check(pcu, ijk.astype(np.int64), 1.0, dtype=np.float32)
    for dt, val in ((np.int32, mc.RANGE - 1), (np.int64, -mc.RANGE - 1), (np.int64, mc.RANGE - 1), (np.uint32, mc.RANGE - 1), (np.uint64, 2 ** 63 + 5)):
        bad = draw(300, 8, 3) + 4
        bad = bad.astype(dt)
        bad[299, 2] = val
        with pytest.raises(ValueError, match=OVERFLOW):
            pcu.sparse_voxel_grid_to_hex_mesh(bad)
        if dt in (np.int32, np.int64):                       # (found on the device for a tensor)
            with pytest.raises(ValueError, match=OVERFLOW):
                pcu.sparse_voxel_grid_to_hex_mesh(to_torch(bad))
    check(pcu, draw(300, 8, 3), what="the context is as good as before")


@pytest.mark.parametrize("it", INT_DTYPES)
@pytest.mark.parametrize("out", [np.float32, np.float64])
def test_dtypes_and_sizes(pcu, it, out):
    ijk = draw(1500, 10, 4)
    if np.dtype(it).kind == "u":
        ijk = ijk + 5
    ijk = ijk.astype(it)
    v, c = check(pcu, ijk, 0.37, (0.1, 0.2, 0.3), out, "scalar size")
    check(pcu, ijk, (0.5, 0.25, 2.0), (-1.0, 0.0, 3.0), out, "a size per axis")
    check(pcu, ijk, np.array([0.1, 0.3, 0.7]), np.array([1e3, -1e3, 0.0]), out, "arrays")
    if it in (np.int32, np.int64):
        import torch
        tv, tc = pcu.sparse_voxel_grid_to_hex_mesh(to_torch(ijk), 0.37, (0.1, 0.2, 0.3), out)
        assert tv.dtype == (torch.float32 if out == np.float32 else torch.float64) and tc.dtype == torch.int64
        assert tv.cpu().numpy().tobytes() == v.tobytes() and np.array_equal(tc.cpu().numpy(), c)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 511, 512, 513])
def test_sort_and_scan_tile_edges(pcu, n):
    """8 n codes: the wave tile (512 keys) and block tile (2,048) of the sort and the tile of the scan (4,096), and one voxel to either side."""
    check(pcu, draw(n, 9, n).astype(np.int32), what=n)


def test_errors(pcu):
    ijk = draw(100, 6, 5)
    call = pcu.sparse_voxel_grid_to_hex_mesh
    with pytest.raises(ValueError, match="Invalid grid_coordinates has zero rows!"):
        call(ijk[:0])
    with pytest.raises(ValueError, match=r"Invalid shape for grid_coordinates must have shape \(N, 3\) but got \(100, 2\)"):
        call(ijk[:, :2])
    with pytest.raises(ValueError, match="Invalid scalar type \\(float64\\) for argument 'grid_coordinates'"):
        call(ijk.astype(np.float64))
    for size in ((1.0, 2.0), "x"):
        with pytest.raises(ValueError, match="Invalid shape"):
            call(ijk, size)
    with pytest.raises(ValueError, match="Invalid shape"):
        call(ijk, 1.0, (0.0, 0.0))
    for size in (0.0, -1.0, (1.0, 0.0, 1.0)):
        with pytest.raises(ValueError, match="Invalid voxel size"):
            call(ijk, size)
    with pytest.raises(ValueError, match="must be finite"):
        call(ijk, 1.0, (0.0, np.inf, 0.0))
    with pytest.raises(ValueError, match="Invalid dtype"):
        call(ijk, 1.0, (0.0, 0.0, 0.0), np.float16)


def test_two_equal_calls_give_equal_bytes(pcu):
    t = to_torch(draw(20000, 30, 6))
    a, b = pcu.sparse_voxel_grid_to_hex_mesh(t, 0.1), pcu.sparse_voxel_grid_to_hex_mesh(t, 0.1)
    assert a[0].cpu().numpy().tobytes() == b[0].cpu().numpy().tobytes() and a[1].cpu().numpy().tobytes() == b[1].cpu().numpy().tobytes()
