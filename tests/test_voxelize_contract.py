"""CPU tests of the voxel contract's restatement (tests/voxelize_contract.py) and of the host-side checks of
voxelize_triangle_mesh, sparse_voxel_grid_boundary and voxel_grid_geometry. The overlap test is held to the recorded verdicts of the
reference's own function (tests/golden/voxelize/tribox_verdicts.npz, made by tests/golden/make_golden_tribox.py); the counts pinned below were found
with the restatement on the golden meshes."""
import functools
import os

import numpy as np
import pytest

import voxelize_contract as vc

MESHES = ["bunny", "cube_twist"]
# rows of voxelize() and of voxelize(x_first_only=True) -- the reference's loop -- at 3, 16 and 64 voxels across
PINNED = {"bunny": {3: (36, 28), 16: (958, 745), 64: (15277, 3388)}, "cube_twist": {3: (55, 55), 16: (1502, 1243), 64: (24016, 7870)}}


def grid_for(v, across):
    """`across` voxels along the longest axis, sizes scaled by (1, 0.7, 1.3), origin min - size / 4."""
    v = np.asarray(v, dtype=np.float64)
    size = (v.max(axis=0) - v.min(axis=0)).max() / across * np.array([1.0, 0.7, 1.3])
    return size, v.min(axis=0) - size / 4


@functools.lru_cache(maxsize=None)
def voxels(name, across, x_first_only=False):
    v, f = vc.golden_mesh(name, np.float64)
    size, origin = grid_for(v, across)
    out = vc.voxelize(v, f, size, origin, x_first_only=x_first_only)
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("family", ["lattice", "random"])
def test_tribox_equals_the_recorded_verdicts(family):
    z = np.load(os.path.join(vc.GOLDEN, "voxelize", "tribox_verdicts.npz"))
    want = z[family + "_verdict"].astype(bool)
    assert want.shape == (4000,) and 0 < want.sum() < 4000
    got = vc.tribox(z[family + "_centre"], z[family + "_half"], z[family + "_tri"].reshape(-1, 3, 3))
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]


def test_tribox_counts_touching_and_degenerate_triangles():
    half = np.array([0.5, 0.5, 0.5])
    tri = np.array([[[0.5, -1.0, -1.0], [0.5, 1.0, -1.0], [0.5, 0.0, 2.0]],          # in the plane of a face of the box
                    [[0.5 + 2.0 ** -40, -1.0, -1.0], [0.5 + 2.0 ** -40, 1.0, -1.0], [0.5 + 2.0 ** -40, 0.0, 2.0]],      # ... just off it
                    [[0.5, 0.5, 0.5], [0.5, 0.5, 0.5], [0.5, 0.5, 0.5]],              # a point on a corner
                    [[0.6, 0.6, 0.6], [0.6, 0.6, 0.6], [0.6, 0.6, 0.6]],              # a point outside
                    [[-2.0, 0.0, 0.0], [0.0, 0.0, 0.0], [2.0, 0.0, 0.0]]])           # a segment through the box
    assert vc.tribox(np.zeros((5, 3)), half, tri).tolist() == [True, False, True, False, True]


@pytest.mark.parametrize("across", [3, 16, 64])
@pytest.mark.parametrize("name", MESHES)
def test_reference_rows_are_a_subset_and_counts_are_pinned(name, across):
    full, first = voxels(name, across), voxels(name, across, True)
    assert (len(full), len(first)) == PINNED[name][across]
    assert full.dtype == np.int32 and first.dtype == np.int32
    assert set(map(tuple, first.tolist())) <= set(map(tuple, full.tolist()))
    code = vc.morton(full)
    assert bool((code[1:] > code[:-1]).all())                  # each voxel once, ascending by Morton code


def test_morton_order_follows_signed_coordinates():
    ijk = np.array([[-1, -1, -1], [0, 0, 0], [-vc.RANGE, 0, 0], [vc.RANGE - 1, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
    c = [int(x) for x in vc.morton(ijk)]
    assert c[0] < c[1] < c[4] < c[5] < c[6] and c[2] < c[1] < c[3]


def test_boundary_of_a_solid_block_is_its_shell():
    ijk = np.stack(np.meshgrid(np.arange(9), np.arange(7), np.arange(5), indexing="ij"), axis=-1).reshape(-1, 3) - 3
    got = vc.boundary(ijk)
    inner = ((ijk[:, 0] > -3) & (ijk[:, 0] < 5) & (ijk[:, 1] > -3) & (ijk[:, 1] < 3) & (ijk[:, 2] > -3) & (ijk[:, 2] < 1))
    assert len(got) == 315 - 105 and np.array_equal(got, np.nonzero(~inner)[0])


def test_geometry_of_one_voxel_is_the_unit_cube():
    v, f = vc.geometry(np.array([[0, 0, 0]]))
    assert v.dtype == np.float32 and f.dtype == np.int32 and v.shape == (8, 3) and f.shape == (12, 3)
    assert np.array_equal(v, vc.UNIT.astype(np.float32)) and np.array_equal(f, vc.CUBE)
    # a closed, consistently oriented surface: every directed edge once, its reverse once
    edges = {(int(a), int(b)) for t in f for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0]))}
    assert len(edges) == 36 and all((b, a) in edges for a, b in edges)
    v2, f2 = vc.geometry(np.array([[0, 0, 0], [2, -1, 5]]), (0.5, 1.0, 2.0), (1.0, 2.0, 3.0), 0.1)
    assert np.array_equal(f2[12:], vc.CUBE + 8)
    assert np.allclose(v2[8:].min(axis=0), [1.0 + 2.05 * 0.5, 2.0 - 0.95, 3.0 + 5.05 * 2.0]) and np.allclose(v2[8:].max(axis=0), [1.0 + 2.95 * 0.5, 2.0 - 0.05, 3.0 + 5.95 * 2.0])


# ---- host-side checks of the package: no GPU is touched
@pytest.fixture(scope="module")
def pcu():
    import point_cloud_utils_amd as m
    return m


def tri():
    return np.array([[0.0, 0, 0], [0, 1, 0], [1, 0, 0]]), np.array([[0, 1, 2]])


def test_names_are_public(pcu):
    for name in ("voxelize_triangle_mesh", "sparse_voxel_grid_boundary", "voxel_grid_geometry"):
        assert name in pcu.__all__ and callable(getattr(pcu, name))


def test_voxelize_validates_before_touching_the_gpu(pcu):
    v, f = tri()
    with pytest.raises(ValueError, match="Invalid input mesh with zero elements"):
        pcu.voxelize_triangle_mesh(v, np.zeros((0, 3), dtype=np.int64), 0.1, (0, 0, 0))
    with pytest.raises(ValueError, match="Invalid input mesh with zero elements"):
        pcu.voxelize_triangle_mesh(np.zeros((0, 3)), f, 0.1, (0, 0, 0))
    with pytest.raises(ValueError, match=r"Only 3D inputs are supported.*f.shape = \(4, 2\)"):
        pcu.voxelize_triangle_mesh(v, np.zeros((4, 2), dtype=np.int64), 0.1, (0, 0, 0))
    with pytest.raises(ValueError, match=r"Invalid scalar type \(int64\) for argument 'v'"):
        pcu.voxelize_triangle_mesh(v.astype(np.int64), f, 0.1, (0, 0, 0))
    with pytest.raises(ValueError, match=r"Invalid scalar type \(float64\) for argument 'f'"):
        pcu.voxelize_triangle_mesh(v, f.astype(np.float64), 0.1, (0, 0, 0))
    for size in ((0.1, 0.1), (0.1, 0.1, 0.1, 0.1), np.ones((2, 3)), "abc"):
        with pytest.raises(ValueError, match="^Invalid shape$"):
            pcu.voxelize_triangle_mesh(v, f, size, (0, 0, 0))
    for origin in (0.0, (0, 0), np.zeros(4)):
        with pytest.raises(ValueError, match="^Invalid shape$"):
            pcu.voxelize_triangle_mesh(v, f, 0.1, origin)
    for size in (0.0, -1.0, (0.1, 0.0, 0.1), (0.1, 0.1, -0.1), float("nan")):
        with pytest.raises(ValueError, match="^Invalid voxel size$"):
            pcu.voxelize_triangle_mesh(v, f, size, (0, 0, 0))
    for size, origin in ((float("inf"), (0, 0, 0)), (0.1, (0, float("nan"), 0)), (0.1, (float("inf"), 0, 0))):
        with pytest.raises(ValueError, match="must be finite"):
            pcu.voxelize_triangle_mesh(v, f, size, origin)
    with pytest.raises(ValueError, match="v must not contain NaN or infinite coordinates"):
        pcu.voxelize_triangle_mesh(np.array([[0.0, 0, 0], [0, np.nan, 0], [1, 0, 0]]), f, 0.1, (0, 0, 0))
    with pytest.raises(ValueError, match=r"found a face index outside \[0, 3\)"):
        pcu.voxelize_triangle_mesh(v, np.array([[0, 1, 3]]), 0.1, (0, 0, 0))


def test_boundary_validates_before_touching_the_gpu(pcu):
    with pytest.raises(ValueError, match="^Invalid grid_coordinates has zero rows!$"):
        pcu.sparse_voxel_grid_boundary(np.zeros((0, 3), dtype=np.int32))
    with pytest.raises(ValueError, match=r"^Invalid shape for grid_coordinates must have shape \(N, 3\) but got \(5, 2\)$"):
        pcu.sparse_voxel_grid_boundary(np.zeros((5, 2), dtype=np.int64))
    with pytest.raises(ValueError, match=r"Invalid scalar type \(float64\) for argument 'grid_coordinates'"):
        pcu.sparse_voxel_grid_boundary(np.zeros((5, 3)))
    for bad in (np.array([[0, 0, 2 ** 20]], dtype=np.int32), np.array([[0, -2 ** 20 - 1, 0]], dtype=np.int64),
                np.array([[2 ** 31 + 5, 0, 0]], dtype=np.uint64), np.array([[0, 0, 2 ** 31 + 5]], dtype=np.uint32)):
        with pytest.raises(ValueError, match="Invalid vertex leads to an overflow integer"):
            pcu.sparse_voxel_grid_boundary(bad)


def test_geometry_validates_before_touching_the_gpu(pcu):
    ijk = np.zeros((4, 3), dtype=np.int32)
    with pytest.raises(ValueError, match=r"Invalid input point cloud with zero points.*Got points.shape =\(0, 3\)"):
        pcu.voxel_grid_geometry(np.zeros((0, 3), dtype=np.int32))
    with pytest.raises(ValueError, match=r"Only 3D inputs are supported.*Got points.shape =\(4, 2\)"):
        pcu.voxel_grid_geometry(np.zeros((4, 2), dtype=np.int32))
    with pytest.raises(ValueError, match=r"Invalid scalar type \(float32\) for argument 'ijk'"):
        pcu.voxel_grid_geometry(np.zeros((4, 3), dtype=np.float32))
    for size in (0.0, (1.0, -1.0, 1.0)):
        with pytest.raises(ValueError, match="^Voxel size must be positive$"):
            pcu.voxel_grid_geometry(ijk, size)
    with pytest.raises(ValueError, match="^Invalid shape$"):
        pcu.voxel_grid_geometry(ijk, (1.0, 1.0))
    with pytest.raises(ValueError, match="^Invalid shape$"):
        pcu.voxel_grid_geometry(ijk, 1.0, (0.0, 0.0, 0.0, 0.0))
    big = np.lib.stride_tricks.as_strided(np.zeros(3, dtype=np.int32), shape=(2 ** 28, 3), strides=(0, 4))      # (no memory behind it)
    with pytest.raises(ValueError, match="more than 2\\^31-1 vertices"):
        pcu.voxel_grid_geometry(big)


def test_no_cpu_fallback_without_gpu(pcu):
    from point_cloud_utils_amd import _lib
    if _lib.device_count() > 0:
        pytest.skip("GPU present")
    v, f = tri()
    ijk = np.zeros((4, 3), dtype=np.int32)
    for call in (lambda: pcu.voxelize_triangle_mesh(v, f, 0.1, (0, 0, 0)), lambda: pcu.sparse_voxel_grid_boundary(ijk), lambda: pcu.voxel_grid_geometry(ijk)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
