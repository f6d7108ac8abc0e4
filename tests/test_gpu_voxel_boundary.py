"""sparse_voxel_grid_boundary on the GPU (-m gpu) against the set restatement of tests/voxelize_contract.py: exact
integer semantics, so the rows are equal one by one."""
import numpy as np
import pytest

import voxelize_contract as vc
from test_voxelize_contract import voxels

pytestmark = pytest.mark.gpu

INT_DTYPES = [np.int32, np.int64, np.uint32, np.uint64]


@pytest.fixture(scope="module")
def pcu():
    import point_cloud_utils_amd as m
    from point_cloud_utils_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: the gfx950 path has no CPU fallback"
    return m


def to_torch(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check(pcu, ijk, what=""):
    want = vc.boundary(ijk)
    got = pcu.sparse_voxel_grid_boundary(ijk)
    assert got.dtype == np.int64 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    assert np.array_equal(got, want), what
    return want


def sparse_set(n, seed, side=12):
    """n rows drawn with repetition from a cube of side^3 cells around the origin: duplicated rows, inner and boundary voxels."""
    rng = np.random.default_rng(seed)
    return rng.integers(-side // 2, side - side // 2, (n, 3))


def test_solid_block(pcu):
    ijk = np.stack(np.meshgrid(np.arange(9), np.arange(7), np.arange(5), indexing="ij"), axis=-1).reshape(-1, 3).astype(np.int32) - 3
    assert len(check(pcu, ijk)) == 315 - 105
    perm = np.random.default_rng(1).permutation(len(ijk))
    check(pcu, ijk[perm], "shuffled")


def test_random_sparse_set_with_duplicated_rows(pcu):
    ijk = sparse_set(3000, 2).astype(np.int64)
    assert len(np.unique(ijk, axis=0)) < len(ijk)
    want = check(pcu, ijk)
    assert 0 < len(want) < len(ijk)


def test_the_voxelized_bunny(pcu):
    ijk = np.array(voxels("bunny", 64))
    want = check(pcu, ijk)
    assert len(want) > 0
    got = pcu.sparse_voxel_grid_boundary(to_torch(ijk))
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("n", [511, 512, 513, 2047, 2048, 2049, 4095, 4096, 4097])
def test_sort_and_scan_tile_edges(pcu, n):
    """The wave tile (512 keys) and block tile (2048) of the library's radix sort, the tile of its scan (4096), and one row to either side."""
    check(pcu, sparse_set(n, n, side=16).astype(np.int32), n)


def test_single_row_and_all_inner_but_the_shell(pcu):
    check(pcu, np.array([[5, -7, 9]], dtype=np.int32))
    check(pcu, np.array([[0, 0, 0], [0, 0, 0]], dtype=np.int64))


def test_neighbours_beyond_the_range_are_absent(pcu):
    top, bottom = vc.RANGE - 1, -vc.RANGE
    # a full 3 x 3 x 3 block in each corner of the range: only a voxel whose six neighbours exist inside the range is inner
    blk = np.stack(np.meshgrid(np.arange(3), np.arange(3), np.arange(3), indexing="ij"), axis=-1).reshape(-1, 3)
    ijk = np.concatenate([blk + bottom, top - blk])
    want = check(pcu, ijk.astype(np.int32))
    assert len(want) == 2 * 26
    line = np.array([[top, 0, 0], [top - 1, 0, 0], [bottom, bottom, bottom], [0, top, top]])
    check(pcu, line.astype(np.int64), "lines at the ends")


@pytest.mark.parametrize("dt", INT_DTYPES)
def test_dtypes(pcu, dt):
    ijk = sparse_set(1500, 7)
    if np.dtype(dt).kind == "u":
        ijk = ijk + 6
    want = check(pcu, ijk.astype(dt), dt)
    if dt in (np.int32, np.int64):
        got = pcu.sparse_voxel_grid_boundary(to_torch(ijk.astype(dt)))
        assert np.array_equal(got.cpu().numpy(), want)


def test_coordinates_beyond_the_range_are_refused(pcu):
    ok = sparse_set(700, 3)
    for dt, val in ((np.int32, vc.RANGE), (np.int64, -vc.RANGE - 1), (np.uint64, 2 ** 31 + 5), (np.uint32, 2 ** 31 + 5)):
        bad = ok.copy() + (6 if np.dtype(dt).kind == "u" else 0)
        bad = bad.astype(dt)
        bad[333, 1] = val
        with pytest.raises(ValueError, match="Invalid vertex leads to an overflow integer"):
            pcu.sparse_voxel_grid_boundary(bad)
        if dt in (np.int32, np.int64):                       # (found on the device for a tensor)
            with pytest.raises(ValueError, match="Invalid vertex leads to an overflow integer"):
                pcu.sparse_voxel_grid_boundary(to_torch(bad))
    check(pcu, ok.astype(np.int32), "the context is as good as before")
