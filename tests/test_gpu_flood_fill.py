"""GPU tests of flood_fill_3d: exact equality with the restatement of tests/components_contract.py. The shapes are the smallest
at which each path of the kernels is taken: rows shorter and longer than a wave (64) and a block (256), runs that cross wave and block
boundaries, regions whose diameter is thousands of cells, many blocks hooking into one root."""
import time

import numpy as np
import pytest

import components_contract as cc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pcu():
    import point_cloud_utils_amd as m
    return m


def check(pcu, grid, seed, fill):
    before = grid.copy()
    got = pcu.flood_fill_3d(grid, seed, fill)
    want = cc.flood_fill(grid, seed, fill)
    assert isinstance(got, np.ndarray) and got.dtype == grid.dtype and got.shape == grid.shape and got.flags.c_contiguous
    assert np.array_equal(got, want, equal_nan=grid.dtype.kind == "f"), np.argwhere(got != want)[:5]
    assert np.array_equal(grid, before, equal_nan=grid.dtype.kind == "f") and got is not grid       # the input is never modified
    return got


def random_grid(shape, p, seed, dtype=np.int32):
    return (np.random.default_rng(seed).random(shape) < p).astype(dtype)


def test_a_single_cell(pcu):
    assert check(pcu, np.array([[[4]]], dtype=np.int32), (0, 0, 0), 9).tolist() == [[[9]]]


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_a_line_and_its_transposes(pcu, axis):
    line = np.ones(130, dtype=np.int64)
    line[70] = 0                                  # the fill stops here: 70 cells from one end, 59 from the other
    shape = [1, 1, 1]
    shape[axis] = 130
    g = line.reshape(shape)
    seed = [0, 0, 0]
    assert (check(pcu, g, seed, 5) == 5).sum() == 70
    seed[axis] = 129
    assert (check(pcu, g, seed, 5) == 5).sum() == 59
    seed[axis] = 70
    assert (check(pcu, g, seed, 5) == 5).sum() == 1


@pytest.mark.parametrize("shape", [(5, 7, 67), (3, 130, 2)])
def test_shapes_that_are_no_multiple_of_a_wave_or_block(pcu, shape):
    for p, s in ((0.7, 1), (0.5, 2)):
        g = random_grid(shape, p, s)
        for seed in np.argwhere(g == 1)[[0, -1]].tolist() + np.argwhere(g == 0)[[0]].tolist():
            check(pcu, g, seed, 3)
    assert (check(pcu, np.zeros(shape, dtype=np.float32), (0, 0, 0), 1.5) == 1.5).all()


def test_a_seed_at_each_corner(pcu):
    g = random_grid((6, 9, 70), 0.7, 3)
    for x in (0, 5):
        for y in (0, 8):
            for z in (0, 69):
                g[x, y, z] = 1
    for x in (0, 5):
        for y in (0, 8):
            for z in (0, 69):
                check(pcu, g, (x, y, z), 2)


def test_the_row_end_leak_is_not_reproduced(pcu):
    w = np.array([[[1, 0], [0, 1]]], dtype=np.int32)
    assert check(pcu, w, (0, 0, 1), 7).tolist() == [[[1, 7], [0, 1]]]
    assert cc.flood_fill(w, (0, 0, 1), 7, reference_offsets=True).tolist() == [[[1, 7], [7, 1]]]
    # every z row alternates value from its neighbouring rows: a row is a region of its own, and the reference's arithmetic would leak
    # from the end of one row to the start of the row after the next
    g = np.zeros((4, 4, 64), dtype=np.int32)
    g[(np.arange(4)[:, None] + np.arange(4)[None, :]) % 2 == 1] = 1
    for seed in ((0, 0, 0), (0, 1, 63), (3, 3, 10), (2, 1, 0)):
        out = check(pcu, g, seed, 9)
        assert (out == 9).sum() == 64 and (out[seed[0], seed[1]] == 9).all()


def test_a_checkerboard_changes_only_the_seed(pcu):
    x, y, z = np.meshgrid(np.arange(7), np.arange(9), np.arange(66), indexing="ij")
    g = ((x + y + z) % 2).astype(np.float64)
    for seed in ((0, 0, 0), (3, 4, 65), (6, 8, 64)):
        assert (check(pcu, g, seed, -1.0) == -1.0).sum() == 1


def test_a_uniform_grid_changes_every_cell(pcu):
    g = np.full((130, 130, 130), 3, dtype=np.int32)
    out = pcu.flood_fill_3d(g, (64, 1, 129), 8)
    assert out.shape == g.shape and out.dtype == g.dtype and (out == 8).all() and (g == 3).all()
    st = pcu.last_stats()
    assert st["n_queries"] == 130 ** 3 and st["n_escalated"] == 130 ** 3


def test_a_serpentine_corridor_takes_a_fixed_number_of_launches(pcu):
    g, seed, cells = cc.serpentine(33)
    assert cells > 9000
    want = cc.flood_fill(g, seed, 2)
    assert (want == 2).sum() == cells and not (want == 1).any()          # one region: the corridor is connected end to end
    cut = g.copy()
    cut[16, 16, 16] = 0                                                  # ... and it is a path: a wall half way leaves half of it
    assert abs(int((cc.flood_fill(cut, seed, 2) == 2).sum()) - cells // 2) < 40
    pcu.flood_fill_3d(g, seed, 2)                                        # (warm: the workspace)
    dt = float("inf")
    for _ in range(3):                                                   # the quickest of three: a busy host must not fail the test
        t0 = time.perf_counter()
        got = pcu.flood_fill_3d(g, seed, 2)
        dt = min(dt, time.perf_counter() - t0)
        assert np.array_equal(got, want)
    # four launches, 36k cells: well under a millisecond of GPU work. A launch per step of a frontier walk along 9,000 cells would take tens of
    # milliseconds at the very least; the bound leaves room for a loaded host.
    print(f"flood_fill_3d over the {cells}-cell corridor: {dt * 1e3:.3f} ms per call")
    assert dt < 0.02, dt


def test_only_the_seeds_region_changes(pcu):
    g = np.zeros((8, 8, 140), dtype=np.int64)
    g[1:3, 1:3, 5:135] = 4
    g[5:7, 5:7, 5:135] = 4
    out = check(pcu, g, (1, 1, 5), 6)
    assert (out == 6).sum() == 2 * 2 * 130 and (out == 4).sum() == 2 * 2 * 130
    out = check(pcu, g, (0, 0, 0), 6)
    assert (out == 6).sum() == g.size - 2 * 2 * 2 * 130 and (out == 4).sum() == 2 * 2 * 2 * 130


@pytest.mark.parametrize("s", [1, 2, 3])
@pytest.mark.parametrize("p", [0.55, 0.65, 0.75])
def test_random_occupancy(pcu, p, s):
    g = random_grid((40, 40, 40), p, 100 * s + int(p * 100))
    rng = np.random.default_rng(s)
    for value in (1, 0):
        cells = np.argwhere(g == value)
        check(pcu, g, cells[rng.integers(len(cells))].tolist(), 2)


@pytest.mark.parametrize("dtype", [np.int32, np.int64, np.float32, np.float64])
def test_every_dtype(pcu, dtype):
    g = random_grid((9, 10, 75), 0.7, 5, dtype) * 3
    check(pcu, g, np.argwhere(g == 3)[0].tolist(), -2)
    check(pcu, g, np.argwhere(g == 0)[0].tolist(), 2.75)                 # (truncated towards zero for the integer types)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_signed_zeros_and_a_nan_seed(pcu, dtype):
    g = np.zeros((3, 4, 70), dtype=dtype)
    g[:, :, ::3] = -0.0
    g[1, 2, 33] = np.nan
    g[2, :, :] = 1.0
    out = check(pcu, g, (0, 0, 0), 5.0)
    assert (out == 5.0).sum() == 2 * 4 * 70 - 1 and np.isnan(out[1, 2, 33])
    out = check(pcu, g, (1, 2, 33), 5.0)                                 # a NaN equals nothing: the copy comes back
    assert np.array_equal(out, g, equal_nan=True) and np.array_equal(np.signbit(out), np.signbit(g))


def test_fill_equal_to_the_seed_value(pcu):
    g = random_grid((5, 6, 70), 0.6, 6, np.float32)
    out = check(pcu, g, np.argwhere(g == 1)[0].tolist(), 1.0)
    assert np.array_equal(out, g)


def test_an_int64_fill_goes_through_double(pcu):
    g = np.zeros((2, 2, 3), dtype=np.int64)
    out = check(pcu, g, (1, 1, 1), 2 ** 53 + 1)
    assert (out == 2 ** 53).all()


def test_fortran_ordered_and_sliced_input(pcu):
    base = random_grid((12, 14, 150), 0.7, 7)
    f_ordered = np.asfortranarray(base[:6, :7, :75])
    assert f_ordered.flags.f_contiguous and not f_ordered.flags.c_contiguous
    sliced = base[1::2, ::2, 3::2]
    assert not sliced.flags.c_contiguous and not sliced.flags.f_contiguous
    for g in (f_ordered, sliced, sliced.transpose(2, 0, 1)):
        check(pcu, g, np.argwhere(g == 1)[0].tolist(), 2)


def test_device_resident_call(pcu):
    import torch
    g = random_grid((20, 21, 70), 0.7, 8)
    seed = np.argwhere(g == 1)[0].tolist()
    want = cc.flood_fill(g, seed, 2)
    for dtype in (torch.int32, torch.int64, torch.float32, torch.float64):
        t = torch.from_numpy(g).to(device="cuda", dtype=dtype)
        keep = t.clone()
        out = pcu.flood_fill_3d(t, seed, 2)
        assert out.is_cuda and out.device == t.device and out.dtype == dtype and tuple(out.shape) == g.shape
        assert np.array_equal(out.cpu().numpy(), want.astype(out.cpu().numpy().dtype)) and torch.equal(t, keep)
        assert out.data_ptr() != t.data_ptr()
    out = pcu.flood_fill_3d(t.permute(2, 0, 1), (seed[2], seed[0], seed[1]), 2)       # a non-contiguous tensor
    assert np.array_equal(out.cpu().numpy(), want.transpose(2, 0, 1).astype(np.float64))
    with pytest.raises(ValueError, match="CUDA/HIP"):
        pcu.flood_fill_3d(torch.zeros((2, 2, 2)), (0, 0, 0), 1)


def test_shell_plus_unreached_cells_is_the_solid(pcu):
    """voxelize_triangle_mesh gives the shell; what a flood fill from an outside corner does not reach, and is not shell, is the interior."""
    v, f = cc.golden_mesh("bunny")
    size = (v.max(axis=0) - v.min(axis=0)).max() / 64
    ijk = pcu.voxelize_triangle_mesh(v, f, size, v.min(axis=0))
    lo = ijk.min(axis=0)
    dense = np.zeros(tuple(ijk.max(axis=0) - lo + 3), dtype=np.int32)
    dense[tuple((ijk - lo + 1).T)] = 1
    out = pcu.flood_fill_3d(dense, (0, 0, 0), 2)
    want = cc.flood_fill(dense, (0, 0, 0), 2)
    assert np.array_equal(out, want)
    interior = int((out == 0).sum())
    assert interior > 0 and interior == int((want == 0).sum()) and (out == 1).sum() == len(ijk)
