"""CPU tests of the restatements in tests/components_contract.py and of the host-side checks of connected_components and
flood_fill_3d: everything that raises before any device work is tested here, without a GPU."""
import numpy as np
import pytest

import components_contract as cc


# ---- connected_components: the label rule
def test_components_are_numbered_by_their_smallest_vertex():
    #            component of vertex 0 is {0, 5}, of vertex 1 {1, 3, 4, 6}, vertex 2 is unreferenced, 7..9 is the last one
    f = np.array([[7, 8, 9], [4, 6, 1], [5, 0, 5], [3, 4, 3]])
    cv, nv, cf, nf = cc.components(10, f)
    assert cv.tolist() == [0, 1, 2, 1, 1, 0, 1, 3, 3, 3]
    assert nv.tolist() == [2, 4, 1, 3] and cf.tolist() == [3, 1, 0, 1] and nf.tolist() == [1, 2, 0, 1]


def test_one_shared_vertex_joins_two_faces():
    cv, nv, cf, nf = cc.components(5, np.array([[0, 1, 2], [2, 3, 4]]))
    assert cv.tolist() == [0] * 5 and nv.tolist() == [5] and cf.tolist() == [0, 0] and nf.tolist() == [2]
    cv, nv, cf, nf = cc.components(6, np.array([[0, 1, 2], [3, 4, 5]]))
    assert cv.tolist() == [0, 0, 0, 1, 1, 1] and nv.tolist() == [3, 3] and cf.tolist() == [0, 1] and nf.tolist() == [1, 1]


def test_unreferenced_vertices_are_components_of_their_own():
    cv, nv, cf, nf = cc.components(7, np.array([[1, 2, 4]]))
    assert cv.tolist() == [0, 1, 1, 2, 1, 3, 4] and nv.tolist() == [1, 3, 1, 1, 1] and cf.tolist() == [1] and nf.tolist() == [0, 1, 0, 0, 0]


def test_the_bunny_is_one_component_and_the_doubled_bunny_two():
    v, f = cc.golden_mesh("bunny")
    cv, nv, cf, nf = cc.components(len(v), f)
    assert len(nv) == 1 and nv.tolist() == [len(v)] and nf.tolist() == [len(f)] and not cv.any() and not cf.any()
    v2, f2 = cc.doubled(v, f)
    cv, nv, cf, nf = cc.components(len(v2), f2)
    assert len(nv) == 2 and nv.sum() == v2.shape[0] and nf.sum() == f2.shape[0]
    assert nv.tolist() == [len(v)] * 2 and nf.tolist() == [len(f)] * 2
    assert np.array_equal(cv, np.repeat([0, 1], len(v))) and np.array_equal(cf, np.repeat([0, 1], len(f)))


# ---- flood_fill_3d: the two neighbour rules
WITNESS = np.array([[[1, 0], [0, 1]]], dtype=np.int32)


def test_the_row_end_leak_of_the_reference_is_not_the_contract():
    got = cc.flood_fill(WITNESS, (0, 0, 1), 7)
    assert got.tolist() == [[[1, 7], [0, 1]]] and got.dtype == np.int32
    ref = cc.flood_fill(WITNESS, (0, 0, 1), 7, reference_offsets=True)
    assert ref.tolist() == [[[1, 7], [7, 1]]]
    assert WITNESS.tolist() == [[[1, 0], [0, 1]]]


def test_both_rules_agree_where_the_region_touches_no_z_border():
    rng = np.random.default_rng(11)
    g = (rng.random((9, 8, 7)) < 0.6).astype(np.int64)
    g[:, :, 0] = 5
    g[:, :, -1] = 5
    seed = tuple(int(c) for c in np.argwhere(g == 1)[0])
    a, b = cc.flood_fill(g, seed, -3), cc.flood_fill(g, seed, -3, reference_offsets=True)
    assert np.array_equal(a, b) and (a == -3).sum() > 1 and (a == 1).sum() > 0


def test_fill_equal_to_the_seed_value_returns_the_copy():
    g = np.arange(24, dtype=np.float32).reshape(2, 3, 4) % 3
    out = cc.flood_fill(g, (1, 1, 1), g[1, 1, 1])
    assert np.array_equal(out, g) and out is not g


def test_nan_and_signed_zero_seeds():
    g = np.zeros((2, 2, 3), dtype=np.float64)
    g[0, 0, 1] = -0.0
    g[1, 1, 1] = np.nan
    out = cc.flood_fill(g, (0, 0, 0), 2.5)
    assert (out == 2.5).sum() == 11 and np.isnan(out[1, 1, 1])
    out = cc.flood_fill(g, (1, 1, 1), 2.5)
    assert np.array_equal(out, g, equal_nan=True) and np.signbit(out[0, 0, 1])


def test_the_fill_value_goes_through_double():
    g = np.zeros((1, 1, 2), dtype=np.int64)
    assert cc.flood_fill(g, (0, 0, 0), 2 ** 53 + 1).tolist() == [[[2 ** 53, 2 ** 53]]]
    assert cc.flood_fill(g.astype(np.int32), (0, 0, 0), 2.9).tolist() == [[[2, 2]]]


# ---- the fast restatements (scipy's labelling) are held to the plain ones, on inputs small enough for the plain ones
def same_components(nv, f):
    want, got = cc.components(nv, f), cc.components_fast(nv, f)
    for w, g, name in zip(want, got, ("cv", "nv", "cf", "nf")):
        assert g.dtype == np.int64 and g.ndim == 1 and np.array_equal(g, w), name
    return got


@pytest.mark.parametrize("nv", [7, 300, 2000, 5000])
def test_components_fast_on_random_face_soups(nv):
    f = np.random.default_rng(nv).integers(0, nv, (max(nv // 2, 1), 3))
    cv, cnv, cf, cnf = same_components(nv, f)
    assert cnv.sum() == nv and cnf.sum() == len(f) and 1 < len(cnv) < nv


def test_components_fast_on_the_rule_cases_and_the_doubled_bunny():
    same_components(10, np.array([[7, 8, 9], [4, 6, 1], [5, 0, 5], [3, 4, 3]]))
    same_components(5, np.array([[0, 1, 2], [2, 3, 4]]))
    same_components(6, np.array([[3, 4, 5], [0, 1, 2]]))
    v, f = cc.doubled(*cc.golden_mesh("bunny"))
    rng = np.random.default_rng(2)
    cv, cnv, cf, cnf = same_components(len(v), f)
    assert cnv.tolist() == [len(v) // 2] * 2 and cnf.tolist() == [len(f) // 2] * 2
    same_components(len(v), rng.permutation(len(v))[f][rng.permutation(len(f))])


def test_components_fast_with_unreferenced_vertices_at_both_ends():
    cv, cnv, cf, cnf = same_components(12, np.array([[2, 3, 4], [7, 8, 9], [4, 2, 3]]))
    assert cv.tolist() == [0, 1, 2, 2, 2, 3, 4, 5, 5, 5, 6, 7] and cnf.tolist() == [0, 0, 2, 0, 0, 1, 0, 0]
    same_components(7, np.array([[1, 2, 4]]))
    f = np.random.default_rng(3).integers(40, 160, (50, 3))
    cv, cnv, cf, cnf = same_components(200, f)
    assert (cnv[:40] == 1).all() and (cnv[-40:] == 1).all() and (cnf[:40] == 0).all()


def test_components_fast_with_repeated_indices_and_repeated_faces():
    same_components(4, np.array([[1, 1, 3], [2, 2, 2], [0, 3, 0]]))
    same_components(3, np.array([[0, 0, 0]]))
    same_components(6, np.array([[4, 4, 5], [5, 4, 4], [1, 2, 1]]))
    cv, cnv, cf, cnf = same_components(9, np.tile([[7, 8, 3]], (1000, 1)))        # one edge a thousand times: its weight must not wrap to none
    assert cnv.tolist() == [1, 1, 1, 3, 1, 1, 1] and cnf.tolist() == [0, 0, 0, 1000, 0, 0, 0]


def same_fill(grid, seed, fill):
    before = grid.copy()
    want, got = cc.flood_fill(grid, seed, fill), cc.flood_fill_fast(grid, seed, fill)
    assert got.dtype == grid.dtype and got.shape == grid.shape and got is not grid
    assert want.tobytes() == got.tobytes()                       # (bytes: signed zeros and NaNs included)
    assert grid.tobytes() == before.tobytes()
    return got


def test_flood_fill_fast_on_the_grids_of_the_tests_above():
    assert same_fill(WITNESS, (0, 0, 1), 7).tolist() == [[[1, 7], [0, 1]]]
    for seed in ((0, 0, 0), (0, 1, 0), (0, 1, 1)):
        same_fill(WITNESS, seed, 7)
    g = (np.random.default_rng(11).random((9, 8, 7)) < 0.6).astype(np.int64)
    g[:, :, 0] = 5
    g[:, :, -1] = 5
    for value in (0, 1, 5):
        same_fill(g, tuple(int(c) for c in np.argwhere(g == value)[0]), -3)
    g = np.arange(24, dtype=np.float32).reshape(2, 3, 4) % 3
    assert np.array_equal(same_fill(g, (1, 1, 1), g[1, 1, 1]), g)
    same_fill(g, (1, 1, 1), 8.5)
    g = np.zeros((1, 1, 2), dtype=np.int64)
    assert same_fill(g, (0, 0, 0), 2 ** 53 + 1).tolist() == [[[2 ** 53, 2 ** 53]]]
    assert same_fill(g.astype(np.int32), (0, 0, 0), 2.9).tolist() == [[[2, 2]]]
    with pytest.raises(ValueError, match="^seed point must be inside grid$"):
        cc.flood_fill_fast(g, (0, 0, 2), 1)


@pytest.mark.parametrize("p", [0.3, 0.5, 0.7])
def test_flood_fill_fast_on_random_grids_seeded_in_both_values(p):
    g = (np.random.default_rng(int(p * 10)).random((24, 24, 24)) < p).astype(np.int32)
    rng = np.random.default_rng(1)
    for value in (1, 0):
        cells = np.argwhere(g == value)
        for seed in (cells[0], cells[-1], cells[rng.integers(len(cells))]):
            out = same_fill(g, seed.tolist(), 2)
            assert 0 < (out == 2).sum() <= len(cells)


@pytest.mark.parametrize("dtype", [np.int32, np.int64, np.float32, np.float64])
def test_flood_fill_fast_in_every_dtype(dtype):
    g = (np.random.default_rng(5).random((9, 10, 11)) < 0.7).astype(dtype) * 3
    same_fill(g, np.argwhere(g == 3)[0].tolist(), -2)
    same_fill(g, np.argwhere(g == 0)[0].tolist(), 2.75)         # (truncated towards zero for the integer types)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_flood_fill_fast_with_signed_zeros_and_a_nan_seed(dtype):
    g = np.zeros((3, 4, 9), dtype=dtype)
    g[:, :, ::3] = -0.0
    g[1, 2, 4] = np.nan
    g[2, :, :] = 1.0
    out = same_fill(g, (0, 0, 0), 5.0)                           # -0.0 == 0.0: one region around the NaN
    assert (out == 5.0).sum() == 2 * 4 * 9 - 1 and np.isnan(out[1, 2, 4])
    out = same_fill(g, (0, 0, 1), 5.0)
    assert (out == 5.0).sum() == 2 * 4 * 9 - 1
    out = same_fill(g, (1, 2, 4), 5.0)                           # a NaN equals nothing: the copy comes back
    assert out.tobytes() == g.tobytes()


def test_the_serpentine_is_one_path():
    g, seed, cells = cc.serpentine(9)
    assert seed == (0, 0, 0) and cells == int(g.sum())
    out = same_fill(g, seed, 2)
    assert (out == 2).sum() == cells and not (out == 1).any()
    g[4, 4, 4] = 0
    assert 0 < (same_fill(g, seed, 2) == 2).sum() < cells


# ---- host-side checks of the package: no GPU is touched
@pytest.fixture(scope="module")
def pcu():
    import point_cloud_utils_amd as m
    return m


def tri():
    return np.array([[0.0, 0, 0], [0, 1, 0], [1, 0, 0]]), np.array([[0, 1, 2]])


def test_names_are_public(pcu):
    for name in ("connected_components", "flood_fill_3d"):
        assert name in pcu.__all__ and callable(getattr(pcu, name))


def test_connected_components_validates_before_touching_the_gpu(pcu):
    v, f = tri()
    with pytest.raises(ValueError, match="Invalid input mesh with zero elements"):
        pcu.connected_components(v, np.zeros((0, 3), dtype=np.int64))
    with pytest.raises(ValueError, match="Invalid input mesh with zero elements"):
        pcu.connected_components(np.zeros((0, 3)), f)
    with pytest.raises(ValueError, match=r"Only 3D inputs are supported.*f.shape = \(4, 2\)"):
        pcu.connected_components(v, np.zeros((4, 2), dtype=np.int64))
    with pytest.raises(ValueError, match=r"Invalid scalar type \(int64\) for argument 'v'"):
        pcu.connected_components(v.astype(np.int64), f)
    with pytest.raises(ValueError, match=r"Invalid scalar type \(float64\) for argument 'f'"):
        pcu.connected_components(v, f.astype(np.float64))
    with pytest.raises(ValueError, match=r"found a face index outside \[0, 3\)"):
        pcu.connected_components(v, np.array([[0, 1, 3]]))
    with pytest.raises(ValueError, match=r"found a face index outside \[0, 3\)"):
        pcu.connected_components(v, np.array([[0, -1, 2]], dtype=np.int32))
    with pytest.raises(ValueError, match=r"found a face index outside \[0, 3\)"):
        pcu.connected_components(v, np.array([[0, 1, 2 ** 40]], dtype=np.uint64))
    big = np.lib.stride_tricks.as_strided(np.zeros(3), shape=(2 ** 27, 3), strides=(0, 8))      # (no memory behind it)
    with pytest.raises(ValueError, match="more than 2\\^27-16 rows"):
        pcu.connected_components(big, f)


def test_flood_fill_validates_before_touching_the_gpu(pcu):
    g = np.zeros((3, 4, 5), dtype=np.int32)
    for coord in ((0, 0), (0, 0, 0, 0), 1, "abc", (0, 0.5, 0), (0, None, 0), np.zeros((2, 3)), (0, float("nan"), 0)):
        with pytest.raises(ValueError, match="^Invalid shape$"):
            pcu.flood_fill_3d(g, coord, 1)
    for bad in (np.zeros((3, 4), dtype=np.int32), np.zeros((3, 4, 5, 1), dtype=np.int32), np.zeros(5, dtype=np.int32)):
        with pytest.raises(ValueError, match=r"^grid must have shape \[w, h, d\]$"):
            pcu.flood_fill_3d(bad, (0, 0, 0), 1)
    for coord in ((3, 0, 0), (0, 4, 0), (0, 0, 5), (-1, 0, 0), (0, 0, -1), (2 ** 40, 0, 0)):
        with pytest.raises(ValueError, match="^seed point must be inside grid$"):
            pcu.flood_fill_3d(g, coord, 1)
    for shape in ((0, 4, 5), (3, 0, 5), (3, 4, 0)):
        with pytest.raises(ValueError, match="^seed point must be inside grid$"):
            pcu.flood_fill_3d(np.zeros(shape, dtype=np.float32), (0, 0, 0), 1)
    for dt in (np.uint32, np.int16, np.float16, bool, np.uint64):
        name = np.dtype(dt).name
        with pytest.raises(ValueError, match=rf"^Invalid scalar type \({name}\) for argument 'grid'. Expected one of \['int32', 'int64', 'float32', 'float64'\]\.$"):
            pcu.flood_fill_3d(g.astype(dt), (0, 0, 0), 1)
    big = np.lib.stride_tricks.as_strided(np.zeros(1, dtype=np.int32), shape=(2 ** 11, 2 ** 10, 2 ** 10), strides=(0, 0, 0))      # (no memory behind it)
    with pytest.raises(ValueError, match="more than 2\\^31-16 cells"):
        pcu.flood_fill_3d(big, (0, 0, 0), 1)
    with pytest.raises((TypeError, ValueError)):
        pcu.flood_fill_3d(g, (0, 0, 0), "x")


def test_no_cpu_fallback_without_gpu(pcu):
    from point_cloud_utils_amd import _lib
    if _lib.device_count() > 0:
        pytest.skip("GPU present")
    v, f = tri()
    for call in (lambda: pcu.connected_components(v, f), lambda: pcu.flood_fill_3d(np.zeros((2, 2, 2)), (0, 0, 0), 1.0)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
