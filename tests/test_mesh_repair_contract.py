"""CPU tests of tests/mesh_repair_contract.py: the restatement against cases small enough to check by eye, its properties
on every mesh the GPU tests use, and the argument checks of the four public calls, which are raised before the GPU is touched."""
import numpy as np
import pytest

import mesh_repair_contract as R


# ---------------------------------------------------------------------------------------------------- orient, by hand
def test_two_triangles_that_agree_stay():
    f = np.array([[0, 1, 2], [1, 0, 3]])                 # 0 -> 1 in the first, 1 -> 0 in the second
    o, p, tw = R.orient(f)
    assert o.tolist() == f.tolist() and p.tolist() == [0, 0] and tw == 0


def test_two_triangles_that_disagree_turn_the_second():
    f = np.array([[0, 1, 2], [0, 1, 3]])                 # 0 -> 1 in both
    o, p, tw = R.orient(f)
    assert o.tolist() == [[0, 1, 2], [3, 1, 0]] and p.tolist() == [0, 0] and tw == 0
    o, p, tw = R.orient(f[::-1].copy())                   # the smallest face keeps its row, whichever it is
    assert o.tolist() == [[0, 1, 3], [2, 1, 0]]


def test_tetrahedron_with_one_face_reversed():
    _, f = R.mesh("tetrahedron")
    assert R.orient(f)[0].tolist() == f.tolist()
    for k in (1, 2, 3):
        g = f.copy()
        g[k] = g[k, ::-1]
        o, p, tw = R.orient(g)
        assert o.tolist() == f.tolist() and p.tolist() == [0, 0, 0, 0] and tw == 0
    g = f.copy()
    g[0] = g[0, ::-1]                                     # the first face is the one that stays: the other three turn
    assert R.orient(g)[0].tolist() == f[:, ::-1].tolist()


def test_three_triangles_on_one_edge_are_three_patches():
    f = np.array([[0, 1, 2], [0, 1, 3], [0, 1, 4]])
    o, p, tw = R.orient(f)
    assert o.tolist() == f.tolist() and p.tolist() == [0, 1, 2] and tw == 0


def test_moebius_band_of_six_comes_back_unchanged():
    f = R.moebius(3)
    assert f.tolist() == [[0, 3, 1], [3, 4, 1], [1, 4, 2], [4, 5, 2], [2, 5, 3], [5, 0, 3]]
    assert len(R.manifold_edges(f)) == 6
    o, p, tw = R.orient(f)
    assert o.tolist() == f.tolist() and p.tolist() == [0] * 6 and tw == 1
    g = R.reverse_some(f, 1)
    assert R.orient(g)[0].tolist() == g.tolist() and R.orient(g)[2] == 1
    cut = f[:5]                                           # without its last face the band is a strip
    o, p, tw = R.orient(cut)
    assert tw == 0 and p.tolist() == [0] * 5 and R.check_orientation(cut, o, p) == 0


def test_a_face_that_lists_a_vertex_twice_has_no_edges():
    f = np.array([[0, 0, 1], [0, 1, 2], [0, 1, 3], [3, 3, 3]])
    o, p, tw = R.orient(f)
    assert o.tolist() == [[0, 0, 1], [0, 1, 2], [3, 1, 0], [3, 3, 3]] and p.tolist() == [0, 1, 1, 2] and tw == 0
    assert sorted(R.manifold_edges(f)) == [(0, 1)]


def test_closed_book_is_one_sphere_per_page():
    f = R.closed_book(6)
    o, p, tw = R.orient(R.reverse_some(f, 2))
    assert tw == 0 and p.tolist() == np.repeat(np.arange(6), 4).tolist()
    assert R.check_orientation(R.reverse_some(f, 2), o, p) == 0
    assert R.orient(f)[0].tolist() == f.tolist()          # as generated it is oriented


# ---------------------------------------------------------------------------------------------------- orient, on every mesh
@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("name", R.MESH_NAMES)
def test_orient_properties(name, seed):
    _, f = R.mesh(name)
    g = R.reverse_some(f, seed) if seed else f
    o, p, tw = R.orient(g)
    assert o.dtype == g.dtype and p.dtype == g.dtype and o.shape == g.shape and p.shape == (len(g),)
    assert R.check_orientation(g, o, p) == tw
    assert np.array_equal(p, R.patches_by_scipy(g))
    i, j, same = R.manifold_pairs(g)
    assert len(i) == len(R.manifold_edges(g))


def test_orient_next_to_a_moebius_band():
    _, sphere = R.mesh("tetrahedron")
    f = np.concatenate([R.moebius(5), R.reverse_some(sphere, 3) + 10, R.moebius(4, 20)])
    o, p, tw = R.orient(f)
    assert tw == 2 and p.tolist() == [0] * 10 + [1] * 4 + [2] * 8
    assert o[:10].tolist() == f[:10].tolist() and o[14:].tolist() == f[14:].tolist()
    assert R.check_orientation(f, o, p) == 2


def test_strips_are_one_patch():
    for n in (1, 2, 63, 64, 65, 257):
        f = R.strip(n)
        o, p, tw = R.orient(f)
        assert tw == 0 and not p.any() and R.check_orientation(f, o, p) == 0
        assert np.array_equal(o[1::2], f[1::2, ::-1]) and np.array_equal(o[0::2], f[0::2])


# ---------------------------------------------------------------------------------------------------- the three vertex calls
def test_remove_mesh_vertices_by_hand():
    v = np.arange(15, dtype=np.float64).reshape(5, 3)
    f = np.array([[0, 1, 2], [2, 3, 4], [4, 2, 0]], dtype=np.int32)
    vo, fo = R.remove_mesh_vertices(v, f, np.array([True, False, True, True, True]))
    assert vo.tolist() == v[[0, 2, 3, 4]].tolist() and fo.tolist() == [[1, 2, 3], [3, 1, 0]] and fo.dtype == np.int32
    vo, fo = R.remove_mesh_vertices(v, f, np.zeros(5, dtype=bool))
    assert vo.shape == (0, 3) and fo.shape == (0, 3)
    vo, fo = R.remove_mesh_vertices(v, f, np.array([[True], [True], [False], [True], [True]]))
    assert vo.shape == (4, 3) and fo.shape == (0, 3)


def test_remove_unreferenced_by_hand():
    v = np.arange(18, dtype=np.float32).reshape(6, 3)
    f = np.array([[4, 1, 2], [2, 1, 4]], dtype=np.uint32)
    vn, fn, cv, cf = R.remove_unreferenced(v, f)
    assert vn.tolist() == v[[1, 2, 4]].tolist() and fn.tolist() == [[2, 0, 1], [1, 0, 2]]
    assert cv.tolist() == [1, 2, 4] and cf.tolist() == [2 ** 32 - 1, 0, 1, 2 ** 32 - 1, 2, 2 ** 32 - 1]
    assert fn.dtype == cv.dtype == cf.dtype == np.uint32


@pytest.mark.parametrize("name", R.MESH_NAMES)
def test_remove_unreferenced_keeps_every_corner_bitwise(name):
    v, f = R.mesh(name)
    v, f, ids = R.with_unreferenced(v, f, 5)
    v[0, 0], v[1, 1] = np.nan, -0.0
    vn, fn, cv, cf = R.remove_unreferenced(v, f)
    assert vn[fn].tobytes() == v[f].tobytes() and vn.tobytes() == v[cv].tobytes()
    gone = np.flatnonzero(cf == -1)
    assert set(ids.tolist()) <= set(gone.tolist()) and len(vn) + len(gone) == len(v)
    assert np.array_equal(cf[cv], np.arange(len(vn))) and (np.diff(cv) > 0).all()


@pytest.mark.parametrize("name", ["tetrahedron", "sphere258", "fan700", "bunny"])
def test_welded_soup_is_the_mesh_again(name):
    v, f = R.S.mesh(name)
    assert len(np.unique(v, axis=0)) == len(v)
    sv, sf = R.soup(v, f)
    vo, fo, svi, svj = R.dedup_mesh(sv, sf, 0.0)
    order = np.lexsort((v[:, 2], v[:, 1], v[:, 0]))      # the stated vertex order: lexicographic
    assert np.array_equal(vo, v[order])
    rank = np.empty(len(v), dtype=np.int64)
    rank[order] = np.arange(len(v))
    assert np.array_equal(fo, rank[f]) and vo[fo].tobytes() == v[f].tobytes()
    assert np.array_equal(sv[svi], vo) and np.array_equal(vo[svj], sv)
    first = np.full(len(vo), len(sv))
    np.minimum.at(first, svj, np.arange(len(sv)))
    assert np.array_equal(first, svi)


def test_dedup_mesh_drops_faces_whose_corners_meet():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1.04, 0, 0], [0, 0, 1]], dtype=np.float32)
    f = np.array([[0, 1, 2], [1, 3, 4], [0, 3, 2], [4, 4, 0]])
    vo, fo, svi, svj = R.dedup_mesh(v, f, 0.1)
    assert svj.tolist() == [0, 3, 2, 3, 1] and svi.tolist() == [0, 4, 2, 1]
    assert fo.tolist() == [[0, 3, 2], [0, 3, 2]] and vo.tolist() == v[[0, 4, 2, 1]].tolist()
    vo, fo, svi, svj = R.dedup_mesh(v, f, 0.0)
    assert len(vo) == 5 and fo.tolist() == svj[f[:3]].tolist()


# ---------------------------------------------------------------------------------------------------- the public calls' argument checks
def test_public_calls_validate_before_touching_the_gpu():
    import point_cloud_utils_amd as pcu
    v = np.zeros((4, 3))
    f = np.array([[0, 1, 2], [1, 2, 3]])
    keep = np.ones(4, dtype=bool)
    for call in (lambda v, f: pcu.remove_mesh_vertices(v, f, keep), pcu.remove_unreferenced_mesh_vertices, lambda v, f: pcu.deduplicate_mesh_vertices(v, f, 0.0)):
        with pytest.raises(ValueError, match=r"Invalid scalar type \(int64\) for argument 'v'"):
            call(v.astype(np.int64), f)
        with pytest.raises(ValueError, match=r"Invalid scalar type \(float64\) for argument 'f'"):
            call(v, f.astype(np.float64))
        with pytest.raises(ValueError, match="Invalid input mesh with zero elements"):
            call(v[:0], f)
        with pytest.raises(ValueError, match="Invalid input mesh with zero elements"):
            call(v, f[:0])
        with pytest.raises(ValueError, match="Only 3D inputs are supported"):
            call(v[:, :2], f)
        with pytest.raises(ValueError, match=r"f must hold row indices of v: found a face index outside \[0, 4\)"):
            call(v, f + 2)
        with pytest.raises(ValueError, match=r"found a face index outside \[0, 4\)"):
            call(v, f - 1)
    for call in (lambda v, f: pcu.remove_mesh_vertices(v, f, keep), lambda v, f: pcu.deduplicate_mesh_vertices(v, f, 0.0)):
        with pytest.raises(ValueError, match=r"Invalid scalar type \(uint32\) for argument 'f'. Expected one of \['int32', 'int64'\]"):
            call(v, f.astype(np.uint32))
    with pytest.raises(ValueError, match="^mask should have the same number of rows as v$"):
        pcu.remove_mesh_vertices(v, f, keep[:3])
    with pytest.raises(ValueError, match="^mask should have only one column$"):
        pcu.remove_mesh_vertices(v, f, np.ones((4, 2), dtype=bool))
    with pytest.raises(ValueError, match=r"Invalid scalar type \(uint8\) for argument 'mask'"):
        pcu.remove_mesh_vertices(v, f, keep.astype(np.uint8))


def test_orient_mesh_faces_validates_before_touching_the_gpu():
    import point_cloud_utils_amd as pcu
    f = np.array([[0, 1, 2], [1, 2, 3]])
    with pytest.raises(ValueError, match=r"Invalid scalar type \(float32\) for argument 'f'"):
        pcu.orient_mesh_faces(f.astype(np.float32))
    with pytest.raises(ValueError, match="Invalid input faces with zero elements"):
        pcu.orient_mesh_faces(f[:0])
    with pytest.raises(ValueError, match="Only triangle inputs are supported"):
        pcu.orient_mesh_faces(f[:, :2])
    with pytest.raises(ValueError, match=r"f must hold row indices of v: found a face index outside \[0, 3\)"):
        pcu.orient_mesh_faces(f - 1)
    with pytest.raises(ValueError, match=r"face indices above 2\^31-17 are not supported"):
        pcu.orient_mesh_faces(f.astype(np.uint64) + np.uint64(2 ** 40))


def test_the_four_calls_are_exported():
    import point_cloud_utils_amd as pcu
    for name in ("remove_mesh_vertices", "remove_unreferenced_mesh_vertices", "deduplicate_mesh_vertices", "orient_mesh_faces"):
        assert name in pcu.__all__ and callable(getattr(pcu, name))
