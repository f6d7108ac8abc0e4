"""GPU tests of connected_components: exact equality with the restatement of tests/components_contract.py on small meshes that
take every path of the code -- one block and up to 45, permuted strips of 4,096 triangles, root scans across one tile boundary, every face
dtype. Nothing here is contended: the largest launch is 45 workgroups. Hooks from every CU onto one word, and a million faces per call, are in
tests/test_gpu_components_scale.py."""
import functools

import numpy as np
import pytest

import components_contract as cc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pcu():
    import point_cloud_utils_amd as m
    return m


def verts(n, dtype=np.float64):
    return np.zeros((n, 3), dtype=dtype)


def check(pcu, nv, f, dtype=np.int64, vdtype=np.float64):
    f = np.asarray(f).astype(dtype)
    got = pcu.connected_components(verts(nv, vdtype), f)
    want = cc.components(nv, f)
    for g, w, name in zip(got, want, ("cv", "nv", "cf", "nf")):
        assert isinstance(g, np.ndarray) and g.dtype == f.dtype and g.ndim == 1, name
        assert np.array_equal(g.astype(np.int64), w), name
    return got


def strip(n_tri, seed):
    """A triangle strip (n_tri + 2 vertices in one component) with vertex ids and face order permuted."""
    rng = np.random.default_rng(seed)
    i = np.arange(n_tri)
    f = np.stack([i, i + 1, i + 2], axis=1)
    return rng.permutation(n_tri + 2)[f][rng.permutation(n_tri)]


def soup(n_tri, seed):
    """n_tri disjoint triangles with permuted vertex ids."""
    rng = np.random.default_rng(seed)
    return rng.permutation(3 * n_tri).reshape(n_tri, 3)


@functools.lru_cache(maxsize=None)
def doubled_bunny():
    v, f = cc.doubled(*cc.golden_mesh("bunny"))
    want = cc.components(len(v), f)
    for a in want:
        a.setflags(write=False)
    return v, f, want


def test_one_face(pcu):
    cv, nv, cf, nf = check(pcu, 3, [[0, 1, 2]])
    assert cv.tolist() == [0, 0, 0] and nv.tolist() == [3] and cf.tolist() == [0] and nf.tolist() == [1]


def test_two_disjoint_faces(pcu):
    cv, nv, cf, nf = check(pcu, 6, [[3, 4, 5], [0, 1, 2]])
    assert cv.tolist() == [0, 0, 0, 1, 1, 1] and cf.tolist() == [1, 0] and nv.tolist() == [3, 3] and nf.tolist() == [1, 1]


def test_two_faces_sharing_one_vertex(pcu):
    cv, nv, cf, nf = check(pcu, 5, [[0, 1, 2], [2, 3, 4]])
    assert nv.tolist() == [5] and nf.tolist() == [2]


def test_a_face_with_a_repeated_index(pcu):
    check(pcu, 4, [[1, 1, 3], [2, 2, 2], [0, 3, 0]])


def test_unreferenced_vertices_at_the_start_in_the_middle_and_at_the_end(pcu):
    cv, nv, cf, nf = check(pcu, 12, [[2, 3, 4], [7, 8, 9], [4, 2, 3]])
    assert cv.tolist() == [0, 1, 2, 2, 2, 3, 4, 5, 5, 5, 6, 7] and nf.tolist() == [0, 0, 2, 0, 0, 1, 0, 0]


def test_a_long_permuted_strip_is_one_component(pcu):
    f = strip(4096, 3)
    cv, nv, cf, nf = check(pcu, 4098, f)
    assert nv.tolist() == [4098] and nf.tolist() == [4096]
    check(pcu, 4098 + 700, f)                     # ... followed by singletons: the root scan crosses its tile (4096)


def test_many_components_with_permuted_ids(pcu):
    cv, nv, cf, nf = check(pcu, 9000, soup(3000, 4))
    assert len(nv) == 3000 and (nv == 3).all() and (nf == 1).all()


def test_the_doubled_bunny(pcu):
    v, f, want = doubled_bunny()
    got = pcu.connected_components(v, f)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    assert len(got[1]) == 2 and got[1].sum() == v.shape[0] and got[3].sum() == f.shape[0]


@pytest.mark.parametrize("vdtype", [np.float32, np.float64])
@pytest.mark.parametrize("fdtype", [np.int32, np.int64, np.uint32, np.uint64])
def test_every_dtype(pcu, fdtype, vdtype):
    f = np.concatenate([strip(300, 5), soup(100, 6) + 302])
    check(pcu, 302 + 300 + 5, f, fdtype, vdtype)


def test_coordinates_are_never_read(pcu):
    v = np.full((6, 3), np.nan)
    v[1] = np.inf
    cv, nv, cf, nf = pcu.connected_components(v, np.array([[0, 1, 2], [3, 4, 5]]))
    assert cv.tolist() == [0, 0, 0, 1, 1, 1]


@pytest.mark.parametrize("fdtype", ["int32", "int64"])
def test_device_resident_call(pcu, fdtype):
    import torch
    f = np.concatenate([strip(2000, 7), soup(500, 8) + 2002])
    nv = 2002 + 1500 + 3
    tv = torch.zeros((nv, 3), dtype=torch.float32, device="cuda")
    tf = torch.from_numpy(f).to(device="cuda", dtype=getattr(torch, fdtype))
    got = pcu.connected_components(tv, tf)
    want = cc.components(nv, f)
    for g, w in zip(got, want):
        assert g.is_cuda and g.device == tf.device and g.dtype == tf.dtype and g.dim() == 1
        assert np.array_equal(g.cpu().numpy().astype(np.int64), w)
    with pytest.raises(ValueError, match="same device"):
        pcu.connected_components(tv, f)


def test_out_of_range_face_indices_raise(pcu):
    import torch
    with pytest.raises(ValueError, match=r"found a face index outside \[0, 5\)"):
        pcu.connected_components(verts(5), np.array([[0, 1, 2], [2, 3, 5]]))
    tv = torch.zeros((5, 3), dtype=torch.float64, device="cuda")
    for bad in ([[0, 1, 2], [2, 3, 5]], [[0, -1, 2], [2, 3, 4]]):           # (device-resident faces are checked on the device)
        with pytest.raises(ValueError, match=r"found a face index outside \[0, 5\)"):
            pcu.connected_components(tv, torch.tensor(bad, device="cuda"))
    cv, nv, cf, nf = pcu.connected_components(tv, torch.tensor([[0, 1, 2], [2, 3, 4]], device="cuda"))      # the context works on
    assert cv.tolist() == [0] * 5 and nv.tolist() == [5]


def test_equal_calls_give_equal_bytes(pcu):
    f = np.concatenate([strip(4096, 9), soup(1000, 10) + 4098])
    a = pcu.connected_components(verts(8000), f)
    b = pcu.connected_components(verts(8000), f)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    st = pcu.last_stats()
    assert st["n_queries"] == len(f) and st["n_escalated"] == len(a[1]) == 1 + 1000 + (8000 - 4098 - 3000)
