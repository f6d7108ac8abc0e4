"""decimate_triangle_mesh on the GPU (-m gpu) against tests/decimate_contract.py: dtype, shape and bytes of all four
outputs; nothing takes a tolerance. The contract's answer is computed once per mesh and float type (a Decimation answers every max_faces
from the rounds it has kept) and shared; the face dtype only casts the three integer outputs."""
import functools

import numpy as np
import pytest

import decimate_contract as D

pytestmark = pytest.mark.gpu

FLOATS = ["float32", "float64"]
KINDS = [np.int32, np.int64, np.uint32, np.uint64]
SIGNED = [np.int32, np.int64]
EDGES = [1, 63, 64, 65, 255, 256, 257]


@pytest.fixture(scope="module")
def pcu():
    import point_cloud_utils_amd as m
    from point_cloud_utils_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: the gfx950 path has no CPU fallback"
    return m


def to_torch(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()          # (a copy: the shared cases are read-only)


def host(a):
    return a.cpu().numpy() if hasattr(a, "is_cuda") else a


def same(got, want, on_device=False):
    """dtype, shape and bytes; a tensor on the device where one is expected, else numpy."""
    if on_device:
        assert got.is_cuda, type(got)
    else:
        assert isinstance(got, np.ndarray), type(got)
    g = host(got)
    assert g.dtype == want.dtype and g.shape == want.shape, (g.dtype, want.dtype, g.shape, want.shape)
    assert g.tobytes() == np.ascontiguousarray(want).tobytes(), int((g != want).sum())


def targets(nf):
    return sorted({m for m in (nf, nf - 1, nf // 2, nf // 4, 4, 1) if m >= 1}, reverse=True)


def special(name):
    if name.startswith("strip"):
        return D.strip(int(name[5:]))
    if name.startswith("fan"):
        return D.fan(int(name[3:]))
    v, f = D.mesh("icosphere2" if name in ("nan_vertex", "tiny") else "two_components")
    if name == "nan_vertex":
        v = v.copy()
        v[5, 1] = np.nan
    elif name == "tiny":            # squared lengths far below the smallest float32: every cost is +0.0
        v = v * 1e-30
    elif name == "half_huge":       # the cylinder's squared lengths overflow float32, the sphere's do not
        v = v.copy()
        v[42:] *= 1e25
    return v, f


@functools.lru_cache(maxsize=None)
def case(name, float_name):
    """(v, f, the contract's Decimation) of a named mesh in one float type."""
    v, f = D.mesh(name) if name in D.MESH_NAMES + ["bunny", "bunny_unreferenced"] else special(name)
    v = np.ascontiguousarray(v.astype(float_name))
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f, D.Decimation(v, f)


def expected(name, float_name, kind, max_faces):
    v, f, d = case(name, float_name)
    v_out, f_out, cv, cf = d.decimate(max_faces)
    return (v_out, f_out.astype(kind), cv.astype(kind), cf.astype(kind)), d.rounds, d.collapses


def check(pcu, name, float_name, kind, max_faces, torch_in=False):
    v, f, _ = case(name, float_name)
    want, rounds, collapses = expected(name, float_name, kind, max_faces)
    fk = f.astype(kind)
    got = pcu.decimate_triangle_mesh(to_torch(v), to_torch(fk), max_faces) if torch_in else pcu.decimate_triangle_mesh(v, fk, max_faces)
    st = pcu.last_stats()
    assert len(got) == 4
    for g, w in zip(got, want):
        same(g, w, torch_in)
    assert st["n_queries"] == len(f) and st["n_passes"] == rounds and st["n_escalated"] == collapses, (st, rounds, collapses)
    return got


# ---------------------------------------------------------------------------------------------------- the call equals the contract
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("float_name", FLOATS)
@pytest.mark.parametrize("name", D.MESH_NAMES)
def test_equals_the_contract(pcu, name, float_name, kind):
    for max_faces in targets(len(case(name, float_name)[1])):
        check(pcu, name, float_name, kind, max_faces)


@pytest.mark.parametrize("kind", SIGNED)
@pytest.mark.parametrize("float_name", FLOATS)
@pytest.mark.parametrize("name", D.MESH_NAMES)
def test_tensors_in_tensors_out(pcu, name, float_name, kind):
    nf = len(case(name, float_name)[1])
    for max_faces in sorted({nf, max(1, nf // 2), 1}):
        check(pcu, name, float_name, kind, max_faces, torch_in=True)


@pytest.mark.parametrize("float_name", FLOATS)
@pytest.mark.parametrize("nf", EDGES)
@pytest.mark.parametrize("shape", ["strip", "fan"])
def test_strips_and_fans_at_wave_and_block_edges(pcu, shape, nf, float_name):
    for max_faces in sorted({nf, max(1, nf - 1), max(1, nf // 2), max(1, nf // 4), 1}):
        check(pcu, f"{shape}{nf}", float_name, np.int32, max_faces)


@pytest.mark.parametrize("float_name", FLOATS)
def test_the_equal_length_grid_is_ordered_by_rank(pcu, float_name):
    v, f, _ = case("grid", "float64")
    assert (D.valid_edges(v, f, len(v))[3] >> np.uint64(32) == np.float32(1.0).view(np.uint32)).all()
    for max_faces in (len(f) - 1, len(f) - 7, len(f) // 2):
        check(pcu, "grid", float_name, np.int64, max_faces)


@pytest.mark.parametrize("float_name", FLOATS)
def test_a_nan_vertex_stays_and_the_rest_collapses(pcu, float_name):
    v, f, _ = case("nan_vertex", float_name)
    lo, hi, _, _, valid, _ = D.valid_edges(v, f, len(v))
    at_nan = (lo == 5) | (hi == 5)
    assert at_nan.any() and not valid[at_nan].any() and valid[~at_nan].all()
    for max_faces in (len(f) // 2, len(f) // 4, 4):
        v_out, _, cv, _ = check(pcu, "nan_vertex", float_name, np.int32, max_faces)
        at = np.flatnonzero(cv == 5)
        assert len(at) == 1 and np.isnan(v_out[at[0], 1]) and np.isnan(v_out).sum() == 1


@pytest.mark.parametrize("float_name", FLOATS)
def test_squared_lengths_that_underflow_float32_tie_at_zero(pcu, float_name):
    v, f, _ = case("tiny", float_name)
    assert (D.valid_edges(v, f, len(v))[3] >> np.uint64(32) == 0).all()
    for max_faces in (len(f) - 1, len(f) // 2, len(f) // 4):
        check(pcu, "tiny", float_name, np.int32, max_faces)


def test_squared_lengths_that_overflow_float32_are_invalid(pcu):
    v, f, d = case("half_huge", "float64")
    valid = D.valid_edges(v, f, len(v))
    assert not valid[4][valid[0] >= 42].any() and valid[4][valid[1] < 42].all()
    for max_faces in (len(f) // 2, 4):
        _, f_out, _, cf = check(pcu, "half_huge", "float64", np.int64, max_faces)
    assert d.valid_left == 0 and len(f_out) > 4 and (cf >= 80).sum() == 42          # no face of the cylinder is gone


# ---------------------------------------------------------------------------------------------------- the bunny: every block boundary of the sort and the scan
@pytest.mark.parametrize("kind", SIGNED)
@pytest.mark.parametrize("float_name", FLOATS)
def test_the_bunny(pcu, float_name, kind):
    _, f, d = case("bunny", float_name)
    check(pcu, "bunny", float_name, kind, len(f) // 4)
    if float_name == "float64":
        assert d.rounds == 55
    check(pcu, "bunny", float_name, kind, 100)
    if float_name == "float64":
        assert d.rounds == 145


def test_the_bunny_with_unreferenced_vertices_on_the_device(pcu):
    _, f, _ = case("bunny_unreferenced", "float32")
    check(pcu, "bunny_unreferenced", "float32", np.int64, len(f) // 4, torch_in=True)
    check(pcu, "bunny_unreferenced", "float32", np.int64, len(f))


def test_the_body_of_the_references_test(pcu):
    """tests/test_examples.py:681-691 of the reference."""
    v, f, _ = case("bunny", "float64")
    target_num_faces = f.shape[0] // 4
    v_decimate, f_decimate, v_correspondence, f_correspondence = pcu.decimate_triangle_mesh(v, f, target_num_faces)
    birth_v, birth_f = v[v_correspondence], f[f_correspondence]
    assert birth_v.shape == v_decimate.shape and birth_f.shape == f_decimate.shape
    assert v_correspondence.max() < v.shape[0]
    assert f_correspondence.max() < f.shape[0]
    assert f_decimate.shape[0] <= target_num_faces


def test_repeated_calls_give_equal_bytes(pcu):
    v, f, _ = case("bunny", "float32")
    f32 = f.astype(np.int32)
    first = pcu.decimate_triangle_mesh(v, f32, 1000)
    tv, tf = to_torch(v), to_torch(f32)
    for _ in range(3):
        for a, b in zip(first, pcu.decimate_triangle_mesh(v, f32, 1000)):
            same(b, a)
        for a, b in zip(first, pcu.decimate_triangle_mesh(tv, tf, 1000)):
            same(b, a, on_device=True)


# ---------------------------------------------------------------------------------------------------- what only the device can refuse
def test_tensors_are_checked_on_the_device(pcu):
    v, f, _ = case("octahedron", "float64")
    tv = to_torch(v)
    g = f.copy()
    g[3, 1] = len(v)
    with pytest.raises(ValueError, match=r"face index outside \[0, 6\)"):
        pcu.decimate_triangle_mesh(tv, to_torch(g), 4)
    g[3, 1] = -1
    with pytest.raises(ValueError, match=r"face index outside \[0, 6\)"):
        pcu.decimate_triangle_mesh(tv, to_torch(g), 4)
    g = f.copy()
    g[2, 2] = g[2, 0]
    with pytest.raises(ValueError, match="lists a vertex twice"):
        pcu.decimate_triangle_mesh(tv, to_torch(g), 4)
    book = np.array([(0, 1, 2), (0, 1, 3), (0, 1, 4)])
    for max_faces in (2, 3):        # whatever max_faces is
        with pytest.raises(ValueError, match=r"^decimate_triangle_mesh_doc produced an empty mesh\. This can happen if the input is non-manifold\.$"):
            pcu.decimate_triangle_mesh(tv, to_torch(book), max_faces)
    for a, b in zip(pcu.decimate_triangle_mesh(tv, to_torch(f), 4), expected("octahedron", "float64", np.int64, 4)[0]):
        same(a, b, on_device=True)          # and the context goes on working
