"""CPU tests of the contract of marching_cubes_sparse_voxel_grid and sparse_voxel_grid_to_hex_mesh: the generated case
table against the rule's restatement and its pinned properties, and the numpy restatement (tests/marching_cubes_contract.py) on inputs whose
answers are known. The GPU tests hold the library to the restatement; these hold the restatement to the contract."""
import collections
import hashlib

import numpy as np
import pytest

import marching_cubes_contract as mc
import voxelize_contract as vc

PINNED = {1: [(0, 8, 3)], 3: [(1, 9, 8), (1, 8, 3)], 0x16: [(0, 2, 10), (0, 10, 9), (4, 7, 8)], 0x69: [(0, 8, 11), (0, 11, 2), (4, 9, 10), (4, 10, 6)],
          0xA5: [(0, 8, 3), (1, 2, 10), (4, 9, 5), (6, 11, 7)], 254: [(0, 3, 8)]}


# ---------------------------------------------------------------------------------------------------- the table
def test_generator_reproduces_the_committed_header_and_the_pinned_hash():
    gen = mc.generator()
    with open(mc.os.path.join(mc.CSRC, "mc_table.h")) as fh:
        assert fh.read() == gen.header_text()
    assert hashlib.sha256(gen.table_bytes()).hexdigest() == mc.TABLE_SHA256 == gen.SHA256
    assert np.array_equal(np.array(gen.table(), dtype=np.int8), mc.TABLE), "generator and restatement of the rule differ"
    assert np.array_equal(mc.header_table(), mc.TABLE)
    assert hashlib.sha256(mc.TABLE.tobytes()).hexdigest() == mc.TABLE_SHA256


def test_every_case_uses_exactly_its_crossed_edges_in_at_most_five_triangles():
    for mask in range(256):
        row = mc.TABLE[mask]
        used = set(int(e) for e in row if e >= 0)
        crossed = set(e for e, (a, b) in enumerate(mc.EDGES.tolist()) if (mask >> a & 1) != (mask >> b & 1))
        assert used == crossed, mask
        n = int(mc.N_TRI[mask])
        assert n <= 5 and (row[:3 * n] >= 0).all() and (row[3 * n:] == -1).all(), mask
    by_count = collections.Counter(int(n) for n in mc.N_TRI)
    assert dict(by_count) == {0: 2, 1: 16, 2: 50, 3: 80, 4: 76, 5: 32} and int(mc.N_TRI.sum()) == 820


def test_pinned_rows():
    for mask, tris in PINNED.items():
        assert mc.case_triangles(mask) == tris, hex(mask)
        assert [tuple(int(e) for e in mc.TABLE[mask, 3 * i:3 * i + 3]) for i in range(len(tris))] == tris


def test_single_corner_caps_have_normals_towards_the_greater_values():
    """The sixteen one-triangle cases, placed at edge midpoints: the normal points towards a lone inside corner and away from a lone outside
    one. (The closed surfaces below check the orientation of all other cases through their neighbours.)"""
    mid = (mc.CORNERS[mc.EDGES[:, 0]] + mc.CORNERS[mc.EDGES[:, 1]]) / 2.0
    for mask in range(1, 255):
        if bin(mask).count("1") == 1:
            c = mc.CORNERS[[i for i in range(8) if mask >> i & 1][0]].astype(float)
            (a, b, d), = mc.case_triangles(mask)
            n = np.cross(mid[b] - mid[a], mid[d] - mid[a])
            assert np.dot(n, c - mid[a]) > 0, mask
        if bin(mask).count("1") == 7:
            c = mc.CORNERS[[i for i in range(8) if not mask >> i & 1][0]].astype(float)
            (a, b, d), = mc.case_triangles(mask)
            n = np.cross(mid[b] - mid[a], mid[d] - mid[a])
            assert np.dot(n, c - mid[a]) < 0, mask


# ---------------------------------------------------------------------------------------------------- the surface
@pytest.fixture(scope="module")
def random_field():
    n = 9
    P, cubes = mc.dense_grid(n, 0.0, float(n - 1))
    S = np.random.default_rng(0).standard_normal((n, n, n))
    S[0], S[-1], S[:, 0], S[:, -1], S[:, :, 0], S[:, :, -1] = -1, -1, -1, -1, -1, -1
    return mc.marching_cubes(S.reshape(-1), P, cubes, 0.0)


def test_random_field_is_closed_oriented_and_has_the_measured_size(random_field):
    v, f = random_field
    assert mc.is_closed_and_oriented(f)
    assert not mc.has_repeated_indices(f)
    assert len(f) == 1208
    assert mc.signed_volume(v, f) < 0                      # the inside (greater values) is enclosed: normals point into it


def test_sphere_has_the_topology_and_volume_of_a_sphere():
    P, cubes = mc.dense_grid(17)
    v, f = mc.marching_cubes(np.linalg.norm(P, axis=1) - 0.7, P, cubes, 0.0)
    assert mc.is_closed_and_oriented(f) and mc.euler_characteristic(v, f) == 2
    vol, want = mc.signed_volume(v, f), 4.0 / 3.0 * np.pi * 0.7 ** 3
    assert vol > 0 and abs(vol - want) <= 0.025 * want, (vol, want)          # (measured: 1.9 % low)


def test_vertices_ascend_by_index_pair_and_faces_follow_the_cubes():
    P, cubes = mc.dense_grid(6, dtype=np.float32)
    S = np.random.default_rng(3).standard_normal(len(P)).astype(np.float32)
    v, f = mc.marching_cubes(S, P, cubes.astype(np.int32), 0.25)
    assert v.dtype == np.float32 and f.dtype == np.int32
    perm = np.random.default_rng(4).permutation(len(cubes))
    v2, f2 = mc.marching_cubes(S, P, cubes[perm].astype(np.int32), 0.25)
    assert np.array_equal(v, v2)                           # the vertex rows do not depend on the order of the cubes
    cnt = mc.N_TRI[((S[cubes] > np.float32(0.25)).astype(np.int64) << np.arange(8)).sum(axis=1)]
    start = np.cumsum(cnt) - cnt
    rows = np.concatenate([np.arange(start[c], start[c] + cnt[c]) for c in perm])
    assert np.array_equal(f2, f[rows])
    # every vertex lies on its grid edge, between the two ends
    assert np.isfinite(v).all() and (v >= -1).all() and (v <= 1).all()


def test_a_scalar_on_the_level_is_outside_and_its_triangles_are_kept():
    P, cubes = mc.dense_grid(2)
    S = np.array([1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0])       # corner 0 inside, the others exactly on the level
    v, f = mc.marching_cubes(S, P, cubes, 0.0)
    assert len(f) == 1 and len(v) == 3
    assert np.array_equal(v, P[[1, 2, 4]])                       # t = 1 from lo = 0: the far ends (x fastest: vertices 1, 2 and 4)
    with pytest.raises(ValueError, match="No level set found for isovalue 1.000000"):
        mc.marching_cubes(S, P, cubes, 1.0)


# ---------------------------------------------------------------------------------------------------- the hex mesh
def test_hex_mesh_of_two_voxels_sharing_a_face():
    v, c = mc.hex_mesh(np.array([[0, 0, 0], [1, 0, 0], [0, 0, 0]]), 0.5, (1.0, 2.0, 3.0))
    assert v.shape == (12, 3) and c.shape == (3, 8) and c.dtype == np.int64 and v.dtype == np.float64
    assert np.array_equal(c[0], c[2]) and len(set(c[0]) & set(c[1])) == 4
    # voxel ijk is centred on origin + ijk * size, and its corners come in the contract's order
    for row, ijk in zip(c, [(0, 0, 0), (1, 0, 0), (0, 0, 0)]):
        want = np.array([1.0, 2.0, 3.0]) + (np.array(ijk) + mc.CORNERS - 0.5) * 0.5
        assert np.array_equal(v[row], want)
    codes = vc.morton(np.rint((v - np.array([1.0, 2.0, 3.0])) / 0.5 + 0.5).astype(np.int64))
    assert (np.diff(codes.astype(np.uint64)) > 0).all()


def test_hex_mesh_range():
    mc.hex_mesh(np.array([[-mc.RANGE, 0, mc.RANGE - 2]]))
    for bad in (mc.RANGE - 1, -mc.RANGE - 1):
        with pytest.raises(ValueError, match="overflow integer"):
            mc.hex_mesh(np.array([[0, bad, 0]]))
