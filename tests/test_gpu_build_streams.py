"""The one-pass index build writes a cloud's cell-ordered row ids -- like its coordinates -- as whole 16-byte chunks from the LDS stage of a
bucket, with the partial chunks at both ends of a bucket's share written word by word (grid2.h: sort2_body). Where a bucket's share starts
and ends inside a chunk depends on the points of the buckets before it (any residue mod 4), on the cloud's size (the id stream begins where
the coordinate stream of n + 8 records ends) and on its own fill (shares of 0, 1, 2, 3, 4, 5 ... records have no whole chunk, or one, with
every combination of head and tail). A misplaced or missing id shows as a wrong neighbour index, a misplaced coordinate as a wrong distance.

Cases: cloud sizes of every residue mod 4 from a few dozen points to several buckets' worth, and clouds that sit almost entirely in one small
blob with a few dozen stragglers spread over the box, so that most buckets of the grid hold none to a handful of points. Both entry points
that read the id stream (k_nearest_neighbors with k = 1, chamfer_distance(return_index=True)), float32 and float64.

Bar: neighbour indices and the k = 1 distances' bits are EQUAL to the oracle's. chamfer_distance's scalar is a mean that the oracle takes
with numpy in another order of additions: it is held to the package's documented tolerance (1e-4 relative for float32, 1e-6 for float64)."""
import numpy as np
import pytest

import oracle
from conftest import cloud

pytestmark = pytest.mark.gpu

SIZES = [65, 66, 67, 68, 1023, 4097, 8193, 100003]


@pytest.fixture(scope="module")
def pcu():
    import point_cloud_utils_amd as m
    from point_cloud_utils_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: the gfx950 path has no CPU fallback"
    return m


def blob_cloud(seed, n, n_stray, dtype):
    """n - n_stray points in a blob of 1 % of the box's edge, n_stray uniform over the unit box: a grid whose buckets mostly hold 0 .. 5 points."""
    rng = np.random.default_rng(seed)
    a = (rng.random((n, 3)) * 0.01 + 0.37).astype(dtype)
    at = rng.choice(n, n_stray, replace=False)
    a[at] = rng.random((n_stray, 3)).astype(dtype)
    return np.ascontiguousarray(a)


def _check_knn(pcu, kind, q, r):
    d, c = pcu.k_nearest_neighbors(q, r, 1)
    d0, c0 = oracle.k_nearest_neighbors(q, r, 1, kind=kind)
    assert c.shape == c0.shape and d.dtype == q.dtype
    assert np.array_equal(c, c0), f"indices differ {pcu.last_stats()}"
    assert np.array_equal(d.view(np.uint8), d0.view(np.uint8)), "distance bits differ"


def _check_chamfer(pcu, kind, a, b):
    ch, cxy, cyx = pcu.chamfer_distance(a, b, return_index=True)
    ch0, cxy0, cyx0 = oracle.chamfer_distance(a, b, return_index=True, kind=kind)
    assert np.array_equal(cxy, cxy0) and np.array_equal(cyx, cyx0), f"indices differ {pcu.last_stats()}"
    rtol = 1e-4 if a.dtype == np.float32 else 1e-6
    assert abs(float(ch) - float(ch0)) <= rtol * abs(float(ch0))
    # the fused call (no indices: the LEAN build, streams only) agrees with the row-based one
    assert abs(float(pcu.chamfer_distance(a, b)) - float(ch0)) <= rtol * abs(float(ch0))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", SIZES)
def test_knn1_every_alignment(pcu, oracle_kind, dtype, n):
    # dataset of n points (its id stream is what the result rows are read from); queries of another size, then the roles swapped
    q, r = cloud(4100 + n, 777, dtype), cloud(4200 + n, n, dtype)
    _check_knn(pcu, oracle_kind, q, r)
    _check_knn(pcu, oracle_kind, r, q)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", SIZES)
def test_chamfer_index_every_alignment(pcu, oracle_kind, dtype, n):
    a, b = cloud(4300 + n, n, dtype), cloud(4400 + n, n + 1, dtype)       # (two sizes of different residue in one call)
    _check_chamfer(pcu, oracle_kind, a, b)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n,n_stray", [(2001, 40), (4098, 25), (20003, 120), (60001, 64)])
def test_blob_with_stragglers(pcu, oracle_kind, dtype, n, n_stray):
    a, b = blob_cloud(4500 + n, n, n_stray, dtype), blob_cloud(4600 + n, n + 2, n_stray + 1, dtype)
    _check_knn(pcu, oracle_kind, a, b)
    _check_chamfer(pcu, oracle_kind, a, b)
