"""GPU edge tests (-m gpu) of SURVEY.md 8f-4: the repo's own stable radix sort and scan (csrc/radix.h, driven by sort_by_triple / runs_of /
own_inclusive_scan in csrc/voxel_host.h) under downsample_point_cloud_on_voxel_grid and deduplicate_point_cloud, and the Morton kernels, at
the sizes, key widths and inputs where they could go wrong unnoticed by tests/test_gpu_voxel.py:

  * sizes at every tile edge (64-lane round, 512-key wave tile, 2048-key block, 4096-value scan tile, the second trip of k_rs_scan_rows
    beyond 512 x 1024 rows and of k_sc_sums beyond 4096 x 1024 rows), each held BIT-EXACT to a CPU oracle that adds in input order -- a sort
    that is a permutation but not stable changes the order of additions (voxels) or the representative row (dedup) and fails;
  * every path of sort_by_triple: zero bits, packed keys of 8 / 9 / 16 / 17 / 24 / 25 bits, a constant axis in each position, negative
    voxel indices, the two shift guards of k_key_pack (w1 + w2 == 64, w2 == 64) and the component-by-component path for triples wider than
    64 bits. Every such case asserts, with a numpy restatement of enc() / key_u64() / bits_of(), the key widths it was built for before
    it calls the GPU, so that a later change of an input cannot silently move it to another path;
  * rounding: duplicate removal on exact halves (round half away from zero, not rint) and points on / one ulp beside voxel boundaries;
  * device-resident (torch) inputs on the current and on a side stream; Morton codes beyond 21 bits, the grid-stride trip of the
    element-wise kernels, morton_knn on duplicate codes with the tie rule of csrc/morton.h; the Python-side argument checks of _voxel.py.

The only tolerance in this module is zero (np.array_equal): every quantity is an integer or a sum whose order the contract fixes.

Out of scope: NaN / infinite coordinates and voxel indices beyond the range of int in these three operators. The reference's own behaviour
there is undefined (int(floor(nan)), libigl's sort of NaN rows); what this project should do with them is a design decision, not a test.
"""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pcu():
    import point_cloud_utils_amd as m
    from point_cloud_utils_amd import _lib
    assert _lib.device_count() > 0
    return m


@pytest.fixture(scope="module")
def mkind():
    return "ref" if oracle.have_ref_morton() else "port"


def _other(dtype):
    return np.float32 if dtype == np.float64 else np.float64


# ------------------------------------------------------------------------------------------------ which path will sort_by_triple take?
# numpy restatement of csrc/pcu_types.h enc(), csrc/radix.h key_u64() and csrc/voxel_host.h bits_of() / the `w0 + w1 + w2 <= 64` choice
def _enc(r):
    r = np.ascontiguousarray(r)
    if r.dtype == np.float32:
        u, sign = r.view(np.uint32), np.uint32(0x80000000)
    else:
        u, sign = r.view(np.uint64), np.uint64(1 << 63)
    return np.where((u & sign) != 0, ~u, u | sign)


def _widths(keys):
    return tuple((int(keys[:, j].max()) - int(keys[:, j].min())).bit_length() for j in range(3))


def _voxel_keys(p, vs, mb):
    vs = np.asarray([vs] * 3 if np.isscalar(vs) else vs, dtype=p.dtype); mb = np.asarray(mb, dtype=p.dtype)
    return np.floor((p - mb) / vs).astype(np.int32)


def voxel_widths(p, vs, mb):
    """bits per component of the packed voxel key: key_u64(int) = (unsigned)v ^ 0x80000000, less the component's minimum"""
    return _widths(np.ascontiguousarray(_voxel_keys(p, vs, mb)).view(np.uint32) ^ np.uint32(0x80000000))


def _round_half_away(p, eps):
    T = p.dtype.type
    r = p
    if eps > 0:
        q = p / T(eps)
        t = np.trunc(q)
        r = t + np.where(np.abs(q - t) >= 0.5, np.sign(q), 0).astype(p.dtype)
    return r + T(0)


def dedup_widths(p, eps):
    """bits per component of the dedup key: enc(round(p / eps) + 0), less the component's minimum"""
    return _widths(_enc(_round_half_away(np.ascontiguousarray(p), eps)))


def _path(w):
    return "packed" if sum(w) <= 64 else "wide"


# ------------------------------------------------------------------------------------------------ comparisons
def _default_bounds(p, vs):
    vs = np.array([vs] * 3 if np.isscalar(vs) else vs)
    return np.min(p, axis=0) - vs * 0.5, np.max(p, axis=0) + vs * 0.5            # the wrapper's own formula (float64, cast by the library)


def check_voxels(pcu, p, a, vs, mb=None, mxb=None, mp=1):
    """GPU result (points + one attribute) bit-equal to oracle.voxel_downsample_fast; returns the number of voxels."""
    kw = {} if mb is None else {"min_bound": mb, "max_bound": mxb}
    if mb is None:
        mb, _ = _default_bounds(p, vs)
    v0, a0 = oracle.voxel_downsample_fast(p, a, [vs] * 3 if np.isscalar(vs) else vs, mb, mp)
    assert len(v0) > 0
    if a is None:
        v = pcu.downsample_point_cloud_on_voxel_grid(vs, p, min_points_per_voxel=mp, **kw)
    else:
        v, ga = pcu.downsample_point_cloud_on_voxel_grid(vs, p, a, min_points_per_voxel=mp, **kw)
        assert ga.dtype == a.dtype and ga.shape == a0.shape and np.array_equal(ga, a0)
    assert v.dtype == p.dtype and v.shape == v0.shape and np.array_equal(v, v0)
    return len(v)


def check_dedup(pcu, p, eps):
    """GPU result equal to oracle.deduplicate_point_cloud; x_new = p[svi]; svi is the lowest row of its group. Returns (x, svi, svj)."""
    x, svi, svj = pcu.deduplicate_point_cloud(p, eps, return_index=True)
    x0, svi0, svj0 = oracle.deduplicate_point_cloud(p, eps)
    n = len(p)
    assert x.dtype == p.dtype and svi.dtype == np.int32 and svj.dtype == np.int32
    assert x.shape == x0.shape and svi.shape == svi0.shape and svj.shape == (n,)
    assert np.array_equal(svj, svj0) and np.array_equal(svi, svi0) and np.array_equal(x, x0)
    assert np.array_equal(p[svi], x)
    lowest = np.full(len(x), n, np.int64)
    np.minimum.at(lowest, svj, np.arange(n))
    assert np.array_equal(svi, lowest)                                            # stability: the first row of every group represents it
    return x, svi, svj


# ------------------------------------------------------------------------------------------------ 1. size sweep, bit-exact
SIZES = [1, 2, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193, 524287, 524288, 524289, 524288 + 513]
BIG = 4096 * 1024 + 4096 + 4            # k_sc_sums: second trip of the carry loop (more than 1024 scan tiles)
SWEEP = [(dt, n) for dt in (np.float32, np.float64) for n in SIZES] + [(np.float64, BIG)]
_sweep_ids = [f"{np.dtype(dt).name}-{n}" for dt, n in SWEEP]


@pytest.mark.parametrize("dtype,n", SWEEP, ids=_sweep_ids)
def test_voxel_size_sweep(pcu, dtype, n):
    """radix.h k_rs_hist / k_rs_scan_rows / k_rs_scatter (partial rounds, partial wave tiles, second trip of the row scan), k_sc_tiles /
    k_sc_sums / k_sc_add (partial tiles, second trip), voxel.h k_run_starts / k_voxel_means at n = 1 and at every tile edge."""
    rng = np.random.default_rng(n)
    p = rng.random((n, 3), dtype=dtype)
    a = rng.standard_normal((n, 2)).astype(_other(dtype))
    # few groups: at most 8 voxels -- long runs of one digit, every lane a peer in the ballot match, runs over many wave and scan tiles
    w = voxel_widths(p, 0.5, (0, 0, 0))
    assert max(w) <= 1 and _path(w) == "packed"
    assert check_voxels(pcu, p, a, 0.5, (0, 0, 0), (1, 1, 1)) <= 8
    # many groups: about n / 3 voxels of a few distinct points each
    g = max(1, round((n / 3.0) ** (1.0 / 3.0)))
    assert _path(voxel_widths(p, 1.0 / g, (0, 0, 0))) == "packed"
    m = check_voxels(pcu, p, a, 1.0 / g, (0, 0, 0), (1, 1, 1))
    if n >= 511:
        assert n / 5 < m < n / 2


@pytest.mark.parametrize("dtype,n", SWEEP, ids=_sweep_ids)
def test_dedup_size_sweep(pcu, dtype, n):
    """The same lines of radix.h under voxel.h k_round_keys / k_dedup_write and the head-flag scan of runs_of, packed and wide keys."""
    rng = np.random.default_rng(n + 1)
    # few groups: rows drawn from 5 distinct points (exact duplicates, eps 0)
    five = rng.random((5, 3), dtype=dtype)
    p = five[rng.integers(0, 5, n)]
    x, _, _ = check_dedup(pcu, p, 0.0)
    assert len(x) <= 5
    # many groups: about n / 3, whose rows differ below eps -- the representative must be the lowest row, not just any of its group
    m = max(1, n // 3)
    base = rng.random((m, 3), dtype=dtype)
    rows = base[np.arange(n) % m]                                                 # base, base, base[:n - 2 m]
    rows = (rows + (rng.random((n, 3), dtype=dtype) - dtype(0.5)) * dtype(1e-5)).astype(dtype)
    rows = rows[rng.permutation(n)]
    x, _, _ = check_dedup(pcu, rows, 1e-3)
    if n >= 511:
        assert n / 5 < len(x) < n / 2


def test_voxel_downsample_large_bit_exact(pcu):
    """test_voxel_downsample_large's 1M x 1/128 case, held bit-exact to the in-order oracle (np.allclose against reduceat passes an unstable sort)."""
    from conftest import cloud
    p = cloud(5, 1_000_000, np.float64)
    assert 500_000 < check_voxels(pcu, p, None, 1.0 / 128.0) < 1_000_000


# ------------------------------------------------------------------------------------------------ 2. key widths and paths: voxels
def lattice_cloud(seed, n, widths, lo, dtype):
    """n points whose voxel index (voxel size 1, min_bound 0) on axis j spans exactly [lo[j], lo[j] + 2^widths[j] - 1], both ends present;
    about n / 3 occupied cells; fractions in [0.25, 0.75) so that no rounding moves a point to another cell."""
    rng = np.random.default_rng(seed)
    m = max(2, n // 3)
    cell = np.stack([rng.integers(0, 1 << w, m) for w in widths], axis=1)
    cell[0] = 0; cell[1] = [(1 << w) - 1 for w in widths]
    idx = np.concatenate([np.arange(m), rng.integers(0, m, n - m)])
    p = cell[idx] + np.asarray(lo) + rng.uniform(0.25, 0.75, (n, 3))
    return p.astype(dtype)[rng.permutation(n)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_voxel_signed_cloud_negative_indices(pcu, dtype):
    """radix.h key_u64(int): the sign flip that orders negative voxel indices below positive ones; voxel.h k_voxel_keys: floor, not
    truncation; points outside [min_bound, max_bound] are binned like any other (src/sample_point_cloud.cpp:199-207 does not clip)."""
    rng = np.random.default_rng(20)
    n = 50000
    p = ((rng.random((n, 3)) - 0.5) * 3.0).astype(dtype)
    a = rng.standard_normal((n, 2)).astype(_other(dtype))
    mb, mxb, vs = (-0.35, 0.15, -0.85), (0.8, 0.9, 0.6), (0.1, 0.07, 0.2)
    key = _voxel_keys(p, vs, mb)
    assert np.all(key.min(0) < -2) and np.all(key.max(0) > 2) and np.all((p > np.asarray(mxb)).any(0))
    assert np.any(np.floor((p - np.asarray(mb, dtype)) / np.asarray(vs, dtype)) != np.trunc((p - np.asarray(mb, dtype)) / np.asarray(vs, dtype)))
    assert _path(voxel_widths(p, vs, mb)) == "packed"
    assert check_voxels(pcu, p, a, vs, mb, mxb) > 1000
    assert check_voxels(pcu, p, a, vs, mb, mxb, mp=3) > 100


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("widths", [(0, 0, 0), (3, 3, 2), (3, 3, 3), (6, 5, 5), (6, 6, 5), (8, 8, 8), (9, 8, 8), (0, 6, 5), (6, 0, 5), (6, 5, 0)],
                         ids=lambda w: "w%d_%d_%d" % w)
def test_voxel_packed_key_widths(pcu, dtype, widths):
    """voxel_host.h sort_by_triple<int>, packed path: 0 bits (no pass, ids stay the identity), totals that end a pass on a full digit
    (8, 16, 24) and on a single bit (9, 17, 25), a zero-width component in each position (k_key_pack's shifts by w1 + w2 and w2)."""
    n = 60000
    lo = (-5, -300, 3)
    p = lattice_cloud(sum(widths) + 7 * widths[0], n, widths, lo, dtype)
    a = np.random.default_rng(21).standard_normal((n, 2)).astype(_other(dtype))
    assert voxel_widths(p, 1.0, (0, 0, 0)) == widths
    key = _voxel_keys(p, 1.0, (0, 0, 0))
    assert np.array_equal(key.min(0), lo) and np.array_equal(key.max(0), [l + (1 << w) - 1 for l, w in zip(lo, widths)])
    m = check_voxels(pcu, p, a, 1.0, (0, 0, 0), (1000, 1000, 1000))
    assert m == len(np.unique(key, axis=0)) and (m == 1 if sum(widths) == 0 else m > min(1 << sum(widths), n // 3) // 2)


@pytest.mark.parametrize("repeats", [False, True], ids=["distinct", "runs"])
def test_voxel_wide_path(pcu, repeats):
    """voxel_host.h sort_by_triple<int>, component-by-component path (k_key_gather + three stable sorts, least significant first) and
    voxel.h k_run_heads (run heads through the permutation): 26 + 26 + 26 = 78 key bits."""
    rng = np.random.default_rng(22)
    n = 100000
    if repeats:      # a quarter of the rows exact repeats, another quarter other points of the same voxels (their order of addition shows)
        base = rng.uniform(-2e7, 2e7, (n // 2, 3))
        p = np.concatenate([base, base[:n // 4], np.floor(base[n // 4:]) + rng.uniform(0.0, 1.0, (n // 4, 3))])[rng.permutation(n)]
    else:
        p = rng.uniform(-2e7, 2e7, (n, 3))
    a = rng.standard_normal((n, 2)).astype(np.float32)
    mb, mxb = (-2e7, -2e7, -2e7), (2e7, 2e7, 2e7)
    w = voxel_widths(p, 1.0, mb)
    assert w == (26, 26, 26) and _path(w) == "wide"
    m = check_voxels(pcu, p, a, 1.0, mb, mxb)
    assert (m < n * 0.51) if repeats else (m > n * 0.99)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_voxel_min_points_per_voxel(pcu, dtype):
    """voxel.h k_run_keep and the compaction scan; _voxel.py's restatement of the reference wrapper's returns for an empty result
    (point_cloud_utils/__init__.py:185-200: a first attribute whose result has size 0 is dropped)."""
    n = 5000
    p = lattice_cloud(23, n, (2, 2, 1), (-1, 0, -1), dtype)
    rng = np.random.default_rng(24)
    a0 = rng.standard_normal((n, 2)).astype(_other(dtype)); a1 = rng.standard_normal((n, 3)).astype(dtype)
    assert voxel_widths(p, 1.0, (0, 0, 0)) == (2, 2, 1)
    _, counts = np.unique(_voxel_keys(p, 1.0, (0, 0, 0)), axis=0, return_counts=True)
    big = int(counts.max())
    kw = dict(min_bound=(0, 0, 0), max_bound=(5, 5, 5))
    assert check_voxels(pcu, p, a0, 1.0, (0, 0, 0), (5, 5, 5), mp=big) == int((counts == big).sum())       # equal to the largest run
    assert check_voxels(pcu, p, a0, 1.0, (0, 0, 0), (5, 5, 5), mp=int(np.median(counts))) < len(counts)
    for mp in (0, -3):                                                                                    # keep all
        assert check_voxels(pcu, p, a0, 1.0, (0, 0, 0), (5, 5, 5), mp=mp) == len(counts)
    # larger than every run: nothing is kept
    v = pcu.downsample_point_cloud_on_voxel_grid(1.0, p, min_points_per_voxel=big + 1, **kw)
    assert isinstance(v, np.ndarray) and v.shape == (0, 3) and v.dtype == dtype
    v = pcu.downsample_point_cloud_on_voxel_grid(1.0, p, a0, min_points_per_voxel=big + 1, **kw)
    assert isinstance(v, np.ndarray) and v.shape == (0, 3) and v.dtype == dtype
    r = pcu.downsample_point_cloud_on_voxel_grid(1.0, p, a0, a1, min_points_per_voxel=big + 1, **kw)
    assert isinstance(r, tuple) and len(r) == 2 and r[0].shape == (0, 3) and r[0].dtype == dtype and r[1].shape == (0, 3) and r[1].dtype == a1.dtype


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_voxel_boundaries_ieee_division(pcu, dtype):
    """voxel.h k_voxel_keys: (p - min_bound) / voxel_size is the IEEE division of the point type. Rows on T(min_bound + j * voxel_size)
    and one ulp to either side, voxel size 0.1 (not representable): an inexact division would bin them differently from the reference."""
    rng = np.random.default_rng(25)
    mb, vs = (-1.3, 0.7, -0.05), 0.1
    j = np.arange(-60, 260)
    cols = []
    for ax in range(3):
        c = (mb[ax] + j * vs).astype(dtype)
        cols.append(np.concatenate([c, np.nextafter(c, dtype(-np.inf)), np.nextafter(c, dtype(np.inf))]))
    n = 40000
    p = np.stack([cols[ax][rng.integers(0, len(cols[ax]), n)] for ax in range(3)], axis=1)
    p[:len(cols[0])] = np.stack(cols, axis=1)                                     # every boundary value of every axis is present
    p = np.ascontiguousarray(p[rng.permutation(n)])
    a = rng.standard_normal((n, 2)).astype(_other(dtype))
    assert _path(voxel_widths(p, vs, mb)) == "packed"
    assert check_voxels(pcu, p, a, vs, mb, (40, 40, 40)) > 10000
    q = np.ascontiguousarray(p[:, [1, 2, 0]])                                      # the same values on the other axes
    assert check_voxels(pcu, q, a, (vs, vs, vs), (mb[1], mb[2], mb[0]), (40, 40, 40)) > 10000


# ------------------------------------------------------------------------------------------------ 2. key widths and paths: dedup
def unit_cube_rows(dtype, n, planar=False):
    """U[0,1)^3 rows with a third of them repeats, and the minima pinned so that the key widths are 27/27/28 (f32) and 57/56/56 (f64)."""
    rng = np.random.default_rng(30)
    m = n - n // 3
    base = rng.random((m, 3), dtype=dtype)
    lo = np.array([1e-4, 1e-4, 1e-6] if dtype == np.float32 else [1e-6, 1e-4, 1e-4], dtype)
    base = np.maximum(base, lo)
    base[0] = lo; base[1] = dtype(1.0) - dtype(2.0 ** -20)
    if planar:
        base[:, 2] = dtype(0.5)
    return np.concatenate([base, base[rng.integers(0, m, n - m)]])[rng.permutation(n)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_dedup_unit_cube_wide(pcu, dtype):
    """voxel_host.h sort_by_triple<K>, component-by-component path, at 600 000 rows (k_rs_scan_rows' second trip); k_run_heads."""
    p = unit_cube_rows(dtype, 600000)
    w = dedup_widths(p, 0.0)
    assert w == ((27, 27, 28) if dtype == np.float32 else (57, 56, 56)) and _path(w) == "wide"
    x, _, _ = check_dedup(pcu, p, 0.0)
    assert len(x) == 400000
    check_dedup(pcu, p[:11010], 0.0)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_dedup_planar(pcu, dtype):
    """A constant last component: 27/27/0 packs into 54 bits (f32: seven passes); 57/56/0 is still wide, with one zero-pass component
    (sort_by_triple: `identity` stays true through the pass of a zero-width component)."""
    p = unit_cube_rows(dtype, 100000, planar=True)
    w = dedup_widths(p, 0.0)
    assert w == ((27, 27, 0) if dtype == np.float32 else (57, 56, 0)) and _path(w) == ("packed" if dtype == np.float32 else "wide")
    check_dedup(pcu, p, 0.0)
    for perm in ([2, 0, 1], [0, 2, 1]):                                           # the constant component first / in the middle
        q = np.ascontiguousarray(p[:, perm])
        assert dedup_widths(q, 0.0) == tuple(w[i] for i in perm)
        check_dedup(pcu, q, 0.0)


def test_dedup_packed_64_bits_two_components(pcu):
    """radix.h k_key_pack, first guard: 0/32/32 bits -> w1 + w2 == 64, the shift of component 0 by 64 must not happen."""
    rng = np.random.default_rng(31)
    n, m = 100000, 60000
    j = rng.integers(0, 1 << 32, (m, 2)).astype(np.uint64)
    j[0] = 0; j[1] = (1 << 32) - 1; j[2] = [0, (1 << 32) - 1]
    base = np.empty((m, 3), np.float64)
    base[:, 0] = -7.25
    base[:, 1:] = 1.0 + j.astype(np.float64) * 2.0 ** -52                        # exact: 1 + j ulp
    p = np.concatenate([base, base[rng.integers(0, m, n - m)]])[rng.permutation(n)]
    w = dedup_widths(p, 0.0)
    assert w == (0, 32, 32) and _path(w) == "packed"
    x, _, _ = check_dedup(pcu, p, 0.0)
    assert len(x) == len(np.unique(j, axis=0))


def test_dedup_packed_64_bits_one_component(pcu):
    """radix.h k_key_pack, second guard: 0/0/64 bits -> w2 == 64 (a signed line along z, eps 1e-3; eps 0 would give 63 bits)."""
    rng = np.random.default_rng(32)
    n = 100000
    p = np.empty((n, 3), np.float64)
    p[:, 0] = 3.0; p[:, 1] = -0.125
    p[:, 2] = rng.uniform(-1.0, 1.0, n)
    p[:4, 2] = [0.9999, -0.9999, 1e-5, -1e-5]
    assert dedup_widths(p, 0.0) == (0, 0, 63)
    w = dedup_widths(p, 1e-3)
    assert w == (0, 0, 64) and _path(w) == "packed"
    x, _, svj = check_dedup(pcu, p, 1e-3)
    assert len(x) == 2001 and svj[2] == svj[3]                                    # round(-0.01) = -0 is the same number as +0


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_dedup_signed_cube_and_zeros(pcu, dtype):
    """voxel.h k_round_keys: `v + 0` makes -0 and +0 one key (their enc() patterns differ); full-width components 32/32/32 and 64/64/64."""
    rng = np.random.default_rng(33)
    n = 200000
    p = rng.uniform(-1.0, 1.0, (n, 3)).astype(dtype)
    p[:6] = [[0.9999, 0.9999, 0.9999], [-0.9999, -0.9999, -0.9999], [0.0, -0.0, 0.0], [-0.0, 0.0, -0.0], [1e-5, -1e-5, 1e-5], [-1e-5, 1e-5, -1e-5]]
    w = dedup_widths(p, 1e-3)
    assert w == ((32, 32, 32) if dtype == np.float32 else (64, 64, 64)) and _path(w) == "wide"
    _, _, svj = check_dedup(pcu, p, 1e-3)
    assert svj[2] == svj[3] == svj[4] == svj[5]
    _, _, svj = check_dedup(pcu, p, 0.0)
    assert svj[2] == svj[3] and svj[4] != svj[5]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_dedup_halves_round_away_from_zero(pcu, dtype):
    """voxel.h k_round_keys: round() is half away from zero (igl::round = std::round). Every coordinate is a multiple of one half, eps 1:
    9 values per axis, 729 groups; rint (half to even) gives another partition."""
    rng = np.random.default_rng(34)
    p = (0.5 * rng.integers(-8, 8, (20000, 3))).astype(dtype)
    _, inv_away = np.unique(_round_half_away(p, 1.0), axis=0, return_inverse=True)
    _, inv_even = np.unique(np.rint(p) + dtype(0), axis=0, return_inverse=True)
    assert not np.array_equal(inv_away.ravel(), inv_even.ravel())                 # the input can tell the two roundings apart
    x, _, svj = check_dedup(pcu, p, 1.0)
    assert len(x) == 729 and np.array_equal(svj, inv_away.ravel())


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_dedup_arguments_and_layouts(pcu, dtype):
    """_voxel.py deduplicate_point_cloud: eps < 0 is eps = 0, return_index=False, zero rows, F-ordered and strided inputs."""
    rng = np.random.default_rng(35)
    base = rng.random((3000, 3), dtype=dtype)
    p = np.concatenate([base, base[:2000]])[rng.permutation(5000)]
    x0, i0, j0 = check_dedup(pcu, p, 0.0)
    x, i, j = pcu.deduplicate_point_cloud(p, -0.5)
    assert len(x0) == 3000 and np.array_equal(x, x0) and np.array_equal(i, i0) and np.array_equal(j, j0)
    only = pcu.deduplicate_point_cloud(p, 0.0, return_index=False)
    assert isinstance(only, np.ndarray) and np.array_equal(only, x0)
    x, i, j = pcu.deduplicate_point_cloud(np.zeros((0, 3), dtype), 0.1)
    assert x.shape == (0, 3) and x.dtype == dtype and i.shape == (0,) and j.shape == (0,) and i.dtype == np.int32 and j.dtype == np.int32
    f = np.asfortranarray(p)
    assert not f.flags.c_contiguous
    for got, want in zip(pcu.deduplicate_point_cloud(f, 1e-3), pcu.deduplicate_point_cloud(p, 1e-3)):
        assert np.array_equal(got, want)
    s = p[::2]
    assert not s.flags.c_contiguous
    check_dedup(pcu, s, 1e-3)
    for got, want in zip(pcu.deduplicate_point_cloud(s, 1e-3), pcu.deduplicate_point_cloud(np.ascontiguousarray(s), 1e-3)):
        assert np.array_equal(got, want)
    a = rng.standard_normal((5000, 2)).astype(_other(dtype))
    for pp, aa in ((f, np.asfortranarray(a)), (s, a[::2])):                       # and through the voxel wrapper
        v, ga = pcu.downsample_point_cloud_on_voxel_grid(0.1, pp, aa)
        v1, ga1 = pcu.downsample_point_cloud_on_voxel_grid(0.1, np.ascontiguousarray(pp), np.ascontiguousarray(aa))
        assert np.array_equal(v, v1) and np.array_equal(ga, ga1)


# ------------------------------------------------------------------------------------------------ 3. device-resident inputs
def _voxel_case(dtype, path):
    rng = np.random.default_rng(40)
    n = 50000
    if path == "packed":
        p = ((rng.random((n, 3)) - 0.5) * 3.0).astype(dtype)
        vs, mb, mxb = (0.1, 0.07, 0.2), (-0.35, 0.15, -0.85), (0.8, 0.9, 0.6)
    else:
        base = rng.uniform(-2e7, 2e7, (n // 2, 3))
        p = np.concatenate([base, np.floor(base) + rng.uniform(0.0, 1.0, (n // 2, 3))]).astype(dtype)[rng.permutation(n)]
        vs, mb, mxb = 1.0, (-2e7, -2e7, -2e7), (2e7 + 4, 2e7 + 4, 2e7 + 4)
    assert _path(voxel_widths(p, vs, mb)) == path
    return p, rng.standard_normal((n, 2)).astype(_other(dtype)), rng.random((n, 3), dtype=dtype), vs, mb, mxb


def _dedup_case(dtype, path):
    if path == "wide":
        p = unit_cube_rows(dtype, 50000)
    elif dtype == np.float32:
        p = unit_cube_rows(dtype, 50000, planar=True)
    else:
        rng = np.random.default_rng(41)
        p = np.empty((50000, 3), np.float64)
        p[:, 0] = 3.0; p[:, 1] = -0.125; p[:, 2] = np.round(rng.uniform(-1.0, 1.0, 50000), 3)
    assert _path(dedup_widths(p, 0.0)) == path
    return p


def _same_as_numpy(torch, got, want, dev):
    got = got if isinstance(got, tuple) else (got,); want = want if isinstance(want, tuple) else (want,)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert isinstance(g, torch.Tensor) and g.device == dev and tuple(g.shape) == w.shape and g.dtype == getattr(torch, w.dtype.name)
        assert np.array_equal(g.cpu().numpy(), w)


@pytest.mark.parametrize("path", ["packed", "wide"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_device_resident_voxels(pcu, dtype, path):
    """voxel_host.h voxel_downsample_impl with PCU_HIP_PTRS_ON_DEVICE: no staging, the caller's buffers written directly, every launch
    and copy on torch's current stream (_voxel.py _ctx_flags)."""
    import torch
    p, a0, a1, vs, mb, mxb = _voxel_case(dtype, path)
    want = pcu.downsample_point_cloud_on_voxel_grid(vs, p, a0, a1, min_bound=mb, max_bound=mxb)
    v0, b0 = oracle.voxel_downsample_fast(p, a0, [vs] * 3 if np.isscalar(vs) else vs, mb)
    assert np.array_equal(want[0], v0) and np.array_equal(want[1], b0) and len(want) == 3
    tp, ta0, ta1 = (torch.from_numpy(x).cuda() for x in (p, a0, a1))
    dev = tp.device
    _same_as_numpy(torch, pcu.downsample_point_cloud_on_voxel_grid(vs, tp, ta0, ta1, min_bound=mb, max_bound=mxb), want, dev)
    want_default = pcu.downsample_point_cloud_on_voxel_grid(vs, p, a0, a1)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):                 # inputs produced on the side stream: a launch on another stream could read them too early
        sp, sa0, sa1 = tp * 1, ta0 * 1, ta1 * 1
        got = pcu.downsample_point_cloud_on_voxel_grid(vs, sp, sa0, sa1, min_bound=mb, max_bound=mxb)
        got_default = pcu.downsample_point_cloud_on_voxel_grid(vs, sp, sa0, sa1)
    side.synchronize()
    _same_as_numpy(torch, got, want, dev)
    _same_as_numpy(torch, got_default, want_default, dev)
    with pytest.raises(ValueError):
        pcu.downsample_point_cloud_on_voxel_grid(vs, tp, a0, min_bound=mb, max_bound=mxb)                  # torch points, numpy attribute
    with pytest.raises(ValueError):
        pcu.downsample_point_cloud_on_voxel_grid(vs, p, ta0, min_bound=mb, max_bound=mxb)                  # numpy points, torch attribute
    with pytest.raises(ValueError):
        pcu.downsample_point_cloud_on_voxel_grid(vs, torch.from_numpy(p), min_bound=mb, max_bound=mxb)    # a tensor on the CPU
    with pytest.raises(ValueError):
        pcu.downsample_point_cloud_on_voxel_grid(vs, tp, torch.from_numpy(a0), min_bound=mb, max_bound=mxb)


@pytest.mark.parametrize("path", ["packed", "wide"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_device_resident_dedup(pcu, dtype, path):
    """voxel_host.h dedup_impl with PCU_HIP_PTRS_ON_DEVICE on torch's current stream."""
    import torch
    p = _dedup_case(dtype, path)
    for eps in (0.0, 1e-3):
        want = check_dedup(pcu, p, eps)
        tp = torch.from_numpy(p).cuda()
        _same_as_numpy(torch, pcu.deduplicate_point_cloud(tp, eps), want, tp.device)
        _same_as_numpy(torch, pcu.deduplicate_point_cloud(tp, eps, return_index=False), want[0], tp.device)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            got = pcu.deduplicate_point_cloud(tp * 1, eps)
        side.synchronize()
        _same_as_numpy(torch, got, want, tp.device)
    with pytest.raises(ValueError):
        pcu.deduplicate_point_cloud(torch.from_numpy(p), 0.0)


# ------------------------------------------------------------------------------------------------ 4. Morton
def test_morton_beyond_21_bits(pcu, mkind):
    """morton.h morton_encode3 (sign + low 20 bits of the int32), _voxel.py morton_encode's narrowing of int64 (int32_t px = pts(i, 0)),
    morton_decode3 of arbitrary patterns (bit 63 set included), morton_add2 / morton_negate across sign changes and carries out of bit 20."""
    rng = np.random.default_rng(50)
    n = 200000
    p32 = rng.integers(-(1 << 31), 1 << 31, (n, 3)).astype(np.int32)
    p32[:4] = [[-(1 << 31)] * 3, [(1 << 31) - 1] * 3, [1 << 20, -(1 << 20) - 1, 1 << 21], [-1, 0, 1]]
    p64 = rng.integers(-(1 << 40), 1 << 40, (n, 3)).astype(np.int64)
    p64[:4] = [[1 << 31, -(1 << 31) - 1, (1 << 32) + 5], [-(1 << 63), (1 << 63) - 1, 1 << 52], [(1 << 31) + (1 << 20), -(1 << 33) + 7, -1], [0, 1, -1]]
    assert np.any(np.abs(p64) > (1 << 31))
    for p in (p32, p64):
        codes = pcu.morton_encode(p)
        assert codes.dtype == np.uint64 and np.array_equal(codes, oracle.morton_encode(p, mkind))
    raw = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    raw[:3] = [0, (1 << 64) - 1, 1 << 63]
    assert np.any(raw >> np.uint64(63))
    assert np.array_equal(pcu.morton_decode(raw), oracle.morton_decode(raw, mkind))
    raw2 = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    edge = np.array([[(1 << 20) - 1, -(1 << 20), -1], [1, -1, 1], [0, 0, 0], [-1, 1, (1 << 20) - 1], [5, -5, -(1 << 20)]], np.int32)
    ea = oracle.morton_encode(edge[rng.integers(0, 5, n)], mkind); eb = oracle.morton_encode(edge[rng.integers(0, 5, n)], mkind)
    for a, b in ((raw, raw2), (ea, eb), (ea, raw2)):
        assert np.array_equal(pcu.morton_add(a, b), oracle.morton_addsub(a, b, False, mkind))
        assert np.array_equal(pcu.morton_subtract(a, b), oracle.morton_addsub(a, b, True, mkind))
    small = rng.integers(-3, 4, (n, 3)).astype(np.int32); other = rng.integers(-3, 4, (n, 3)).astype(np.int32)          # sums that change sign
    assert np.any(np.sign(small + other) != np.sign(small))
    assert np.array_equal(pcu.morton_decode(pcu.morton_add(pcu.morton_encode(small), pcu.morton_encode(other))), small + other)
    assert np.array_equal(pcu.morton_decode(pcu.morton_subtract(pcu.morton_encode(small), pcu.morton_encode(other))), small - other)
    with pytest.raises(ValueError, match="same number of entries"):
        pcu.morton_add(raw, raw2[:-1])
    with pytest.raises(ValueError, match="same number of entries"):
        pcu.morton_subtract(raw[:10], raw2)
    with pytest.raises(ValueError, match="invalid shape"):
        pcu.morton_decode(raw.reshape(-1, 2))
    with pytest.raises(ValueError, match="invalid shape"):
        pcu.morton_add(raw.reshape(-1, 2), raw2.reshape(-1, 2))


def test_morton_grid_stride_trip(pcu, mkind):
    """morton.h k_morton_encode / k_morton_decode: the grid is capped at 65 536 blocks of 256; row 65 536 x 256 and later are the second
    trip of the grid-stride loop (voxel_host.h morton_map_impl)."""
    n = 65536 * 256 + 257
    rng = np.random.default_rng(51)
    p = rng.integers(-(1 << 31), 1 << 31, (n, 3), dtype=np.int64).astype(np.int32)
    codes = pcu.morton_encode(p)
    want = oracle.morton_encode(p, mkind)
    assert codes.shape == (n,) and np.array_equal(codes, want)
    del p
    back = pcu.morton_decode(want)
    assert back.shape == (n, 3) and np.array_equal(back, oracle.morton_decode(want, mkind))


def _knn_expect(codes, q, k, mkind):
    """(window, window in ascending squared distance of the decoded integers, ties: lower index first)"""
    win = oracle.morton_knn_window(codes, q, k, mkind)
    pc = oracle.morton_decode(codes, mkind).astype(np.int64); pq = oracle.morton_decode(q, mkind).astype(np.int64)
    d2 = ((pc[win] - pq[:, None, :]) ** 2).sum(-1)
    return win, np.take_along_axis(win, np.argsort(d2, axis=1, kind="stable"), axis=1), d2


def test_morton_knn_duplicates_ends_and_ties(pcu, mkind):
    """morton.h k_morton_knn: the lower bound on runs of equal codes (first of the run), queries below the first / above the last code, the
    window's shifts at both ends, k = 1, k = n, k > n, n = 1, uint32 codes, and the stated order of sort_dist=True (ties: lower index first)."""
    rng = np.random.default_rng(52)
    pts = rng.integers(0, 6, (4000, 3)).astype(np.int32)                          # a 6^3 lattice: 216 codes, runs of ~18 duplicates, many equal distances
    codes = np.sort(oracle.morton_encode(pts, mkind))
    qp = rng.integers(-2, 8, (3000, 3)).astype(np.int32)
    qp[:3] = [[-2, -2, -2], [7, 7, 7], pts[0]]
    q = oracle.morton_encode(qp, mkind)
    assert len(np.unique(codes)) == 216 and np.any(q < codes[0]) and np.any(q > codes[-1]) and np.isin(q, codes).sum() > 500
    ties = 0
    for c, qq, ks in ((codes, q, (1, 2, 7, 16, 33)), (codes[:37], q, (36, 37, 50)), (codes[:1], q, (1, 5)),
                      (codes[::100].astype(np.uint32), q.astype(np.uint32), (1, 4, 9))):
        if c.dtype == np.uint32:
            assert np.array_equal(np.sort(c), c)
        for k in ks:
            win, srt, d2 = _knn_expect(c, qq, k, mkind)
            got = pcu.morton_knn(c, qq, k, sort_dist=False)
            assert got.dtype == np.int64 and got.shape == (len(qq), min(k, len(c))) and np.array_equal(got, win)
            assert np.array_equal(pcu.morton_knn(c, qq, k), srt)
            ties += int((np.diff(np.sort(d2, axis=1), axis=1) == 0).sum())
    assert ties > 10000
    # random uint32 codes and queries (no lattice)
    c32 = np.sort(rng.integers(0, 1 << 32, 5000, dtype=np.uint64).astype(np.uint32)); q32 = rng.integers(0, 1 << 32, 2000, dtype=np.uint64).astype(np.uint32)
    q32[:100] = c32[rng.integers(0, 5000, 100)]
    win, srt, _ = _knn_expect(c32, q32, 8, mkind)
    assert np.array_equal(pcu.morton_knn(c32, q32, 8, sort_dist=False), win) and np.array_equal(pcu.morton_knn(c32, q32, 8), srt)
    with pytest.raises(ValueError, match="Expected it to match"):
        pcu.morton_knn(codes, q.astype(np.uint32), 3)
    with pytest.raises(ValueError, match="invalid shape"):
        pcu.morton_knn(codes.reshape(-1, 2), q, 3)
    import torch
    with pytest.raises(ValueError):
        pcu.morton_knn(codes, torch.from_numpy(q.view(np.int64)).cuda(), 3)       # numpy codes, torch queries


# ------------------------------------------------------------------------------------------------ 5. Python-side checks of _voxel.py
def test_voxel_argument_checks_and_attribute_shapes(pcu):
    rng = np.random.default_rng(60)
    n = 4000
    p = rng.random((n, 3))
    a = rng.standard_normal((n, 4)).astype(np.float32)
    with pytest.raises(ValueError, match="Invalid voxel size must be a 3-tuple or a single float"):
        pcu.downsample_point_cloud_on_voxel_grid((0.1, 0.1), p)
    with pytest.raises(ValueError, match="min_bound must be a 3 tuple"):
        pcu.downsample_point_cloud_on_voxel_grid(0.1, p, min_bound=(0, 0), max_bound=(1, 1, 1))
    with pytest.raises(ValueError, match="max_bound must be a 3 tuple"):
        pcu.downsample_point_cloud_on_voxel_grid(0.1, p, min_bound=(0, 0, 0), max_bound=(1, 1))
    with pytest.raises(ValueError, match="Voxel size is too small"):
        pcu.downsample_point_cloud_on_voxel_grid(1e-3, p, min_bound=(0, 0, 0), max_bound=(1e12, 1e12, 1e12))
    with pytest.raises(ValueError, match="points must be a numpy array"):
        pcu.downsample_point_cloud_on_voxel_grid(0.1, p.tolist())
    with pytest.raises(ValueError, match="must be numpy arrays"):
        pcu.downsample_point_cloud_on_voxel_grid(0.1, p, a.tolist())
    v2, a2 = pcu.downsample_point_cloud_on_voxel_grid(0.1, p, a)
    v0, a0 = oracle.voxel_downsample_fast(p, a, [0.1] * 3, _default_bounds(p, 0.1)[0])
    assert np.array_equal(v2, v0) and np.array_equal(a2, a0)
    v1, a1 = pcu.downsample_point_cloud_on_voxel_grid(0.1, p, a[:, 0])            # (n,) -> (m,)
    assert a1.shape == (len(v2),) and a1.dtype == np.float32 and np.array_equal(v1, v2) and np.array_equal(a1, a2[:, 0])
    v3, a3 = pcu.downsample_point_cloud_on_voxel_grid(0.1, p, a.reshape(n, 2, 2))  # (n, 2, 2) -> (m, 2, 2)
    assert a3.shape == (len(v2), 2, 2) and a3.dtype == np.float32 and np.array_equal(v3, v2) and np.array_equal(a3.reshape(len(v2), 4), a2)
