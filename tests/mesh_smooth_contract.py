"""The contract of mesh_vertex_adjacency / adjacency_list, estimate_mesh_vertex_normals and laplacian_smooth_mesh restated
in numpy, the float64 direct solve the smoothing is measured against, and the meshes the tests share. Nothing here imports the package.

Sums whose order the contract fixes (a vertex's corners, the duplicates of a directed pair, a row's entries) are taken in that order, one
addition at a time, in the dtype; the conjugate-gradient dot products use numpy's own summation, which the contract does not fix for a
restatement: the smoothing is compared within a tolerance, never bit for bit."""
import numpy as np

CG_CAP = 4096


# ---------------------------------------------------------------------------------------------------- structure
def adjacency_sets(f, nv):
    """The adjacency by a loop over Python sets: (offsets int64 (nv + 1), neighbours int64)."""
    rows = [set() for _ in range(nv)]
    for a, b, c in np.asarray(f).tolist():
        for i, j in ((a, b), (b, a), (a, c), (c, a), (b, c), (c, b)):
            if i != j:
                rows[i].add(j)
    off = np.zeros(nv + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(r) for r in rows])
    nb = np.array([j for r in rows for j in sorted(r)], dtype=np.int64)
    return off, nb


def incidence(f, nv):
    """(pos (nv + 1), corner ids): the corners 3 t + c of vertex i are ids[pos[i]:pos[i + 1]], ascending."""
    keys = np.asarray(f).astype(np.int64).reshape(-1)
    ids = np.argsort(keys, kind="stable")
    pos = np.searchsorted(keys[ids], np.arange(nv + 1), side="left")
    return pos.astype(np.int64), ids.astype(np.int64)


def _ordered_sums(vals, gid, ngroups):
    """acc[g] = ((0 + v_0) + v_1) + ... over the items of group g in the order given (items sorted by group), one addition at a time."""
    vals = np.asarray(vals)
    acc = np.zeros((ngroups,) + vals.shape[1:], dtype=vals.dtype)
    if len(gid) == 0:
        return acc
    start = np.searchsorted(gid, np.arange(ngroups), side="left")
    rank = np.arange(len(gid)) - start[gid]
    order = np.argsort(rank, kind="stable")
    cuts = np.cumsum(np.bincount(rank))
    lo = 0
    for hi in cuts:
        sel = order[lo:hi]
        acc[gid[sel]] = acc[gid[sel]] + vals[sel]
        lo = hi
    return acc


def pairs(f, nv):
    """The sorted directed pairs: (row, col, corner id) of every non-self pair, sorted by (row, col), duplicates ascending by corner."""
    f = np.asarray(f).astype(np.int64)
    nf = len(f)
    c = np.arange(3 * nf)
    t, cc = c // 3, c % 3
    j, k = f[t, (cc + 1) % 3], f[t, (cc + 2) % 3]
    row = np.stack([j, k], axis=1).reshape(-1)
    col = np.stack([k, j], axis=1).reshape(-1)
    corner = np.repeat(c, 2)
    order = np.argsort(row * nv + col, kind="stable")
    row, col, corner = row[order], col[order], corner[order]
    keep = row != col
    return row[keep], col[keep], corner[keep]


def adjacency(f, nv):
    """The contract's CSR: (offsets int64 (nv + 1), neighbours int64) by one sort, run heads and a count."""
    row, col, _ = pairs(f, nv)
    key = row * nv + col
    head = np.ones(len(key), dtype=bool)
    head[1:] = key[1:] != key[:-1]
    off = np.zeros(nv + 1, dtype=np.int64)
    off[1:] = np.cumsum(np.bincount(row[head], minlength=nv))
    return off, col[head]


# ---------------------------------------------------------------------------------------------------- geometry in the dtype
def _cross(e1, e2):
    return np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)


def _dot(x, y):
    return (x[:, 0] * y[:, 0] + x[:, 1] * y[:, 1]) + x[:, 2] * y[:, 2]


def face_normals(v, f):
    """(N, |N|, unit normal) per face, in v's dtype."""
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    N = _cross(b - a, c - a)
    r = np.sqrt(_dot(N, N))
    with np.errstate(invalid="ignore", divide="ignore"):
        unit = np.where((r == 0)[:, None], v.dtype.type(0), N / r[:, None])
    return N, r, unit.astype(v.dtype)


def corner_terms(v, f):
    """(|e1 x e2|, e1 . e2) for every corner 3 t + c, in v's dtype."""
    f = np.asarray(f).astype(np.int64)
    nf = len(f)
    c = np.arange(3 * nf)
    t, cc = c // 3, c % 3
    p, q, r = v[f[t, cc]], v[f[t, (cc + 1) % 3]], v[f[t, (cc + 2) % 3]]
    e1, e2 = q - p, r - p
    X = _cross(e1, e2)
    return np.sqrt(_dot(X, X)), _dot(e1, e2)


def vertex_normals(v, f, weighting="uniform"):
    """The serial restatement in v's dtype."""
    v = np.ascontiguousarray(v)
    f = np.asarray(f).astype(np.int64)
    nv = len(v)
    N, _, unit = face_normals(v, f)
    pos, ids = incidence(f, nv)
    t = ids // 3
    if weighting == "uniform":
        contrib = unit[t]
    elif weighting == "area":
        contrib = N[t]
    elif weighting == "angle":
        length, dot = corner_terms(v, f)
        contrib = unit[t] * np.arctan2(length, dot)[ids][:, None]
    else:
        raise ValueError(weighting)
    gid = np.repeat(np.arange(nv), np.diff(pos))
    s = _ordered_sums(contrib.astype(v.dtype), gid, nv)
    r = np.sqrt(_dot(s, s))
    with np.errstate(invalid="ignore", divide="ignore"):
        out = np.where((r == 0)[:, None], v.dtype.type(0), s / r[:, None])
    return out.astype(v.dtype)


def cot_matrix(v, f):
    """L without its diagonal as CSR (offsets, columns, values) and the diagonal, in v's dtype."""
    v = np.ascontiguousarray(v)
    T = v.dtype.type
    nv = len(v)
    length, dot = corner_terms(v, f)
    with np.errstate(invalid="ignore", divide="ignore"):
        w = np.where(length == 0, T(0), (T(0.5) * dot) / length).astype(v.dtype)
    row, col, corner = pairs(f, nv)
    key = row * nv + col
    head = np.ones(len(key), dtype=bool)
    head[1:] = key[1:] != key[:-1]
    entry = np.cumsum(head) - 1
    ne = int(head.sum())
    val = _ordered_sums(w[corner], entry, ne)
    erow, ecol = row[head], col[head]
    off = np.zeros(nv + 1, dtype=np.int64)
    off[1:] = np.cumsum(np.bincount(erow, minlength=nv))
    diag = -_ordered_sums(val, erow, nv)
    return off, ecol, val, diag


def mass(u, f):
    """M_ii = (sum of |N| over the incidence of i) / 6, in u's dtype."""
    f = np.asarray(f).astype(np.int64)
    nv = len(u)
    _, r, _ = face_normals(u, f)
    pos, ids = incidence(f, nv)
    gid = np.repeat(np.arange(nv), np.diff(pos))
    return _ordered_sums(r[ids // 3], gid, nv) / u.dtype.type(6)


def rescale(u, f, M):
    """u <- (u - c) / sqrt(A) + c for the vertices with M != 0."""
    T = u.dtype.type
    f = np.asarray(f).astype(np.int64)
    _, r, _ = face_normals(u, f)
    bary = ((u[f[:, 0]] + u[f[:, 1]]) + u[f[:, 2]]) / T(3)
    total = r.sum(dtype=u.dtype)
    A = T(0.5) * total
    c = (r[:, None] * bary).sum(axis=0, dtype=u.dtype) / total
    out = u.copy()
    live = M != 0
    out[live] = (u[live] - c) / np.sqrt(A) + c
    return out


def _spmv(off, col, val, x, D, h, live):
    prod = val[:, None] * x[col]
    a = np.zeros_like(x)
    counts = np.diff(off)
    rows = np.nonzero(counts)[0]
    if len(rows):
        a[rows] = np.add.reduceat(prod, off[rows], axis=0)
    y = D[:, None] * x - h * a
    y[~live] = 0
    return y


def solve_cg(off, col, val, diag, M, h, u):
    """(M - h L) x = M u by Jacobi-preconditioned conjugate gradients from x0 = u, in u's dtype. Returns (x, iterations)."""
    T = u.dtype.type
    tol2 = (T(64) * np.finfo(u.dtype).eps) ** 2
    live = M != 0
    D = M - h * diag
    x = u.copy()
    b = M[:, None] * u
    r = b - _spmv(off, col, val, x, D, h, live)
    r[~live] = 0
    Dsafe = np.where(live, D, T(1))
    z = r / Dsafe[:, None]
    p = z.copy()
    rz = (r * z).sum(axis=0, dtype=u.dtype)
    bb = (b * b).sum(axis=0, dtype=u.dtype)
    done = (r * r).sum(axis=0, dtype=u.dtype) <= tol2 * bb
    iters = 0
    while not done.all():
        if iters == CG_CAP:
            raise RuntimeError("the conjugate-gradient solve has not converged")
        Ap = _spmv(off, col, val, p, D, h, live)
        pAp = (p * Ap).sum(axis=0, dtype=u.dtype)
        if not (pAp[~done] > 0).all():
            raise RuntimeError("p.Ap <= 0")
        run = ~done
        alpha = np.where(run, rz / np.where(run, pAp, T(1)), T(0)).astype(u.dtype)
        x[:, run] = x[:, run] + alpha[run] * p[:, run]
        r[:, run] = r[:, run] - alpha[run] * Ap[:, run]
        z[:, run] = r[:, run] / Dsafe[:, None]
        rz_new = (r * z).sum(axis=0, dtype=u.dtype)
        rr = (r * r).sum(axis=0, dtype=u.dtype)
        beta = np.where(run, rz_new / np.where(run, rz, T(1)), T(0)).astype(u.dtype)
        rz = np.where(run, rz_new, rz)
        done = done | (run & (rr <= tol2 * bb))
        p[:, run] = z[:, run] + beta[run] * p[:, run]
        iters += 1
    return x, iters


def smooth(v, f, num_iters, step_size=0.1, use_cotan_weights=False):
    """The contract in v's dtype. Returns (u, [iterations of every solve])."""
    v = np.ascontiguousarray(v)
    T = v.dtype.type
    off, col, val, diag = cot_matrix(v, f)
    h = T(step_size * 1e-3 if use_cotan_weights else step_size)
    u = v.copy()
    counts = []
    for _ in range(num_iters):
        M = mass(u, f) if use_cotan_weights else np.ones(len(v), dtype=v.dtype)
        u, it = solve_cg(off, col, val, diag, M, h, u)
        counts.append(it)
        if use_cotan_weights:
            u = rescale(u, f, M)
    return u, counts


def system_matrix(off, col, val, diag, M, h):
    """M - h L, dense, with the identity in the row of a vertex whose M is zero."""
    nv = len(M)
    A = np.zeros((nv, nv), dtype=val.dtype)
    rows = np.repeat(np.arange(nv), np.diff(off))
    A[rows, col] = -h * val
    A[np.arange(nv), np.arange(nv)] = M - h * diag
    dead = M == 0
    A[dead] = 0
    A[dead, dead] = 1
    return A


def smooth_direct(v, f, num_iters, step_size=0.1, use_cotan_weights=False, sparse=False):
    """The same iteration in float64 with a direct solve (numpy's dense one, or scipy's sparse one)."""
    v = np.ascontiguousarray(v, dtype=np.float64)
    off, col, val, diag = cot_matrix(v, f)
    h = np.float64(step_size * 1e-3 if use_cotan_weights else step_size)
    u = v.copy()
    nv = len(v)
    for _ in range(num_iters):
        M = mass(u, f) if use_cotan_weights else np.ones(nv)
        b = M[:, None] * u
        b[M == 0] = u[M == 0]
        if sparse:
            import scipy.sparse as sp
            import scipy.sparse.linalg as spl
            live = M != 0
            rows = np.repeat(np.arange(nv), np.diff(off))
            keep = live[rows]
            A = sp.csr_matrix((-h * val[keep], (rows[keep], col[keep])), shape=(nv, nv)) + sp.diags(np.where(live, M - h * diag, 1.0))
            u = np.asarray(spl.spsolve(A.tocsc(), b))
        else:
            u = np.linalg.solve(system_matrix(off, col, val, diag, M, h), b)
        if use_cotan_weights:
            u = rescale(u, f, M)
    return u


def dense_system_by_faces(v, f, h, M=None):
    """M - h L in float64 built independently: a loop over the faces that adds 0.5 cot of every corner to the opposite edge."""
    v = np.asarray(v, dtype=np.float64)
    nv = len(v)
    L = np.zeros((nv, nv))
    for tri in np.asarray(f).tolist():
        for c in range(3):
            i, j, k = tri[c], tri[(c + 1) % 3], tri[(c + 2) % 3]
            e1, e2 = v[j] - v[i], v[k] - v[i]
            s = np.linalg.norm(np.cross(e1, e2))
            w = 0.0 if s == 0 else 0.5 * np.dot(e1, e2) / s
            if j != k:
                L[j, k] += w; L[k, j] += w
                L[j, j] -= w; L[k, k] -= w
    Mm = np.eye(nv) if M is None else np.diag(M)
    return Mm - h * L


def surface_area(v, f):
    v = np.asarray(v, dtype=np.float64)
    return 0.5 * np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1).sum()


# ---------------------------------------------------------------------------------------------------- meshes
def tetrahedron():
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    f = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]])
    return v, f


def sphere(levels):
    """An octahedron subdivided `levels` times onto the unit sphere: 4^levels * 4 + 2 vertices (258 at 3, 4,098 at 5), slightly squashed so
    that no two coordinates are symmetric."""
    v = np.array([[1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [0, -1.0, 0], [0, 0, 1.0], [0, 0, -1.0]])
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])
    for _ in range(levels):
        n = len(v)
        e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
        uniq, inv = np.unique(e[:, 0] * n + e[:, 1], return_inverse=True)
        mid = v[uniq // n] + v[uniq % n]
        mid /= np.linalg.norm(mid, axis=1)[:, None]
        v = np.concatenate([v, mid])
        m = n + inv.reshape(3, -1)
        a, b, c = f[:, 0], f[:, 1], f[:, 2]
        f = np.concatenate([np.stack([a, m[0], m[2]], 1), np.stack([m[0], b, m[1]], 1), np.stack([m[2], m[1], c], 1), np.stack([m[0], m[1], m[2]], 1)])
    return v * np.array([1.0, 0.9, 1.1]) + np.array([0.1, -0.2, 0.3]), f


def grid(n=33):
    """An open n x n height field: boundary rows have fewer neighbours."""
    x, y = np.meshgrid(np.linspace(0, 1, n), np.linspace(0, 1.3, n), indexing="ij")
    z = 0.1 * np.sin(5 * x) * np.cos(3 * y)
    v = np.stack([x, y, z], axis=-1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij")
    a = (i * n + j).reshape(-1)
    f = np.concatenate([np.stack([a, a + n, a + 1], 1), np.stack([a + 1, a + n, a + n + 1], 1)])
    return v, f


def fan(k=700):
    """k faces round one apex (vertex 0): a valence above a wave, a block and a sort tile."""
    ang = np.linspace(0, 2 * np.pi, k, endpoint=False)
    ring = np.stack([np.cos(ang), np.sin(ang), 0.05 * np.cos(7 * ang)], axis=1)
    v = np.concatenate([[[0.0, 0.0, 0.4]], ring])
    i = np.arange(k)
    f = np.stack([np.zeros(k, dtype=np.int64), 1 + i, 1 + (i + 1) % k], axis=1)
    return v, f


def book(k=300):
    """k faces on one shared edge (vertices 0 and 1): one run of 2 k duplicates per direction."""
    ang = np.linspace(0.1, 2 * np.pi - 0.1, k)
    pages = np.stack([0.5 + 0.1 * np.sin(3 * ang), np.cos(ang), np.sin(ang)], axis=1)
    v = np.concatenate([[[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]], pages])
    f = np.stack([np.zeros(k, dtype=np.int64), np.ones(k, dtype=np.int64), 2 + np.arange(k)], axis=1)
    return v, f


def defective_sphere():
    """The 258-vertex sphere with a duplicated face, a face without area (three collinear vertices), a face that lists a vertex twice, and
    vertices that no face lists in the middle and at the end. Returns (v, f, unreferenced vertex ids)."""
    v, f = sphere(3)
    n = len(v)
    mid = n // 2
    v = np.concatenate([v[:mid], [[5.0, 5.0, 5.0], [6.0, 5.0, 5.0], [7.0, 5.0, 5.0], [9.0, 9.0, 9.0]], v[mid:], [[-3.0, 2.0, 1.0], [4.0, 4.0, -4.0]]])
    f = np.where(f >= mid, f + 4, f)
    extra = np.array([f[10], [mid, mid + 1, mid + 2], [f[20, 0], f[20, 1], f[20, 1]]])
    f = np.concatenate([f[:100], extra, f[100:]])
    return v, f, np.array([mid + 3, n + 4, n + 5])


def permuted_sphere(seed=3):
    v, f = sphere(3)
    perm = np.random.default_rng(seed).permutation(len(v))
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(v))
    return v[perm], inv[f]


def golden(name):
    import os
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    return np.load(os.path.join(here, name + "_v.npy")).astype(np.float64), np.load(os.path.join(here, name + "_f.npy")).astype(np.int64)


_MESHES = {"tetrahedron": tetrahedron, "sphere258": lambda: sphere(3), "sphere4098": lambda: sphere(5), "grid33": grid, "fan700": fan, "book300": book,
           "defective": lambda: defective_sphere()[:2], "permuted": permuted_sphere, "cube_twist": lambda: golden("cube_twist"), "bunny": lambda: golden("bunny")}
MESH_NAMES = list(_MESHES)
_CACHE = {}


def mesh(name):
    """(v float64, f int64) of a named mesh, made once."""
    if name not in _CACHE:
        v, f = _MESHES[name]()
        _CACHE[name] = (np.ascontiguousarray(v, dtype=np.float64), np.ascontiguousarray(f, dtype=np.int64))
    return _CACHE[name]
