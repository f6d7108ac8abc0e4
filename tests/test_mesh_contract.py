"""closest_points_on_mesh on the CPU: the contract (tests/mesh_contract.py) against an independent float64 formulation, degenerate and needle
faces, validation before any device work, and the no-FMA rule of the k_mesh_* kernels on the shipped binary.

The bound B. |d - d64| <= B * eps(T) * scale, scale = the largest absolute coordinate of the case (mesh and queries). Measured with this
restatement on these inputs (bunny and an 8192-face sphere; box / surface / vertex / far queries, 1000 and 500 each): the largest excess was
0.912 eps*scale in float32 and 1.001 in float64; over the degenerate cases below it was 1.040 (a face collapsed to a point, float32). B is four
times the largest of these, 4.16 (the factor covers inputs the sample did not draw); every test prints its figure before it asserts."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import mesh_contract as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = mc.B
DTYPES = [np.float32, np.float64]


def _excess(d, d64, T, scale):
    return float(np.max(np.abs(d.astype(np.float64) - d64)) / (np.finfo(T).eps * scale))


@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("mesh", ["bunny", "sphere"])
def test_restatement_agrees_with_independent_float64(T, mesh):
    v, f = mc.bunny(T) if mesh == "bunny" else mc.sphere(32, T)
    n = 1000 if mesh == "bunny" else 500
    for kind, q in mc.query_sets(v, f, n, T).items():
        scale = max(float(np.abs(v).max()), float(np.abs(q).max()))
        d, fi, bc = mc.closest_brute(q, v, f)
        assert d.dtype == T and bc.dtype == T and not np.isnan(d).any() and not np.isnan(bc).any()
        ex = _excess(d, mc.mesh_distance64(q, v, f), T, scale)
        rep = _excess(d, mc.reproduce64(q, v, f, fi, bc), T, scale)
        print(f"{mesh} {np.dtype(T).name} {kind}: excess {ex:.3f} eps*scale, d reproduced from (fi, bc) within {rep:.3f}")
        assert ex <= B and rep <= B, (mesh, kind, ex, rep)


def _degenerate_case(T, seed):
    """Vertices 0..5: random; 6, 7, 8: collinear and distinct, and collinear to the arithmetic too (one edge is twice the other, so the
    edge dot products are exact multiples and va = vb = vc = 0; any other ratio is a needle of height zero plus rounding: the next test and
    README "Limits"). Faces: the five degenerate kinds."""
    rng = np.random.default_rng(seed)
    v = rng.random((9, 3))
    v[6] = [0.25, 0.5, 0.125]; v[7] = [0.5, 0.75, 0.25]; v[8] = [0.75, 1.0, 0.375]         # v7 - v6 = (.25, .25, .125), v8 - v6 = 2 (v7 - v6)
    f = np.concatenate([mc.degenerate_faces(0, 1), mc.degenerate_faces(3, 4), [[6, 7, 8], [8, 6, 7], [7, 8, 6]]]).astype(np.int64)
    ends = [(0, 1), (0, 0), (0, 1), (0, 1), (3, 4), (3, 3), (3, 4), (3, 4), (6, 8), (6, 8), (6, 8)]     # the segment (or point) every face is
    q = (rng.random((400, 3)) * 3 - 1).astype(T)
    return v.astype(T), f, ends, q


@pytest.mark.parametrize("T", DTYPES)
def test_degenerate_faces_alone_are_segments_and_points(T):
    v, f, ends, q = _degenerate_case(T, 3)
    scale = max(float(np.abs(v).max()), float(np.abs(q).max()))
    v64, q64 = v.astype(np.float64), q.astype(np.float64)
    for row, (i, j) in zip(f, ends):
        d2, vv, ww = mc.face_d2(q, v[row[0]][None], v[row[1]][None], v[row[2]][None])
        assert not np.isnan(d2).any() and not np.isnan(vv).any() and not np.isnan(ww).any(), row
        want = mc._segment64(q64, v64[i][None], v64[j][None])
        ex = _excess(np.sqrt(d2), want, T, scale)
        print(f"face {row.tolist()} {np.dtype(T).name}: excess {ex:.3f} eps*scale")
        assert ex <= B, (row, ex)


@pytest.mark.parametrize("T", DTYPES)
def test_degenerate_faces_mixed_into_the_bunny(T):
    v, f = mc.bunny(T)
    rng = np.random.default_rng(9)
    v = np.concatenate([v, np.array([[0.0625, 0.125, 0.03125], [0.125, 0.1875, 0.0625], [0.1875, 0.25, 0.09375]], dtype=T)])     # exactly collinear
    extra = [np.array([[len(v) - 3, len(v) - 2, len(v) - 1], [len(v) - 1, len(v) - 3, len(v) - 2]], dtype=np.int64)]
    for _ in range(40):
        i, j = rng.choice(len(v), 2, replace=False)
        extra.append(mc.degenerate_faces(int(i), int(j)))
    f2 = np.concatenate([f] + extra)
    f2 = f2[rng.permutation(len(f2))]
    q = np.concatenate([a[:150] for a in mc.query_sets(v, f2, 150, T).values()])
    scale = max(float(np.abs(v).max()), float(np.abs(q).max()))
    d, fi, bc = mc.closest_brute(q, v, f2)
    assert not np.isnan(d).any() and not np.isnan(bc).any()
    ex = _excess(d, mc.mesh_distance64(q, v, f2), T, scale)
    rep = _excess(d, mc.reproduce64(q, v, f2, fi, bc), T, scale)
    print(f"bunny + degenerate faces {np.dtype(T).name}: excess {ex:.3f}, reproduced within {rep:.3f}")
    assert ex <= B and rep <= B


@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("height", [1e-1, 1e-3, 1e-5, 1e-7, 1e-10])
def test_properties_on_soups_and_needles(T, height):
    """No NaN; bc sums to 1 within 2 eps and no coordinate is below -eps (u = (1 - v) - w is two roundings); d is the distance of the point
    (fi, bc) stand for. (A needle thinner than the rounding of its coordinates may miss the true minimum: README, "Limits".)"""
    eps = np.finfo(T).eps
    v, f = mc.needle_soup(1500, height, T, seed=int(-np.log10(height)))
    q = np.random.default_rng(4).random((300, 3)).astype(T)
    scale = max(float(np.abs(v).max()), 1.0)
    d, fi, bc = mc.closest_brute(q, v, f)
    assert not np.isnan(d).any() and not np.isnan(bc).any()
    s = float(np.abs(bc.astype(np.float64).sum(1) - 1).max() / eps)
    lo = float(bc.min() / eps)
    rep = _excess(d, mc.reproduce64(q, v, f, fi, bc), T, scale)
    print(f"height {height:g} {np.dtype(T).name}: sum off by {s:.3f} eps, smallest coordinate {lo:.3f} eps, d reproduced within {rep:.3f} eps*scale")
    assert s <= 2 and lo >= -1 and rep <= B


@pytest.mark.parametrize("T", DTYPES)
def test_inexactly_collinear_triangle_keeps_the_properties(T):
    """Collinear corners whose edge ratio is not a power of two (here 3): the edge dot products round differently, va / vb / vc are rounding
    noise of either sign and the region tests can misjudge the face, as for any needle thinner than the rounding of its coordinates. The
    returned point is still a point of the face and d is its distance; d may exceed the distance to the segment (measured here: up to 1.3e3
    eps*scale in float32)."""
    eps = np.finfo(T).eps
    v = np.array([[0.25, 0.5, 0.125], [0.5, 0.75, 0.25], [1.0, 1.25, 0.5]], dtype=T)
    q = (np.random.default_rng(3).random((400, 3)) * 3 - 1).astype(T)
    for row in ([0, 1, 2], [2, 0, 1], [1, 2, 0]):
        f = np.array([row], dtype=np.int64)
        d, fi, bc = mc.closest_brute(q, v, f)
        assert not np.isnan(d).any() and not np.isnan(bc).any()
        assert np.abs(bc.astype(np.float64).sum(1) - 1).max() <= 2 * eps and bc.min() >= -eps
        assert _excess(d, mc.reproduce64(q, v, f, fi, bc), T, float(np.abs(q).max())) <= B
        assert np.all(d.astype(np.float64) >= mc.mesh_distance64(q, v, f) - B * eps * 2.0)


def test_first_minimum_wins_on_exact_ties():
    """Two copies of one triangle and a neighbour sharing an edge: the lowest face index among equal d2."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], dtype=np.float32)
    f = np.array([[1, 3, 2], [0, 1, 2], [0, 1, 2]], dtype=np.int64)
    q = np.array([[0.25, 0.25, 1.0], [0.5, 0.5, 2.0], [2.0, 2.0, 0.0]], dtype=np.float32)
    d, fi, bc = mc.closest_brute(q, v, f)
    assert fi.tolist() == [1, 0, 0] and np.allclose(d, [1.0, 2.0, np.sqrt(2.0)])


# ---------------------------------------------------------------------------------------------------- validation (numpy input: no device work)
def _mesh():
    v = np.random.default_rng(0).random((8, 3)).astype(np.float32)
    f = np.array([[0, 1, 2], [2, 3, 4], [5, 6, 7]], dtype=np.int64)
    return np.random.default_rng(1).random((5, 3)).astype(np.float32), v, f


def test_validation_errors_are_raised_before_the_gpu_is_touched():
    import point_cloud_utils_amd as pcu
    p, v, f = _mesh()
    with pytest.raises(ValueError, match=r"Invalid scalar type \(int32\) for argument 'p'"):
        pcu.closest_points_on_mesh(p.astype(np.int32), v, f)
    with pytest.raises(ValueError, match=r"Invalid scalar type \(float64\) for argument 'v'. Expected it to match argument 'p' which is of type float32"):
        pcu.closest_points_on_mesh(p, v.astype(np.float64), f)
    with pytest.raises(ValueError, match=r"Invalid scalar type \(float32\) for argument 'f'"):
        pcu.closest_points_on_mesh(p, v, f.astype(np.float32))
    with pytest.raises(ValueError, match=r"Invalid scalar type \(int16\) for argument 'f'"):
        pcu.closest_points_on_mesh(p, v, f.astype(np.int16))
    with pytest.raises(ValueError, match=r"Only 3D inputs are supported: v must have shape \(n, 3\) \(n > 0\)\. Got points\.shape =\(5, 2\)\."):
        pcu.closest_points_on_mesh(p[:, :2], v, f)
    with pytest.raises(ValueError, match=r"Invalid input mesh with zero elements: v and f must have shape \(n, 3\) and \(m, 3\) \(n, m > 0\)\. Got v\.shape =\(0, 3\), f\.shape = \(3, 3\)\."):
        pcu.closest_points_on_mesh(p, v[:0], f)
    with pytest.raises(ValueError, match=r"Invalid input mesh with zero elements.*f\.shape = \(0, 3\)"):
        pcu.closest_points_on_mesh(p, v, f[:0])
    with pytest.raises(ValueError, match=r"Only 3D inputs are supported: v and f must have shape \(n, 3\) and \(m, 3\) \(n, m > 0\)\. Got v\.shape =\(8, 3\), f\.shape = \(3, 2\)\."):
        pcu.closest_points_on_mesh(p, v, f[:, :2])
    with pytest.raises(ValueError, match=r"Only 3D inputs are supported: v and f.*v\.shape =\(8, 2\)"):
        pcu.closest_points_on_mesh(p, v[:, :2], f)
    for bad in (np.nan, np.inf, -np.inf):
        pb = p.copy(); pb[3, 1] = bad
        with pytest.raises(ValueError, match="p must not contain NaN or infinite coordinates"):
            pcu.closest_points_on_mesh(pb, v, f)
        vb = v.copy(); vb[7, 2] = bad                       # (referenced or not: any row of v)
        with pytest.raises(ValueError, match="v must not contain NaN or infinite coordinates"):
            pcu.closest_points_on_mesh(p, vb, f)
    for dt, badval in ((np.int64, 8), (np.int64, -1), (np.int32, -1), (np.uint32, 8), (np.uint64, 2 ** 63)):
        fb = f.astype(dt); fb[1, 2] = badval
        with pytest.raises(ValueError, match=r"found a face index outside \[0, 8\)"):
            pcu.closest_points_on_mesh(p, v, fb)
    big = np.lib.stride_tricks.as_strided(np.zeros(3, dtype=np.float32), shape=(2 ** 27 - 15, 3), strides=(0, 4))
    with pytest.raises(ValueError, match=r"more than 2\^27-16 rows"):
        pcu.closest_points_on_mesh(big, v, f)
    with pytest.raises(ValueError, match=r"more than 2\^27-16 rows"):
        pcu.closest_points_on_mesh(p, big, f)
    bigf = np.lib.stride_tricks.as_strided(np.zeros(3, dtype=np.int32), shape=(2 ** 27 - 15, 3), strides=(0, 4))
    with pytest.raises(ValueError, match=r"more than 2\^27-16 rows"):
        pcu.closest_points_on_mesh(p, v, bigf)


def test_mesh_index_validates_before_touching_the_gpu():
    import point_cloud_utils_amd as pcu
    p, v, f = _mesh()
    with pytest.raises(ValueError, match=r"Invalid scalar type \(int32\) for argument 'v'"):
        pcu.MeshIndex(v.astype(np.int32), f)
    with pytest.raises(ValueError, match="Invalid input mesh with zero elements"):
        pcu.MeshIndex(v, f[:0])
    with pytest.raises(ValueError, match="v must not contain NaN or infinite coordinates"):
        pcu.MeshIndex(np.where(np.arange(24).reshape(8, 3) == 4, np.nan, v).astype(np.float32), f)
    with pytest.raises(ValueError, match=r"found a face index outside \[0, 8\)"):
        pcu.MeshIndex(v, f + 6)
    assert "closest_points_on_mesh" in pcu.__all__ and "MeshIndex" in pcu.__all__


def test_no_cpu_fallback_without_gpu():
    import point_cloud_utils_amd as pcu
    from point_cloud_utils_amd import _lib
    if _lib.device_count() > 0:
        pytest.skip("GPU present")
    p, v, f = _mesh()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pcu.closest_points_on_mesh(p, v, f)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pcu.MeshIndex(v, f)


def test_new_entry_points_are_cancellable():
    from point_cloud_utils_amd import _lib
    L = _lib.lib()
    for suf in ("f32", "f64"):
        for op in ("closest_points_on_mesh", "mesh_index_create", "mesh_index_closest"):
            name = f"pcu_hip_{op}_{suf}"
            assert name in _lib._COMPUTE_ENTRY_POINTS and getattr(L, name).errcheck is _lib._after_call


# ---------------------------------------------------------------------------------------------------- disassembly
PROBE = """#include <hip/hip_runtime.h>
extern "C" __global__ void probe_div32(float* x) { x[0] = x[1] / x[2]; }
extern "C" __global__ void probe_div64(double* x) { x[0] = x[1] / x[2]; }
extern "C" __global__ void probe_sqrt32(float* x) { x[0] = sqrt(x[1]); }
extern "C" __global__ void probe_sqrt64(double* x) { x[0] = sqrt(x[1]); }
"""
MARKS = {"div32": r"\bv_div_fixup_f32", "div64": r"\bv_div_fixup_f64", "sqrt32": r"\bv_sqrt_f32", "sqrt64": r"\bv_rsq_f64"}


def _tally(lines):
    import test_disasm as td
    c = {k: 0 for k in MARKS}
    c.update(fma32=0, fma64=0, other=[])
    for ln in lines:
        ins = ln.split("//")[0].split(";")[0].strip()
        for k, pat in MARKS.items():
            if re.search(pat + td.SUF, ins):
                c[k] += 1
        m = td.FMA.search(ins)
        if m:
            if m.group(1) or m.group(4) == "16": c["other"].append(ins)
            elif m.group(4) == "32": c["fma32"] += 1
            else: c["fma64"] += 1
    return c


def test_mesh_kernels_fuse_only_inside_division_and_square_root(tmp_path):
    """Every k_mesh_* kernel: floating-point fused multiply-adds only as many as its correctly rounded divisions and square roots expand to.
    What one division / square root expands to is counted on a probe compiled with the library's own flags, not remembered."""
    import test_disasm as td
    import __graft_entry__ as g
    hipcc = os.environ.get("HIPCC", "hipcc")
    if not shutil.which(hipcc):
        pytest.skip("hipcc not in this image")
    cos = td._code_object(tmp_path)                        # (skips without the llvm tools or the library)
    src, asm = tmp_path / "probe.hip", tmp_path / "probe.s"
    src.write_text(PROBE)
    flags = [x for x in g.HIPCC_FLAGS if x not in ("-Xoffload-linker", "--discard-all", "-pthread", "-fPIC")]
    subprocess.run([hipcc] + flags + ["--cuda-device-only", "-S", "-o", str(asm), str(src)], check=True, capture_output=True)
    text = asm.read_text()
    per = {}
    for name in ("div32", "div64", "sqrt32", "sqrt64"):
        body = re.search(r"^probe_%s:.*?s_endpgm" % name, text, re.S | re.M).group(0).splitlines()
        c = _tally(body)
        assert c[name] == 1 and not c["other"], (name, c)
        per[name] = c["fma32"] if name.endswith("32") else c["fma64"]
        assert (c["fma64"] if name.endswith("32") else c["fma32"]) == 0
    print("fused multiply-adds per operation:", per)
    assert per["div32"] > 0 and per["div64"] > 0           # (the patterns match this ISA's expansions)
    seen = []
    for co in cos:
        syms = subprocess.run([f"{td.LLVM}/llvm-readelf", "-s", "--wide", co], capture_output=True, text=True, check=True).stdout
        names = sorted({ln.split()[-1] for ln in syms.splitlines() if " FUNC " in ln and "k_mesh_" in ln})
        for i in range(0, len(names), 8):
            out = subprocess.run([f"{td.LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--disassemble-symbols=" + ",".join(names[i:i + 8]), co],
                                 capture_output=True, text=True, check=True).stdout
            chunks = re.split(r"^[0-9a-f]+ <(\S+)>:\n", out, flags=re.M)
            for name, body in zip(chunks[1::2], chunks[2::2]):
                c = _tally(body.splitlines())
                assert not c["other"], (name, c["other"][:4])
                assert c["fma32"] == per["div32"] * c["div32"] + per["sqrt32"] * c["sqrt32"], (name, c)
                assert c["fma64"] == per["div64"] * c["div64"] + per["sqrt64"] * c["sqrt64"], (name, c)
                seen.append(name)
    assert len(seen) >= 20 and sum("k_mesh_closest" in n for n in seen) == 2, seen      # ten kernels x {f32, f64}
