"""The farthest-point kernels on the shipped binary (CPU test): no fused multiply-add anywhere in them beyond the expansion of the correctly
rounded sqrt of their output -- the distance AND the box bound are the contract's separate multiplies and adds, or the pruning would not be
exact --, and none uses private (scratch) memory or spills a register: the one-block kernel keeps its whole cloud in registers by design."""
import re
import subprocess

from test_disasm import LLVM, PER_RSQ_F64, PER_SQRT_F32, _code_object, _count_fma
from test_kernel_resources import _kernel_resources

import point_cloud_utils_amd as pcu

assert callable(pcu.downsample_point_cloud_farthest_point)
KERNELS = ["k_fps_block", "k_fps_iter", "k_fps_init", "k_fps_setup"]


def test_fps_kernels_have_no_fused_multiply_add(tmp_path):
    counts = {}
    for co in _code_object(tmp_path):
        syms = subprocess.run([f"{LLVM}/llvm-readelf", "-s", "--wide", co], capture_output=True, text=True, check=True).stdout
        names = sorted({ln.split()[-1] for ln in syms.splitlines() if " FUNC " in ln and re.search(r"k_fps_", ln)})
        _count_fma(co, names, counts)
    for k in KERNELS:
        assert sum(k in n for n in counts) == 2, (k, sorted(counts))              # float and double
    assert len(counts) == 2 * len(KERNELS), sorted(counts)
    sqrts = 0
    for k, c in counts.items():
        assert not c["other"], (k, c["other"][:4])
        assert c["fma32"] == PER_SQRT_F32 * c["sqrt32"], (k, c)
        assert c["fma64"] == PER_RSQ_F64 * c["rsq64"], (k, c)
        sqrts += c["sqrt32"] + c["rsq64"]
    assert sqrts >= 4                                                             # both output sites, both types: the patterns match this ISA


def test_fps_kernels_use_no_scratch(tmp_path):
    res = {n: r for n, r in _kernel_resources(tmp_path).items() if "k_fps_" in n}
    assert len(res) == 2 * len(KERNELS), sorted(res)
    for name, r in res.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (name, r)
        if "k_fps_block" in name:
            assert r["vgpr"] + r["agpr"] <= 128, (name, r)                        # 1024 threads: four waves per SIMD share its 512 registers
