"""Register budget of the k = 1 lane pass, checked on the shipped binary (CPU test). The fused float instantiations of k_search1_flat
(Chamfer sum, FUSE_SUM = 1, the headline; Hausdorff value-only, FUSE_MAXVAL = 3) are launched with 8 waves per SIMD, i.e. at most 64
VGPRs per lane, and must get there without private (scratch) memory: a spill costs the texture-address path -- the kernel's tightest
resource -- a vector-memory instruction per store and per reload, and writes ~28 bytes per lane to HBM (search.h: search1_flat_body).
No instantiation of the kernel may use scratch."""
import re
import subprocess

from test_disasm import LLVM, _code_object

FLAT = "_ZN3pcu14k_search1_flatI"
FUSED_F32 = ["_ZN3pcu14k_search1_flatIfLb0ELi8ELi1EEEvNS_11SearchArgs2IT_EEi",     # <float, false, 8, FUSE_SUM>
             "_ZN3pcu14k_search1_flatIfLb0ELi8ELi3EEEvNS_11SearchArgs2IT_EEi"]     # <float, false, 8, FUSE_MAXVAL>
# every instantiation the host launches (pcu_hip.hip: launch_search_fast): float and double, rows / fused sum / value-only arg-max
LAUNCHED = FUSED_F32 + ["_ZN3pcu14k_search1_flatIfLb0ELi4ELi0EEEvNS_11SearchArgs2IT_EEi",     # <float, false, 4, FUSE_NONE>
                        "_ZN3pcu14k_search1_flatIdLb0ELi4ELi0EEEvNS_11SearchArgs2IT_EEi",     # <double, false, 4, FUSE_NONE>
                        "_ZN3pcu14k_search1_flatIdLb0ELi4ELi1EEEvNS_11SearchArgs2IT_EEi",     # <double, false, 4, FUSE_SUM>
                        "_ZN3pcu14k_search1_flatIdLb0ELi4ELi3EEEvNS_11SearchArgs2IT_EEi"]     # <double, false, 4, FUSE_MAXVAL>


def _kernel_resources(tmp_path):
    res = {}
    for co in _code_object(tmp_path):
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
        for blk in notes.split("- .agpr_count:")[1:]:
            field = lambda k: re.search(r"^\s+\." + k + r":\s+(\S+)", blk, re.M).group(1)
            res[field("name")] = {"agpr": int(blk.split()[0]), "vgpr": int(field("vgpr_count")), "scratch": int(field("private_segment_fixed_size")),
                                  "vgpr_spill": int(field("vgpr_spill_count"))}
    return res


def test_fused_k1_float_kernels_fit_eight_waves_without_scratch(tmp_path):
    res = _kernel_resources(tmp_path)
    for name in FUSED_F32:
        assert name in res, sorted(n for n in res if n.startswith(FLAT))
        r = res[name]
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (name, r)
        assert r["agpr"] == 0 and r["vgpr"] <= 64, (name, r)


def test_every_launched_k1_lane_pass_is_built_without_scratch(tmp_path):
    res = _kernel_resources(tmp_path)
    flat = {n: r for n, r in res.items() if n.startswith(FLAT)}
    for name in LAUNCHED:
        assert name in flat, (name, sorted(flat))
    for name, r in flat.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (name, r)
