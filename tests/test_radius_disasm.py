"""The no-FMA and no-scratch rules for the kernels of csrc/radius.h, checked on the shipped binary with the method of tests/test_disasm.py
(whose list of kernels is the search kernels'): the walk that evaluates d2 = ((dx*dx) + (dy*dy)) + (dz*dz) holds no fused multiply-add at
all, and in the other kernels the only ones are the expansion of the correctly rounded sqrt. No GPU."""
import re
import subprocess

import test_disasm as td


def _radius_kernels(tmp_path):
    counts, notes = {}, ""
    for co in td._code_object(tmp_path):
        syms = subprocess.run([f"{td.LLVM}/llvm-readelf", "-s", "--wide", co], capture_output=True, text=True, check=True).stdout
        names = sorted({ln.split()[-1] for ln in syms.splitlines() if " FUNC " in ln and "k_radius" in ln})
        td._count_fma(co, names, counts)
        notes += subprocess.run([f"{td.LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
    return counts, notes


def test_radius_kernels_have_no_fused_multiply_add(tmp_path):
    counts, _ = _radius_kernels(tmp_path)
    walks = [k for k in counts if "k_radius_walk" in k]
    assert len(walks) == 4, walks                                          # float and double, count and fill
    for k in walks:
        assert counts[k] == {"sqrt32": 0, "rsq64": 0, "fma32": 0, "fma64": 0, "other": []}, (k, counts[k])
    assert len(counts) >= 16, sorted(counts)
    for k, c in counts.items():
        assert not c["other"], (k, c["other"][:4])
        assert c["fma32"] == td.PER_SQRT_F32 * c["sqrt32"] and c["fma64"] == td.PER_RSQ_F64 * c["rsq64"], (k, c)
    outs = [c for k, c in counts.items() if "k_radius_out" in k]
    assert sum(c["sqrt32"] + c["rsq64"] for c in outs) == 2                 # the patterns match this ISA: the two square roots are seen


def test_radius_kernels_use_no_scratch(tmp_path):
    _, notes = _radius_kernels(tmp_path)
    seen = 0
    for blk in notes.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        if "k_radius" not in name:
            continue
        seen += 1
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)) == 0, name
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)) == 0, name
    assert seen >= 16
