"""The no-FMA and no-scratch rules for the kernels of csrc/icp.h, checked on the shipped binary with the method of tests/test_dbscan_disasm.py:
the transform, the terms and every level of the sum tree are separate multiplies and adds (a fused one would round differently from
tests/icp_contract.py), there is no square root in a kernel, and no k_icp kernel uses scratch or spills a register. No GPU."""
import re
import subprocess

import test_disasm as td


def _icp_kernels(tmp_path):
    counts, notes = {}, ""
    for co in td._code_object(tmp_path):
        syms = subprocess.run([f"{td.LLVM}/llvm-readelf", "-s", "--wide", co], capture_output=True, text=True, check=True).stdout
        names = sorted({ln.split()[-1] for ln in syms.splitlines() if " FUNC " in ln and "k_icp" in ln})
        td._count_fma(co, names, counts)
        notes += subprocess.run([f"{td.LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
    return counts, notes


def test_icp_kernels_have_no_fused_multiply_add(tmp_path):
    counts, _ = _icp_kernels(tmp_path)
    assert len([k for k in counts if "k_icp_sums" in k]) == 4, sorted(counts)          # float and double; point and plane mode
    assert len([k for k in counts if "k_icp_transform" in k]) == 2, sorted(counts)
    assert len([k for k in counts if "k_icp_fold" in k]) == 1, sorted(counts)
    assert len(counts) == 7, sorted(counts)
    for k, c in counts.items():
        assert c == {"sqrt32": 0, "rsq64": 0, "fma32": 0, "fma64": 0, "other": []}, (k, c)


def test_icp_kernels_use_no_scratch(tmp_path):
    _, notes = _icp_kernels(tmp_path)
    seen = 0
    for blk in notes.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        if "k_icp" not in name:
            continue
        seen += 1
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)) == 0, name
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)) == 0, name
        assert int(re.search(r"\.sgpr_spill_count:\s+(\d+)", blk).group(1)) == 0, name
    assert seen == 7
