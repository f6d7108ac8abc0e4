"""The no-FMA and no-scratch rules for the kernels of csrc/dbscan.h, checked on the shipped binary with the method of tests/test_disasm.py and
tests/test_radius_disasm.py: the three passes of the walk evaluate d2 = ((dx*dx) + (dy*dy)) + (dz*dz) and hold no fused multiply-add (and no
square root) at all; no k_dbscan kernel uses scratch or spills a register. No GPU."""
import re
import subprocess

import test_disasm as td


def _dbscan_kernels(tmp_path):
    counts, notes = {}, ""
    for co in td._code_object(tmp_path):
        syms = subprocess.run([f"{td.LLVM}/llvm-readelf", "-s", "--wide", co], capture_output=True, text=True, check=True).stdout
        names = sorted({ln.split()[-1] for ln in syms.splitlines() if " FUNC " in ln and "k_dbscan" in ln})
        td._count_fma(co, names, counts)
        notes += subprocess.run([f"{td.LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
    return counts, notes


def test_dbscan_kernels_have_no_fused_multiply_add(tmp_path):
    counts, _ = _dbscan_kernels(tmp_path)
    walks = [k for k in counts if "k_dbscan_walk" in k]
    assert len(walks) == 6, walks                                          # float and double; core, union and border pass
    assert len(counts) == 7, sorted(counts)                                # ... and k_dbscan_roots
    for k, c in counts.items():
        assert c == {"sqrt32": 0, "rsq64": 0, "fma32": 0, "fma64": 0, "other": []}, (k, c)


def test_dbscan_kernels_use_no_scratch(tmp_path):
    _, notes = _dbscan_kernels(tmp_path)
    seen = 0
    for blk in notes.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        if "k_dbscan" not in name:
            continue
        seen += 1
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)) == 0, name
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)) == 0, name
        assert int(re.search(r"\.sgpr_spill_count:\s+(\d+)", blk).group(1)) == 0, name
    assert seen == 7
