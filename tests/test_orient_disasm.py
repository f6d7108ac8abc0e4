"""The no-FMA and no-scratch rules for the kernels of csrc/orient.h, checked on the shipped binary with the method of tests/test_plane_disasm.py:
the agreement of two normals is separate multiplies and adds (a fused one would round differently from tests/orient_contract.py), the row of
a slot is found without the compiler's floating-point division, and no k_orient kernel uses scratch or spills a register. No GPU."""
import re
import subprocess

import test_disasm as td


def _orient_kernels(tmp_path):
    counts, notes = {}, ""
    for co in td._code_object(tmp_path):
        syms = subprocess.run([f"{td.LLVM}/llvm-readelf", "-s", "--wide", co], capture_output=True, text=True, check=True).stdout
        names = sorted({ln.split()[-1] for ln in syms.splitlines() if " FUNC " in ln and "k_orient" in ln})
        td._count_fma(co, names, counts)
        notes += subprocess.run([f"{td.LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
    return counts, notes


def test_orient_kernels_have_no_fused_multiply_add(tmp_path):
    counts, _ = _orient_kernels(tmp_path)
    for name, copies in (("k_orient_init", 1), ("k_orient_hook", 1), ("k_orient_flatten", 2), ("k_orient_offer", 4), ("k_orient_write", 2)):
        assert len([k for k in counts if name in k]) == copies, (name, sorted(counts))
    assert len(counts) == 10, sorted(counts)
    for k, c in counts.items():
        assert c == {"sqrt32": 0, "rsq64": 0, "fma32": 0, "fma64": 0, "other": []}, (k, c)


def test_orient_kernels_use_no_scratch(tmp_path):
    _, notes = _orient_kernels(tmp_path)
    seen = 0
    for blk in notes.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        if "k_orient" not in name:
            continue
        seen += 1
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)) == 0, name
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)) == 0, name
        assert int(re.search(r"\.sgpr_spill_count:\s+(\d+)", blk).group(1)) == 0, name
    assert seen == 10
