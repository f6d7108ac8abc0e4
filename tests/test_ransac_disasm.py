"""The no-FMA and no-scratch rules for the kernels of csrc/ransac.h and their instantiations of csrc/consensus.h (the kernels over RansacModel),
checked on the shipped binary with the method of tests/test_fpfh_disasm.py and tests/test_plane_disasm.py: the pre-check, the motion of a hypothesis, the test of a correspondence, the terms and every level of the sum
tree are separate multiplies and adds (a fused one would round differently from tests/ransac_contract.py). The contract's float64 divisions and
square roots are IEEE ones, which the compiler expands into a reciprocal (or reciprocal square root) estimate and fused fix-up steps: those are
accounted for by count, and k_ransac_hypotheses alone has any. None of these kernels uses scratch or spills a register. No GPU."""
import re
import subprocess

import test_disasm as td
from test_fpfh_disasm import PER_DIV_F64

EXPECTED = (("k_ransac_gather", 2), ("k_ransac_hypotheses", 1), ("k_ransac_score", 1), ("k_consensus_best", 1), ("k_ransac_sums", 2), ("k_consensus_mark", 1))
MINE = re.compile(r"k_ransac|RansacModel")                     # (on mangled names)
TOTAL = 8


def _kernels(tmp_path):
    counts, divs, notes = {}, {}, ""
    for co in td._code_object(tmp_path):
        syms = subprocess.run([f"{td.LLVM}/llvm-readelf", "-s", "--wide", co], capture_output=True, text=True, check=True).stdout
        names = sorted({ln.split()[-1] for ln in syms.splitlines() if " FUNC " in ln and MINE.search(ln)})
        td._count_fma(co, names, counts)
        for name in names:
            out = subprocess.run([f"{td.LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--disassemble-symbols=" + name, co],
                                 capture_output=True, text=True, check=True).stdout
            divs[name] = len(re.findall(r"\bv_div_fixup_f64" + td.SUF, out))
        notes += subprocess.run([f"{td.LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
    return counts, divs, notes


def test_the_ransac_kernels_are_the_expected_ones_without_fused_multiply_add(tmp_path):
    counts, divs, _ = _kernels(tmp_path)
    for name, copies in EXPECTED:
        assert len([k for k in counts if name in k]) == copies, (name, sorted(counts))
    assert len(counts) == sum(c for _, c in EXPECTED) == TOTAL, sorted(counts)
    assert len([k for k in counts if "k_ransac_sumsILi17E" in k]) == 1 and len([k for k in counts if "k_ransac_sumsILi2E" in k]) == 1, sorted(counts)
    for k, c in counts.items():
        assert c["sqrt32"] == 0 and c["fma32"] == 0 and not c["other"], (k, c)
        if "k_ransac_hypotheses" in k:
            # four square roots (two lengths per frame) and 24 divisions (two unit vectors per frame, two centroids), however the compiler shares them
            assert 1 <= c["rsq64"] <= 4 and 1 <= divs[k] <= 24, (k, c, divs[k])
            assert c["fma64"] == td.PER_RSQ_F64 * c["rsq64"] + PER_DIV_F64 * divs[k], (k, c, divs[k])
        else:
            assert c["fma64"] == 0 and c["rsq64"] == 0 and divs[k] == 0, (k, c, divs[k])       # (the sums divide nothing: the solve is the host's)


def test_ransac_kernels_use_no_scratch(tmp_path):
    _, _, notes = _kernels(tmp_path)
    seen = 0
    for blk in notes.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        if not MINE.search(name):
            continue
        seen += 1
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)) == 0, name
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)) == 0, name
        assert int(re.search(r"\.sgpr_spill_count:\s+(\d+)", blk).group(1)) == 0, name
    assert seen == TOTAL
