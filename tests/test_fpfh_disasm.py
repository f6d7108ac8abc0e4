"""The no-FMA and no-scratch rules for the kernels of csrc/fpfh.h and csrc/feature_match.h, checked on the shipped binary with the method of
tests/test_orient_disasm.py. The pair features and the squared feature distances are separate multiplies and adds (a fused one would round
differently from tests/fpfh_contract.py and tests/feature_match_contract.py). The contract's float64 divisions and square roots are IEEE
ones, which the compiler expands into a reciprocal (or reciprocal square root) estimate and fused fix-up steps: those, and only those, are
accounted for by count -- 7 per v_rsq_f64 as tests/test_disasm.py states it, 5 per v_div_fixup_f64 (hipcc 7.2 on gfx950: v_div_scale x 2,
v_rcp, 3 v_fma + 2 v_fmac, v_div_fmas, v_div_fixup). No k_fpfh or k_feature_match kernel uses scratch or spills a register. No GPU."""
import re
import subprocess

import test_disasm as td

PER_DIV_F64 = 5
EXPECTED = (("k_fpfh_normals", 2), ("k_fpfh_walk1", 2), ("k_fpfh_walk2", 2), ("k_feature_match_fold", 2), ("k_feature_match_mutual", 1),
            ("k_feature_matchI", 4))          # (the search itself: float and double, D = 33 and any D)
PATTERN = r"k_fpfh|k_feature_match"


def _kernels(tmp_path):
    counts, divs, notes = {}, {}, ""
    for co in td._code_object(tmp_path):
        syms = subprocess.run([f"{td.LLVM}/llvm-readelf", "-s", "--wide", co], capture_output=True, text=True, check=True).stdout
        names = sorted({ln.split()[-1] for ln in syms.splitlines() if " FUNC " in ln and re.search(PATTERN, ln)})
        td._count_fma(co, names, counts)
        for name in names:
            out = subprocess.run([f"{td.LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--disassemble-symbols=" + name, co],
                                 capture_output=True, text=True, check=True).stdout
            divs[name] = len(re.findall(r"\bv_div_fixup_f64" + td.SUF, out))
        notes += subprocess.run([f"{td.LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
    return counts, divs, notes


def test_fpfh_and_feature_match_kernels_have_no_fused_multiply_add(tmp_path):
    counts, divs, _ = _kernels(tmp_path)
    for name, copies in EXPECTED:
        assert len([k for k in counts if name in k]) == copies, (name, sorted(counts))
    assert len(counts) == sum(c for _, c in EXPECTED) == 13, sorted(counts)
    for k, c in counts.items():
        assert c["sqrt32"] == 0 and c["fma32"] == 0 and not c["other"], (k, c)
        assert c["fma64"] == td.PER_RSQ_F64 * c["rsq64"] + PER_DIV_F64 * divs[k], (k, c, divs[k])
        if "k_fpfh_walk" not in k:
            assert c["fma64"] == 0, (k, c)          # the dense search, its fold and the gather of the normals divide nothing
    assert sum(divs.values()) > 0 and sum(c["rsq64"] for c in counts.values()) > 0          # the guard sees the expansions it accounts for


def test_fpfh_and_feature_match_kernels_use_no_scratch(tmp_path):
    _, _, notes = _kernels(tmp_path)
    seen = 0
    for blk in notes.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        if not re.search(PATTERN, name):
            continue
        seen += 1
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)) == 0, name
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)) == 0, name
        assert int(re.search(r"\.sgpr_spill_count:\s+(\d+)", blk).group(1)) == 0, name
    assert seen == 13
