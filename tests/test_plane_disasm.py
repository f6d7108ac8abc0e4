"""The no-FMA and no-scratch rules for the kernels of csrc/plane.h and their instantiations of csrc/consensus.h (the kernels over PlaneModel<T>,
and k_consensus_emit, which has no model), checked on the shipped binary with the method of tests/test_icp_disasm.py:
the hypotheses, the point-plane test, the terms and every level of the sum tree are separate multiplies and adds (a fused one would round
differently from tests/plane_contract.py), there is no square root in a kernel -- and no floating-point fused multiply-add hidden in an
integer remainder: the draws reduce their hashes in integers --, and none of these kernels uses scratch or spills a register. No GPU."""
import re
import subprocess

import test_disasm as td

MINE = re.compile(r"k_plane|PlaneModel|k_consensus_emit")       # (on mangled names)


def _plane_kernels(tmp_path):
    counts, notes = {}, ""
    for co in td._code_object(tmp_path):
        syms = subprocess.run([f"{td.LLVM}/llvm-readelf", "-s", "--wide", co], capture_output=True, text=True, check=True).stdout
        names = sorted({ln.split()[-1] for ln in syms.splitlines() if " FUNC " in ln and MINE.search(ln)})
        td._count_fma(co, names, counts)
        notes += subprocess.run([f"{td.LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
    return counts, notes


def test_plane_kernels_have_no_fused_multiply_add(tmp_path):
    counts, _ = _plane_kernels(tmp_path)
    for name in ("k_plane_hypotheses", "k_consensus_score", "k_consensus_best", "k_plane_sums", "k_consensus_mark"):
        assert len([k for k in counts if name in k]) == 2, (name, sorted(counts))      # float and double
    assert len([k for k in counts if "k_consensus_emit" in k]) == 1, sorted(counts)
    assert len(counts) == 11, sorted(counts)
    for k, c in counts.items():
        assert c == {"sqrt32": 0, "rsq64": 0, "fma32": 0, "fma64": 0, "other": []}, (k, c)


def test_plane_kernels_use_no_scratch(tmp_path):
    _, notes = _plane_kernels(tmp_path)
    seen = 0
    for blk in notes.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        if not MINE.search(name):
            continue
        seen += 1
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)) == 0, name
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)) == 0, name
        assert int(re.search(r"\.sgpr_spill_count:\s+(\d+)", blk).group(1)) == 0, name
    assert seen == 11
