"""The index build's bulk output leaves the CU with 16-byte write-through stores (pcu_types.h: store16_wt), checked on the shipped binary
(CPU test, as test_disasm.py: the gfx950 code objects inside libpcu_hip.so are extracted and the two build kernels disassembled):

  * in k_bucket_onepass3<float, 8> and k_bucket_sort2<float> every store that carries the write-through bit (`sc1`) is 16 bytes wide -- a
    narrower write-through store is one fabric write each and costs 2.7x - 12x the time per byte;
  * the scatter's run copies and the sort's two stream copy-outs (coordinates, row ids) do carry the bit;
  * no source file of the package uses an instruction of the scalar-store family (scalar stores, scalar atomics, scalar data-cache write-back
    or discard): values are written with vector stores or plain C++.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "point_cloud_utils_amd")
LIB = os.path.join(PKG, "libpcu_hip.so")
LLVM = "/opt/rocm/lib/llvm/bin"
STORE = re.compile(r"^(global|flat|buffer|scratch)_store_(\w+)")
KERNELS = {"scatter": re.compile(r"k_bucket_onepass3IfLi8E"), "sort": re.compile(r"k_bucket_sort2IfE")}


def _code_objects(tmp_path):
    for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-objdump", "llvm-readelf"):
        if not os.path.exists(os.path.join(LLVM, t)):
            pytest.skip(f"{t} not in this image")
    if not os.path.exists(LIB):
        pytest.skip("libpcu_hip.so not built")
    fat = str(tmp_path / "fat.bin")
    subprocess.run([f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", LIB, fat], check=True)
    blob, magic = open(fat, "rb").read(), b"__CLANG_OFFLOAD_BUNDLE__"
    starts = [m.start() for m in re.finditer(re.escape(magic), blob)]
    assert starts, "no offload bundle in .hip_fatbin"
    cos = []
    for i, a in enumerate(starts):
        part, co = str(tmp_path / f"fat{i}.bin"), str(tmp_path / f"co{i}.gfx950")
        open(part, "wb").write(blob[a:starts[i + 1] if i + 1 < len(starts) else len(blob)])
        subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={part}",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True)
        cos.append(co)
    return cos


def _stores(tmp_path):
    """kernel tag -> [(width suffix, has the write-through bit)] of every vector-memory store of the kernel."""
    found = {}
    for co in _code_objects(tmp_path):
        syms = subprocess.run([f"{LLVM}/llvm-readelf", "-s", "--wide", co], capture_output=True, text=True, check=True).stdout
        for tag, pat in KERNELS.items():
            names = sorted({ln.split()[-1] for ln in syms.splitlines() if " FUNC " in ln and pat.search(ln)})
            if not names:
                continue
            assert len(names) == 1, names
            out = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--disassemble-symbols=" + names[0], co],
                                 capture_output=True, text=True, check=True).stdout
            rows = []
            for ln in out.splitlines():
                ins = ln.split("//")[0].strip()
                m = STORE.match(ins)
                if m:
                    rows.append((m.group(2), re.search(r"\bsc1\b", ins) is not None))
            assert tag not in found, tag
            found[tag] = rows
    assert sorted(found) == sorted(KERNELS), sorted(found)
    return found


def test_write_through_stores_are_16_bytes_wide(tmp_path):
    for tag, rows in _stores(tmp_path).items():
        assert rows, tag
        narrow = [w for w, wt in rows if wt and w != "dwordx4"]
        assert not narrow, (tag, narrow)


def test_bulk_copies_are_write_through(tmp_path):
    st = _stores(tmp_path)
    wt = {tag: sum(1 for w, t in rows if t and w == "dwordx4") for tag, rows in st.items()}
    assert wt["scatter"] >= 1, wt          # the run copies (one store per float record)
    assert wt["sort"] >= 2, wt             # the coordinate chunks and the row-id chunks of the FAST path


def test_sources_use_no_scalar_store_family():
    # (the mnemonics are put together here so that this file does not spell them either)
    s = "s"
    fam = ["_".join((s, "store")), "_".join((s, "buffer", "store")), "_".join((s, "scratch", "store")), "_".join((s, "atomic")),
           "_".join((s, "buffer", "atomic")), "_".join((s, "dcache", "wb")), "_".join((s, "dcache", "discard"))]
    pat = re.compile(r"(?<![A-Za-z0-9_])(" + "|".join(fam) + ")", re.IGNORECASE)
    hits = []
    for d, _, files in os.walk(PKG):
        if "_build" in d or "__pycache__" in d:
            continue
        for f in files:
            if f.endswith((".h", ".hip", ".cpp", ".c", ".inc", ".py", ".s", ".S")):
                p = os.path.join(d, f)
                for i, ln in enumerate(open(p, errors="replace"), 1):
                    if pat.search(ln):
                        hits.append(f"{os.path.relpath(p, ROOT)}:{i}")
    assert not hits, hits
