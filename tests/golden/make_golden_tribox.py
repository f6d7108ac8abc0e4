"""Records the verdicts of the reference's triangle-box overlap test (src/common/tribox.h of the reference checkout) for two seeded families
of cases into tests/golden/voxelize/tribox_verdicts.npz (a directory of its own: the KNN tests take every .npz directly under
tests/golden/ for one of their cases). Run where the reference's checkout exists (never on the GPU machine):

    python tests/golden/make_golden_tribox.py [path to the reference checkout]

A few lines of C++ of this script's own include the reference's header by path and loop over the cases; they are compiled with
g++ -O2 -ffp-contract=off into a temporary directory. The fixture holds inputs and verdicts only: float32-representable coordinates (stored
as float32, evaluated in double) and one byte per case.
  lattice: triangle coordinates on multiples of 0.25 in [-1, 1], centres on multiples of 0.5 in [-1, 1], half size 0.25 -- 548 of the 4000 cases
           overlap, most of them by touching;
  random:  triangle coordinates and centres in [0, 1), half size (0.1, 0.07, 0.13) rounded to float32."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
N = 4000
SEED = 20240612

DRIVER = r"""
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include TRIBOX_HEADER
int main(int argc, char** argv) {
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    double rec[15];
    while (fread(rec, sizeof(double), 15, in) == 15) {
        double* tri[3] = {rec + 6, rec + 9, rec + 12};
        unsigned char verdict = (unsigned char)triBoxOverlap(rec, rec + 3, tri);
        fwrite(&verdict, 1, 1, out);
    }
    fclose(in); fclose(out);
    return 0;
}
"""


def cases():
    rng = np.random.default_rng(SEED)
    lat_tri = (rng.integers(-4, 5, (N, 9)) * 0.25).astype(np.float32)
    lat_centre = (rng.integers(-2, 3, (N, 3)) * 0.5).astype(np.float32)
    lat_half = np.full((N, 3), 0.25, dtype=np.float32)
    rnd_tri = rng.random((N, 9), dtype=np.float32)
    rnd_centre = rng.random((N, 3), dtype=np.float32)
    rnd_half = np.broadcast_to(np.array([0.1, 0.07, 0.13], dtype=np.float32), (N, 3)).copy()
    return {"lattice": (lat_centre, lat_half, lat_tri), "random": (rnd_centre, rnd_half, rnd_tri)}


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    header = os.path.join(ref, "src", "common", "tribox.h")
    if not os.path.exists(header):
        raise SystemExit(f"{header} not found: pass the path of the reference checkout")
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "driver.cpp"), os.path.join(tmp, "driver")
        open(src, "w").write(DRIVER)
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-w", f'-DTRIBOX_HEADER="{header}"', "-o", exe, src], check=True)
        for name, (centre, half, tri) in cases().items():
            rec = np.concatenate([centre, half, tri], axis=1).astype(np.float64)
            fin, fout = os.path.join(tmp, name + ".in"), os.path.join(tmp, name + ".out")
            rec.tofile(fin)
            subprocess.run([exe, fin, fout], check=True)
            verdict = np.fromfile(fout, dtype=np.uint8)
            assert verdict.shape == (N,) and set(np.unique(verdict)) <= {0, 1}
            out[name + "_centre"], out[name + "_half"], out[name + "_tri"], out[name + "_verdict"] = centre, half, tri, verdict
            print(name, "overlapping:", int(verdict.sum()), "of", N)
    os.makedirs(os.path.join(HERE, "voxelize"), exist_ok=True)
    np.savez_compressed(os.path.join(HERE, "voxelize", "tribox_verdicts.npz"), **out)


if __name__ == "__main__":
    main()
