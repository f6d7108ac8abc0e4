"""Generator of csrc/mc_table.h, the case table of marching_cubes_sparse_voxel_grid. The table is derived from a rule,
not copied from a published one:

  * corners 0:(0,0,0) 1:(1,0,0) 2:(1,1,0) 3:(0,1,0) 4:(0,0,1) 5:(1,0,1) 6:(1,1,1) 7:(0,1,1); edges 0:0-1 1:1-2 2:2-3 3:3-0 4:4-5 5:5-6
    6:6-7 7:7-4 8:0-4 9:1-5 10:2-6 11:3-7; a case is the 8-bit mask of the corners that are inside (scalar > isovalue);
  * the six faces are corner cycles, each counter-clockwise seen from outside the cube. On a face, every maximal run of inside corners along
    the cycle is cut off by one directed segment, from the cube edge where the walk along the cycle leaves the run to the cube edge where it
    enters the run. Only the face's own four signs are read, so the two cubes that share a face draw the same segments: no cracks;
  * every crossed edge then has exactly one successor; the loops are followed from their lowest-numbered edge, in ascending order of it;
  * a loop e0, e1, ... is triangulated as the fan (e0, ei, ei+1).

Run `python gen_mc_table.py` to rewrite mc_table.h next to this file; tests/test_marching_cubes_contract.py holds the file to this output."""
import hashlib
import os

EDGES = [(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7)]
FACES = [[3, 0, 4, 7], [5, 1, 2, 6], [4, 0, 1, 5], [6, 2, 3, 7], [1, 0, 3, 2], [7, 4, 5, 6]]
SHA256 = "adcb2239f3f3693051b66260acad88e37eb439a287ca3cb5fd65b810e8775999"

_EDGE_OF = {frozenset(e): i for i, e in enumerate(EDGES)}


def case_triangles(mask):
    """The triangles of one case: a list of edge triples."""
    inside = [(mask >> c) & 1 for c in range(8)]
    succ = {}
    for cyc in FACES:
        for k in range(4):
            a, b = cyc[k], cyc[(k + 1) % 4]
            if not (inside[a] and not inside[b]):
                continue                                  # the walk leaves a run between a and b ...
            j = k
            while inside[cyc[(j - 1) % 4]]:               # ... which began where the walk entered it
                j -= 1
            leave, enter = _EDGE_OF[frozenset((a, b))], _EDGE_OF[frozenset((cyc[(j - 1) % 4], cyc[j % 4]))]
            assert leave not in succ
            succ[leave] = enter
    tris, seen = [], set()
    for e0 in sorted(succ):
        if e0 in seen:
            continue
        loop, e = [], e0
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = succ[e]
        assert e == e0 and len(loop) >= 3
        tris += [(loop[0], loop[i], loop[i + 1]) for i in range(1, len(loop) - 1)]
    return tris


def table():
    """256 rows of 16 int8 values: edge triples, -1 padded."""
    rows = []
    for mask in range(256):
        flat = [e for t in case_triangles(mask) for e in t]
        assert len(flat) <= 15
        rows.append(flat + [-1] * (16 - len(flat)))
    return rows


def table_bytes(rows=None):
    return bytes((x + 256) % 256 for r in (rows or table()) for x in r)


def header_text():
    rows = table()
    assert hashlib.sha256(table_bytes(rows)).hexdigest() == SHA256
    out = ["// csrc/mc_table.h -- the case table of marching cubes (marching_cubes.h). Written by gen_mc_table.py from the rule stated there: do not edit.",
           "// Row = the 8-bit mask of the corners with scalar > isovalue; up to five triangles as triples of cube edges, -1 padded.",
           "// sha256 of the 4096 bytes: " + SHA256,
           "#pragma once",
           "",
           "namespace pcu {",
           "",
           "static __device__ const signed char kMcTable[256][16] __attribute__((aligned(16))) = {"]
    for mask, r in enumerate(rows):
        out.append("    {" + ", ".join("%2d" % x for x in r) + "},  // 0x%02X" % mask)
    out += ["};", "", "}  // namespace pcu", ""]
    return "\n".join(out)


if __name__ == "__main__":
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "mc_table.h"), "w") as fh:
        fh.write(header_text())
