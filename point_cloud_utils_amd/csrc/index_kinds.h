// csrc/index_kinds.h -- integer arrays "of kind 0..3" on the device (kind 0 int32, 1 int64, 2 uint32, 3 uint64: faces, cube corners, voxel
// coordinates, and every integer output that takes its input's type). Included by pcu_types.h. The one place where a kind is told apart, and
// the one statement of the three rules:
//   reading    a value comes in as 64 unsigned bits, a signed one sign-extended first: a negative index is a huge unsigned one;
//   checking   every range check is made on those 64 bits, before any narrowing to int: no uint64 value is truncated, or read as signed, into range;
//   writing    an unsigned value is zero-extended (index_out), a signed one -- the -1 of "no such row" -- sign-extended (index_out_signed).
#pragma once
#include <hip/hip_runtime.h>

namespace pcu {

// The two shared bits of every operator's flag word (pcu_hip.hip: mesh_refusal); an operator's own bits lie above them.
constexpr int kMeshBadVertex = 1, kMeshBadFace = 2;

__device__ __forceinline__ unsigned long long index_in(const void* __restrict__ p, int kind, size_t at) {
    if (kind == 0) return (unsigned long long)(long long)static_cast<const int*>(p)[at];
    if (kind == 1) return (unsigned long long)static_cast<const long long*>(p)[at];
    if (kind == 2) return (unsigned long long)static_cast<const unsigned*>(p)[at];
    return static_cast<const unsigned long long*>(p)[at];
}
__device__ __forceinline__ bool index_kind_signed(int kind) { return kind < 2; }
__device__ __forceinline__ bool index_kind_wide(int kind) { return (kind & 1) != 0; }
__device__ __forceinline__ void index_out(void* __restrict__ p, int kind, size_t at, unsigned x) {
    if (index_kind_wide(kind)) static_cast<unsigned long long*>(p)[at] = x;
    else static_cast<unsigned*>(p)[at] = x;
}
__device__ __forceinline__ void index_out_signed(void* __restrict__ p, int kind, size_t at, int x) {
    if (index_kind_wide(kind)) static_cast<long long*>(p)[at] = (long long)x;
    else static_cast<int*>(p)[at] = x;
}
// Face i of f (nf, 3): true ("bad") if one of its indices lies outside [0, nv); id holds the three indices, (0, 0, 0) for a bad face.
__device__ __forceinline__ bool face_in(const void* __restrict__ f, int kind, size_t i, unsigned nv, int (&id)[3]) {
    bool bad = false;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const unsigned long long u = index_in(f, kind, 3 * i + j);
        bad |= u >= (unsigned long long)nv;
        id[j] = (int)u;
    }
    if (bad) id[0] = id[1] = id[2] = 0;
    return bad;
}

}  // namespace pcu
