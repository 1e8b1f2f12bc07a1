// hispmv_block_jacobi_device.h -- the block-Jacobi multiply of a thread: ONE text for the apply kernel of hispmv_block_jacobi.hip and for
// the CG and GMRES kernels that form z = M^-1 r where their inverse-diagonal variants form d[j] * r[j] (hispmv_krylov.hip,
// hispmv_gmres.hip).  It rides on the chunk walk of hispmv_krylov_device.h: a thread owns the 4 consecutive rows i .. i + 3 of a chunk
// (i a multiple of 4), and for_chunks calls its body on all 256 threads, so every lane takes part in the cross-lane reads.
//   z_i = ((+0 + B[i][0] r_0) + B[i][1] r_1) + ... + B[i][bs-1] r_{bs-1}: fp32, every product rounded, then added, k ascending
// over the columns of row i's block; r at or beyond n counts as +0.  BS = 4: the block is the thread's own.  BS = 8 / 16 / 32: the
// 2 / 4 / 8 neighbouring lanes of the wavefront own it and hand each other their 4 values of r (ds_bpermute: no LDS memory, no
// barrier).  A thread reads its 4 rows of the block as 16-byte loads, a 4-column piece at a time.  Included by those three kernel files
// only, which compile with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace hispmv {
namespace {

// z[0 .. 4) = rows i .. i + 3 of M^-1 r; r[0 .. 4) = the thread's own elements of r, of which m lie below n.  blocks: the block area
// of the buffer (hispmv_block_jacobi.h), 16-byte aligned.  A thread with m == 0 loads nothing and returns zeros; rows of the padded
// last block at or beyond n are computed (their block rows exist) and not stored by the caller's st4.
template <int BS>
__device__ __forceinline__ void block_jacobi_mul4(const float* blocks, int64_t i, int m, const float r[4], float z[4]) {
    static_assert(BS == 4 || BS == 8 || BS == 16 || BS == 32, "block sizes 4, 8, 16, 32");
    constexpr int L = BS / 4;                                   // lanes of a block
    float mine[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        mine[e] = e < m ? r[e] : 0.0f;
        z[e] = 0.0f;
    }
    const int q = (int)(threadIdx.x & (L - 1));                 // the thread's 4 rows are rows 4 q .. 4 q + 3 of the block
    const float* const rows = blocks + (i / BS) * (int64_t)(BS * BS) + (int64_t)(4 * q) * BS;
#pragma unroll
    for (int t = 0; t < L; ++t) {
        float rt[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) rt[e] = L == 1 ? mine[e] : __shfl(mine[e], t, L);
        if (m > 0) {
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const float4 b = *reinterpret_cast<const float4*>(rows + a * BS + 4 * t);
                float p = b.x * rt[0];
                z[a] = z[a] + p;
                p = b.y * rt[1];
                z[a] = z[a] + p;
                p = b.z * rt[2];
                z[a] = z[a] + p;
                p = b.w * rt[3];
                z[a] = z[a] + p;
            }
        }
    }
}

}  // namespace
}  // namespace hispmv
