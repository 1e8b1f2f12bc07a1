// hispmv_spmm_bf16.h -- the wide-batch product with bf16 activations (hispmv_spmm_bf16.hip; include/hispmv.h: hispmv_spmm_device_bf16):
//   yt[r, v] = bf16(alpha * sum_k a_rk * xt[k, v] + beta * bias),      xt = [cols, ld_x], yt = [rows, ld_y], row-major, bf16
// hispmv_spmm.h with 2-byte operands.  Grid, groups, walk, the fp32 accumulators, the +-0 rule, the fp32 workspace of the cut rows and
// the fix-up launch are those of the fp32 entry; a lane owns VB = 8, 4, 2 or 1 consecutive vectors (one dwordx4, dwordx2, dword or
// 16-bit load per stored element), so a tile is 64 * VB vectors.  The value before the one rounding is, bit for bit, what
// hispmv_spmm_device computes on the widened operands.
#pragma once
#include "hispmv_spmm.h"

namespace hispmv {

// The tile rule (host-only; hispmv_prep_spmm_bf16_tiles): the largest VB in {8, 4, 2, 1} for a tile that begins with `left` vectors to go with
//   (a) 64 * (VB / 2) < left                         -- do not widen past the batch
//   (b) cols * 64 * VB * 2 <= kSpmmTileBytes         -- the fp32 rule's 8 MiB REUSED UNMEASURED: it was measured with 4-byte activations
//                                                       (VL 4 up to 8192 columns) and is taken over as the same cap in bytes: VB 8 up to 8192
//   (c) every ld % VB == 0 and align_bytes % (2 * VB) == 0      -- a lane's VB halves are one aligned load in every row
inline int spmm_bf16_vb(int64_t cols, int64_t left, int64_t ld_x, int64_t ld_y, int64_t align_bytes) {
    for (int vb = 8; vb >= 2; vb >>= 1)
        if (64 * (vb / 2) < left && cols * 64 * vb * 2 <= kSpmmTileBytes && ld_x % vb == 0 && ld_y % vb == 0 && align_bytes % (2 * vb) == 0) return vb;
    return 1;
}
// (SpmmTiles of hispmv_spmm.h with vl_* holding VB.)  As there, only the last tile can take another VB than the first.
inline SpmmTiles spmm_bf16_tiles(int64_t cols, int64_t num_vecs, int64_t ld_x, int64_t ld_y, int64_t align_bytes) {
    SpmmTiles t;
    for (int64_t k = 0; k < num_vecs;) {
        const int vb = spmm_bf16_vb(cols, num_vecs - k, ld_x, ld_y, align_bytes);
        const int64_t n = std::min<int64_t>(num_vecs - k, 64 * vb);
        if (t.tiles == 0) t.vl_first = vb;
        t.vl_last = vb; t.last_vecs = n; t.tiles += 1; k += n;
    }
    return t;
}

// Workspace of one part for tiles of 64 * vb vectors: the fp32 partials of hispmv_spmm.h (spmm_work_bytes with VL = vb) ...
inline int64_t spmm_bf16_work_bytes(const SpmvDeviceMatrix& m, int vb) { return spmm_work_bytes(m, vb); }
// ... and, behind the partials of the largest part, for a handle of more than one part the fp32 tile accumulator [rows, 64 * vb]: the
// parts add in fp32 and only the last one rounds.
inline int64_t spmm_bf16_acc_bytes(int64_t rows, int vb) { return rows * 64 * (int64_t)vb * 4; }

// what a finished row reads as its bias, and where it goes
enum : int {
    kBf16BiasShared = 0,      // fp32 bias[row] under every vector
    kBf16BiasMatrix = 1,      // a bf16 matrix laid out like yt (may be yt)
    kBf16BiasAcc = 2,         // the fp32 tile accumulator (a later part of a multi-part handle)
};
struct SpmmBf16Operands {
    const uint16_t* xt; const void* bias; uint16_t* yt; float* work;
    float* acc;                              // [rows, 64 * VB] fp32, or NULL for a handle of one part
    long long ld_x, ld_y;
    int tile0, n_vecs;                       // first vector of the tile, vectors of the call (lanes past them are masked)
    int bias_kind;                           // kBf16Bias*
    int to_acc;                              // 1: the row is stored in fp32 to acc (not the last part); 0: rounded once and stored to yt
    float alpha, beta;
};

// One tile of vectors on one part: the slice grid, then one wavefront per cut row.  alpha != 0.
hipError_t launch_spmm_bf16_part(const SpmvDeviceMatrix& m, int vb, const SpmmBf16Operands& a, hipStream_t stream);
// yt[r, v] = bf16(beta * bias) (+0 when beta == 0: bias is not read) for v < n_vecs: the whole call when alpha == 0.
hipError_t launch_spmm_bf16_bias(const SpmmBf16Operands& a, int32_t rows, hipStream_t stream);

}  // namespace hispmv
