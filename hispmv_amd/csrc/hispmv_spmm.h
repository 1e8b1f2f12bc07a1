// hispmv_spmm.h -- the wide-batch product on feature-major operands (hispmv_spmm.hip; include/hispmv.h: hispmv_spmm_device,
// hispmv_spmm_device_bf16):
//   yt[r, v] = alpha * sum_k a_rk * xt[k, v] + beta * bias,      xt = [cols, ld_x], yt = [rows, ld_y], row-major, fp32 or bf16
// on the slice stream a loaded handle already holds.  The 64 lanes of a wavefront are 64 * V vectors (a lane owns VL = 4, 2 or 1
// consecutive floats, or VB = 8, 4, 2 or 1 bf16: one dwordx4, dwordx2, dword or 16-bit load per stored element), the elements of a slice
// are walked in stream order, and the matrix stream is read once per tile of 64 * V vectors instead of once per 4.  Nothing is stored
// in the handle for it: the workspace of the cut rows is the caller's.
// bf16 activations keep grid, groups, walk, the fp32 accumulators, the +-0 rule, the fp32 workspace of the cut rows and the fix-up launch;
// the value before the one rounding of yt is, bit for bit, what hispmv_spmm_device computes on the widened operands.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdint>

#include "hispmv_kernels.h"

namespace hispmv {

// A tile of xt is cols x 64 * VL floats, gathered once per stored element of the matrix.  The bound began as 2 MiB -- half an XCD's
// 4 MiB L2, from the cache sizes -- and was raised to 8 MiB by the measurement (tools/spmm_bench.py, profiles/spmm_tile_bound_*.json;
// DESIGN.md 2.12): a VL = 1 tile is bound per stored element, not by the bytes gathered, so at 8192 columns wider lanes are faster even
// though their tile of xt no longer fits the L2.  B = 256: 8192 x 8192 d = 0.1 797 us at 2 MiB (VL 1), 477 at 4 MiB (VL 2), 483 at 8 MiB (VL 4);
// 1024 x 8192 391 / 215 / 154 us; 8192 x 8192 d = 0.01 278 / 156 / 138 us.  Bounds above 8 MiB (VL 4 past 8192 columns) were not measured.
constexpr int64_t kSpmmTileBytes = 8ll << 20;

// The tile rule (host-only; hispmv_prep_spmm_tiles, hispmv_prep_spmm_bf16_tiles) for activations of elem_bytes = 4 or 2: the largest
// V in {16 / elem_bytes, ..., 2, 1} for a tile that begins with `left` vectors to go such that
//   (a) 64 * (V / 2) < left                                   -- do not widen past the batch
//   (b) cols * 64 * V * elem_bytes <= kSpmmTileBytes          -- at 8 MiB a cap on the columns, not a cache bound: VL 4 up to 8192, VL 2 up to 16384
//                                                                (measured up to 8192).  bf16 REUSES it UNMEASURED, as the same cap in bytes: VB 8 up to 8192
//   (c) every ld % V == 0 and align_bytes % (elem_bytes * V) == 0      -- a lane's V elements are one aligned load in every row
inline int spmm_lane_width(int elem_bytes, int64_t cols, int64_t left, int64_t ld_x, int64_t ld_y, int64_t align_bytes) {
    for (int v = 16 / elem_bytes; v >= 2; v >>= 1)
        if (64 * (v / 2) < left && cols * 64 * v * elem_bytes <= kSpmmTileBytes && ld_x % v == 0 && ld_y % v == 0 && align_bytes % (elem_bytes * v) == 0) return v;
    return 1;
}
struct SpmmTiles { int vl_first = 1, vl_last = 1; int64_t tiles = 0, last_vecs = 0; };      // (vl_*: VL, or VB for bf16)
// Only the last tile can take another V than the first: a tile that is not the last is full, and a full tile leaves (a) as it was.
inline SpmmTiles spmm_tiles_of(int elem_bytes, int64_t cols, int64_t num_vecs, int64_t ld_x, int64_t ld_y, int64_t align_bytes) {
    SpmmTiles t;
    for (int64_t k = 0; k < num_vecs;) {
        const int v = spmm_lane_width(elem_bytes, cols, num_vecs - k, ld_x, ld_y, align_bytes);
        const int64_t n = std::min<int64_t>(num_vecs - k, 64 * v);
        if (t.tiles == 0) t.vl_first = v;
        t.vl_last = v; t.last_vecs = n; t.tiles += 1; k += n;
    }
    return t;
}
inline int spmm_vl(int64_t cols, int64_t left, int64_t ld_x, int64_t ld_y, int64_t align_bytes) { return spmm_lane_width(4, cols, left, ld_x, ld_y, align_bytes); }
inline int spmm_bf16_vb(int64_t cols, int64_t left, int64_t ld_x, int64_t ld_y, int64_t align_bytes) { return spmm_lane_width(2, cols, left, ld_x, ld_y, align_bytes); }
inline SpmmTiles spmm_tiles(int64_t cols, int64_t num_vecs, int64_t ld_x, int64_t ld_y, int64_t align_bytes) { return spmm_tiles_of(4, cols, num_vecs, ld_x, ld_y, align_bytes); }
inline SpmmTiles spmm_bf16_tiles(int64_t cols, int64_t num_vecs, int64_t ld_x, int64_t ld_y, int64_t align_bytes) { return spmm_tiles_of(2, cols, num_vecs, ld_x, ld_y, align_bytes); }

// Workspace of one part for tiles of 64 * vl vectors (fp32 and bf16 alike): per slice the fp32 partial sum of its open last row and the
// raw sum of a first row that continues a chain, 64 * vl floats each ...
inline int64_t spmm_work_bytes(const SpmvDeviceMatrix& m, int vl) { return 2 * m.n_slices * 64 * (int64_t)vl * 4; }
inline int64_t spmm_bf16_work_bytes(const SpmvDeviceMatrix& m, int vb) { return spmm_work_bytes(m, vb); }
// ... and, bf16 only, behind the partials of the largest part, for a handle of more than one part the fp32 tile accumulator
// [rows, 64 * vb]: the parts add in fp32 and only the last one rounds.
inline int64_t spmm_bf16_acc_bytes(int64_t rows, int vb) { return rows * 64 * (int64_t)vb * 4; }
// launches of one tile on this part: the slice grid, and the cut rows if it has any
inline int spmm_part_launches(const SpmvDeviceMatrix& m) { return m.n_slices > 0 ? 1 + ((m.n_fix_short > 0 || m.n_fix_long > 0) ? 1 : 0) : 0; }

struct SpmmOperands {
    using Elem = float;                      // of xt and yt
    const float* xt; const float* bias; float* yt; float* work;
    long long ld_x, ld_y, bias_stride;      // bias_stride 0: bias[row]; ld_y: bias laid out like yt (may be yt)
    int tile0, n_vecs;                       // first vector of the tile, vectors of the call (lanes past them are masked)
    float alpha, beta;
};

// what a finished row of a bf16 call reads as its bias, and where it goes
enum : int {
    kBf16BiasShared = 0,      // fp32 bias[row] under every vector
    kBf16BiasMatrix = 1,      // a bf16 matrix laid out like yt (may be yt)
    kBf16BiasAcc = 2,         // the fp32 tile accumulator (a later part of a multi-part handle)
};
struct SpmmBf16Operands {
    using Elem = uint16_t;                   // of xt and yt
    const uint16_t* xt; const void* bias; uint16_t* yt; float* work;
    float* acc;                              // [rows, 64 * VB] fp32, or NULL for a handle of one part
    long long ld_x, ld_y;
    int tile0, n_vecs;                       // first vector of the tile, vectors of the call (lanes past them are masked)
    int bias_kind;                           // kBf16Bias*
    int to_acc;                              // 1: the row is stored in fp32 to acc (not the last part); 0: rounded once and stored to yt
    float alpha, beta;
};

// One tile of vectors on one part: the slice grid (one workgroup per group of the forward plan, the forward launch's window in
// the LDS, holding column numbers), then one wavefront per cut row.  alpha != 0.
hipError_t launch_spmm_part(const SpmvDeviceMatrix& m, int vl, const SpmmOperands& a, hipStream_t stream);
hipError_t launch_spmm_bf16_part(const SpmvDeviceMatrix& m, int vb, const SpmmBf16Operands& a, hipStream_t stream);
// yt[r, v] = beta * bias, rounded once for bf16 (+0 when beta == 0: bias is not read), for v < n_vecs: the whole call when alpha == 0.
hipError_t launch_spmm_bias(const SpmmOperands& a, int32_t rows, hipStream_t stream);
hipError_t launch_spmm_bf16_bias(const SpmmBf16Operands& a, int32_t rows, hipStream_t stream);

}  // namespace hispmv
