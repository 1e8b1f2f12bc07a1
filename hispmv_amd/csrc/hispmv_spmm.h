// hispmv_spmm.h -- the wide-batch product on feature-major operands (hispmv_spmm.hip; include/hispmv.h: hispmv_spmm_device):
//   yt[r, v] = alpha * sum_k a_rk * xt[k, v] + beta * bias,      xt = [cols, ld_x], yt = [rows, ld_y], row-major
// on the slice stream a loaded handle already holds.  The 64 lanes of a wavefront are 64 * VL vectors (a lane owns VL = 4, 2 or 1
// consecutive ones), the elements of a slice are walked in stream order, and the matrix stream is read once per tile of 64 * VL
// vectors instead of once per 4.  Nothing is stored in the handle for it: the workspace of the cut rows is the caller's.
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

// The tile rule (host-only; hispmv_prep_spmm_tiles): the largest VL in {4, 2, 1} for a tile that begins with `left` vectors to go such that
//   (a) 64 * (VL / 2) < left                         -- do not widen past the batch
//   (b) cols * 64 * VL * 4 <= kSpmmTileBytes         -- at 8 MiB a cap on the columns, not a cache bound: VL 4 up to 8192, VL 2 up to 16384 (measured up to 8192)
//   (c) every ld % VL == 0 and align_bytes % (4 * VL) == 0      -- a lane's VL floats are one aligned load in every row
inline int spmm_vl(int64_t cols, int64_t left, int64_t ld_x, int64_t ld_y, int64_t align_bytes) {
    for (int vl = 4; vl >= 2; vl >>= 1)
        if (64 * (vl / 2) < left && cols * 64 * vl * 4 <= kSpmmTileBytes && ld_x % vl == 0 && ld_y % vl == 0 && align_bytes % (4 * vl) == 0) return vl;
    return 1;
}
struct SpmmTiles { int vl_first = 1, vl_last = 1; int64_t tiles = 0, last_vecs = 0; };
// Only the last tile can take another VL than the first: a tile that is not the last is full, and a full tile leaves (a) as it was.
inline SpmmTiles spmm_tiles(int64_t cols, int64_t num_vecs, int64_t ld_x, int64_t ld_y, int64_t align_bytes) {
    SpmmTiles t;
    for (int64_t k = 0; k < num_vecs;) {
        const int vl = spmm_vl(cols, num_vecs - k, ld_x, ld_y, align_bytes);
        const int64_t n = std::min<int64_t>(num_vecs - k, 64 * vl);
        if (t.tiles == 0) t.vl_first = vl;
        t.vl_last = vl; t.last_vecs = n; t.tiles += 1; k += n;
    }
    return t;
}

// Workspace of one part for tiles of 64 * vl vectors: per slice the partial sum of its open last row and the raw sum of a first row
// that continues a chain, 64 * vl floats each.
inline int64_t spmm_work_bytes(const SpmvDeviceMatrix& m, int vl) { return 2 * m.n_slices * 64 * (int64_t)vl * 4; }
// launches of one tile on this part: the slice grid, and the cut rows if it has any
inline int spmm_part_launches(const SpmvDeviceMatrix& m) { return m.n_slices > 0 ? 1 + ((m.n_fix_short > 0 || m.n_fix_long > 0) ? 1 : 0) : 0; }

struct SpmmOperands {
    const float* xt; const float* bias; float* yt; float* work;
    long long ld_x, ld_y, bias_stride;      // bias_stride 0: bias[row]; ld_y: bias laid out like yt (may be yt)
    int tile0, n_vecs;                       // first vector of the tile, vectors of the call (lanes past them are masked)
    float alpha, beta;
};

// One tile of vectors on one part: the slice grid (one workgroup per group of the forward plan, the forward launch's window in
// the LDS, holding column numbers), then one wavefront per cut row.  alpha != 0.
hipError_t launch_spmm_part(const SpmvDeviceMatrix& m, int vl, const SpmmOperands& a, hipStream_t stream);
// yt[r, v] = beta * bias (0 when beta == 0: bias is not read) for v < n_vecs: the whole call when alpha == 0.
hipError_t launch_spmm_bias(const SpmmOperands& a, int32_t rows, hipStream_t stream);

}  // namespace hispmv
