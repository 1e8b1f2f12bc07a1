// hispmv_spmm_grad.h -- the wide-batch value gradient on feature-major operands (hispmv_spmm_grad.hip; include/hispmv.h:
// hispmv_spmm_value_grad_device, hispmv_spmm_value_grad_device_bf16):
//   grad[k] = alpha * sum_{v < n_vecs} gyt[row_k, v] * xt[col_k, v] + beta * grad[k],      gyt = [rows, ld_gy], xt = [cols, ld_x], row-major
// for every entry k of the creation input of a loaded, updatable slice-stream handle; gyt and xt fp32 or bf16, grad, alpha and beta fp32.
// Grid, groups and walk are those of the wide-batch product (hispmv_spmm.h): the 64 lanes of a wavefront are 64 * V vectors (a lane owns
// V = 4, 2 or 1 floats, or 8, 4, 2 or 1 bf16: one load per stored element and per row of gyt), the elements of a slice are walked in
// stream order, and the slice stream -- its metas only -- is read once per tile of 64 * V vectors instead of once per 4
// (hispmv_value_grad.h).  The tiles follow spmm_tiles / spmm_bf16_tiles (hispmv_spmm.h) with the smaller alignment of the two operands.
//
// BITS.  Widening a bf16 is exact.  The sum of an entry over one tile has a fixed order: a lane's V products ascending,
// p = (+0 + gy[0] * x[0]) + gy[1] * x[1] + ..., unfused, the product of a vector >= n_vecs replaced by +0; then the pairwise tree over the
// 64 lanes -- lanes (2i, 2i + 1), then pairs of pairs, ... -- and grad = alpha * s + beta * grad.  Tiles add one after the other (the
// first with the caller's beta, every later one with beta = 1).  Two identical calls give identical bits; the bits depend on (num_vecs,
// ld, alignment) through V and the tiles.  They are NOT the bits of hispmv_value_grad_device and they are NOT independent of the batch;
// where a bf16 tile has VB <= 4 and the same boundaries they are the bits of the fp32 entry on the widened operands.  Nothing is stored
// in the handle, there is no workspace, no second launch and no atomic.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "hispmv_kernels.h"

namespace hispmv {

template <class T> struct SpmmGradOperandsOf {
    const T* gyt; const T* xt; float* grad;
    long long ld_gy, ld_x, n;                // n: entries of the creation input (the length of grad)
    int tile0, n_vecs;                       // first vector of the tile, vectors of the call (lanes and lane parts past them add +0)
    float alpha, beta;
};
using SpmmGradOperands = SpmmGradOperandsOf<float>;
using SpmmGradBf16Operands = SpmmGradOperandsOf<uint16_t>;

// One tile of vectors on one part: one workgroup per group of the forward plan, the forward launch's window in the LDS holding column
// numbers.  `map`: the part's chunks of the handle's value map (chunk s = slice s of the part); a word q in 1 .. n names entry q - 1,
// every other word writes nothing.  Every entry has one writer per launch.  alpha != 0.  tile0, both leading dimensions and both
// operand addresses must be multiples of a lane's vl floats (vb bf16), so that they are one aligned load inside the row: (c) of the tile rule.
hipError_t launch_spmm_grad_part(const SpmvDeviceMatrix& m, int vl, const int32_t* map, const SpmmGradOperands& a, hipStream_t stream);
hipError_t launch_spmm_grad_bf16_part(const SpmvDeviceMatrix& m, int vb, const int32_t* map, const SpmmGradBf16Operands& a, hipStream_t stream);

}  // namespace hispmv
