// hispmv_spmm_grad_bf16.h -- the wide-batch value gradient with bf16 activations (hispmv_spmm_grad_bf16.hip; include/hispmv.h:
// hispmv_spmm_value_grad_device_bf16):
//   grad[k] = alpha * sum_{v < n_vecs} gyt[row_k, v] * xt[col_k, v] + beta * grad[k],      gyt = [rows, ld_gy], xt = [cols, ld_x], row-major, bf16
// hispmv_spmm_grad.h with 2-byte operands; grad, alpha and beta stay fp32.  Grid, groups, walk and the order of the sum are those of the
// fp32 entry; a lane owns VB = 8, 4, 2 or 1 consecutive vectors (one dwordx4, dwordx2, dword or 16-bit load per stored element and per
// row of gyt), so a tile is 64 * VB vectors.  The tiles follow spmm_bf16_tiles (hispmv_spmm_bf16.h) with the smaller alignment of the
// two operands.
//
// BITS.  Widening a bf16 is exact.  The sum of an entry over one tile: a lane's VB products ascending, p = (+0 + gy[0] * x[0]) + gy[1] *
// x[1] + ..., unfused, the product of a vector >= n_vecs replaced by +0; then the pairwise tree over the 64 lanes; then alpha * s + beta *
// grad for the first tile and grad + alpha * s for every later one.  Where a tile has VB <= 4 and the same boundaries these are the bits
// of hispmv_spmm_value_grad_device on the widened operands.  No workspace, no second launch, no atomic, nothing kept in the handle.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "hispmv_kernels.h"

namespace hispmv {

struct SpmmGradBf16Operands {
    const uint16_t* gyt; const uint16_t* xt; float* grad;
    long long ld_gy, ld_x, n;                // n: entries of the creation input (the length of grad)
    int tile0, n_vecs;                       // first vector of the tile, vectors of the call (lanes and lane parts past them add +0)
    float alpha, beta;
};

// launch_spmm_grad_part (hispmv_spmm_grad.h) for lanes of vb bf16.  Beyond its checks: tile0, both leading dimensions and both operand
// addresses must be multiples of vb elements, so that a lane's vb halves are one aligned load inside the row.  alpha != 0.
hipError_t launch_spmm_grad_bf16_part(const SpmvDeviceMatrix& m, int vb, const int32_t* map, const SpmmGradBf16Operands& a, hipStream_t stream);

}  // namespace hispmv
