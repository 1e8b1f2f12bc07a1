// hispmv_value_grad.h -- launchers of the value gradient grad[k] = alpha * sum_v gy[v, row_k] * x[v, col_k] + beta * grad[k] for every
// entry k of the creation input of a loaded, updatable handle (hispmv_value_grad.hip; include/hispmv.h: hispmv_value_grad_device).
// Nothing is stored for it: the row of a slice element is its slice's row_base plus the row ends before it (the transposed kernel's
// decode), its column is the meta (the forward kernel's x window, stray areas and gathers), and the position k of the input entry a
// slot holds is the value map of hispmv_update.h.  Every input entry lives in exactly one slot of a handle's first layouts, so every
// grad[k] has one writer per launch: plain stores, no atomics, the same bits run to run.  The values themselves are not read.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "hispmv_kernels.h"

namespace hispmv {

// One pass of nv = 1, 2 or 4 vectors over one slice stream (one part of a handle): one workgroup per group of the part's plan with the
// plan's workgroup size; LDS = slice_lds_bytes(m, nv): [nv x windows of m.lds_floats, stray areas included][one gy tile per wavefront].
// `map`: the part's chunks of the handle's value map (m.n_slices * kValueChunk words, chunk s = slice s of the part); every word q with
// 1 <= q <= n names grad[q - 1], every other word writes nothing.  gy: nv x m.rows, x: nv x m.cols, row-major.
//   grad[q - 1] = alpha * s + beta * grad[q - 1]      (beta == 0: grad is not read),
// s = (+0 + gy[0, r] * x[0, c]) + gy[1, r] * x[1, c] ..., products and sums unfused.  No alignment condition on any pointer.
hipError_t launch_value_grad(const SpmvDeviceMatrix& m, int nv, const int32_t* map, const float* gy, const float* x, float* grad, int64_t n,
                             float alpha, float beta, hipStream_t stream);

// Dense: grad[r * cols + c] = alpha * sum_v gy[v, r] * x[v, c] + beta * grad[r * cols + c], all `vecs` vectors in ONE launch, summed
// ascending from +0.  A thread owns 4 consecutive columns of kValueGradRows consecutive rows; 16-byte accesses when cols % 4 == 0 and x and
// grad are 16-byte aligned, element accesses otherwise (the same bits).
constexpr int kValueGradRows = 4;
hipError_t launch_value_grad_dense(int32_t rows, int32_t cols, int64_t vecs, const float* gy, const float* x, float* grad, float alpha, float beta,
                                   hipStream_t stream);

}  // namespace hispmv
