// hispmv_transpose.h -- launchers of the transposed product y[cols] = alpha * A^T * x[rows] + beta * bias[cols] on the layouts a loaded
// handle already holds (hispmv_transpose.hip; include/hispmv.h: hispmv_spmv_device_t).  Nothing is stored for it: the row of a slice
// element is its slice's row_base plus the row ends before it, its column is the meta (through the group's fragment table where the
// meta is a window index), and the LDS window that holds x in the forward kernel holds the accumulators of y here.  Sums into one
// y[col] arrive through float atomics, in no fixed order.  A stored slot whose value is +-0 adds nothing, whatever x holds.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "hispmv_kernels.h"

namespace hispmv {

// y[i] = beta * bias[i] (0 when beta == 0: bias is not read), i < n.  Elementwise, so bias may be y.
// `vecs` vectors in the one launch: y[v * n + i] = beta * bias[v * bias_stride + i], bias_stride 0 (one bias for all) or n.
hipError_t launch_transpose_prologue(const float* bias, float* y, int32_t n, float beta, hipStream_t stream, int64_t vecs = 1,
                                     int64_t bias_stride = 0);

// y += alpha * A^T * x for one slice stream (one part of a handle) and nv = 1, 2 or 4 vectors in one pass over the stream: one
// workgroup per group of the part's plan, the forward launch's workgroup size.  Vector v reads x + v * m.rows (m.rows floats) and adds
// into y + v * m.cols (m.cols floats).  The LDS holds nv accumulator windows and one x tile per wavefront: slice_lds_bytes(m, nv), with
// nv = 1 the forward launch's.  spmv_t_width: the widest pass (4, 2, 1) for `vecs` vectors left; a plan without a window always takes
// 4.  nv > 1 must be what spmv_t_width gives for nv vectors; any other nv is hipErrorInvalidValue.  No alignment condition on x or y.
int spmv_t_width(const SpmvDeviceMatrix& m, int64_t vecs);
hipError_t launch_spmv_t(const SpmvDeviceMatrix& m, int nv, const float* x, float* y, float alpha, hipStream_t stream);

// y += alpha * W^T * x, W row-major rows x cols (fp32, or bfloat16 when bf16).  The rows are split over gemv_t_row_blocks() workgroups
// per block of kGemvTCols columns; their column sums meet in y through one contiguous atomic per 64 columns (plain read-add-write when
// one row block suffices).  nv = 1, 2, 4 or 8 vectors per pass over W (x + v * rows -> y + v * cols; any other nv is
// hipErrorInvalidValue); gemv_t_width: 8, 4, 2, 1 by the vectors left.
constexpr int kGemvTCols = 1024;
int gemv_t_row_blocks(int32_t rows, int32_t cols);
int gemv_t_width(int64_t vecs);
hipError_t launch_gemv_t(const void* W, int32_t rows, int32_t cols, bool bf16, int nv, const float* x, float* y, float alpha, hipStream_t stream);

}  // namespace hispmv
