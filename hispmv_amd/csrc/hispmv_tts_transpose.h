// hispmv_tts_transpose.h -- launchers of the transposed product y[cols] += alpha * A^T * x[rows] and of the value gradient on the
// TRANSPOSED TILE STREAM of a loaded handle (hispmv_tts.h; kernels: hispmv_tts_transpose.hip; include/hispmv.h: hispmv_spmv_device_t,
// hispmv_linear_device_t, hispmv_value_grad_device).  Nothing is stored for them: they are the forward tile kernel run backwards.
//   forward (hispmv_kernels.hip: tts_tile_body)                 transposed / value gradient
//   row accumulators of the tile in the LDS                     x (gradient: gy) of the tile's rows, one coalesced load
//   phase A, column order: gather x, product -> staging[slot]   SECOND: staging[slot] * value -> atomic add into y[col]
//                                                               (gradient: staging[slot] * x[col] -> grad through the value map)
//   phase B, row order: reduce the staging by the row ends      FIRST: expand -- staging[slot] = x[row(slot)], the row of a slot
//                                                               being the chunk's row base plus the row ends before it
//   chunk tails, carry[] of cut rows, the fix-up launch         none: a piece of a cut row reads the row's x through `fix`
// Accepted: a one-part stream with stream words for every row (TtsDeviceMatrix::zero_fill == 0: the standard and the small geometry).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "hispmv_kernels.h"

namespace hispmv {

// the stream is one these launchers read (zero_fill == 0, a workgroup of whole wavefronts, the one-vector LDS fits a CU)
bool tts_t_accepts(const TtsDeviceMatrix& m);
// The widest pass (4, 2; 1 = the one-vector kernel) for `vecs` vectors left: the largest of {4, 2} that is <= vecs and for which nv
// copies of [x rows: acc_floats][staging: batch_stage_floats][64] fit kDynLdsMax -- the forward rule (tts_batch_width) without its
// x-in-LDS branch, with the forward kernel's byte count, so one host mirror serves both.
int tts_t_width(const TtsDeviceMatrix& m, int64_t vecs);

// y[v * cols + c] += alpha * sum over the stored words of column c of value * x[v * rows + row], v < nv (1, 2 or 4 = tts_t_width).
// One workgroup of m.threads per tile.  A word whose value is +-0 adds nothing (fillers, padding, explicit zeros).  Float atomics, no
// fixed order.  carry[] is neither read nor written; no fix-up launch follows.  No alignment condition on x or y.
hipError_t launch_tts_t(const TtsDeviceMatrix& m, int nv, const float* x, float* y, float alpha, hipStream_t stream);

// grad[q - 1] = alpha * s + beta * grad[q - 1] for every stream word whose map word q names an input entry (1 <= q <= n);
// s = (+0 + gy[0, row] * x[0, col]) + gy[1, row] * x[1, col] ... over the nv vectors of the pass, products and adds unfused.
// `map`: the part's chunks of the value map, one chunk of kValueChunk words per 1024-word slice, in the order of the words.  The
// values are not read.  One writer per grad[k]: plain stores, the same bits run to run.  beta == 0 does not read grad.
hipError_t launch_tts_value_grad(const TtsDeviceMatrix& m, int nv, const int32_t* map, const float* gy, const float* x, float* grad, int64_t n,
                                 float alpha, float beta, hipStream_t stream);

}  // namespace hispmv
