// hispmv_block_jacobi.h -- the block-Jacobi preconditioner (hispmv_block_jacobi.hip; include/hispmv.h: "Block-Jacobi preconditioner"): the
// layout rule of the caller's buffer, which the host-only hispmv_prep_block_jacobi and the device entries follow, and the launchers of
// the extraction, the batched inversion and the multiply.  The arithmetic of the inversion and of the multiply is written down in
// include/hispmv.h; the multiply of a thread, which the CG and GMRES kernels share, is hispmv_block_jacobi_device.h's.
//
// The extraction walks the slice stream like the transposed product and adds every stored value of a diagonal block into its word with
// a hardware float atomic.  An entry stored once is one add onto +0: the same bits every run.  Two duplicates of one position give the
// same bits in either order (fp addition commutes).  THREE OR MORE duplicates of one position are summed in no fixed order.  A stored
// +-0 (fillers, padding, explicit zeros) adds nothing.  As for the y of hispmv_spmv_device_t, the buffer must be ordinary device memory
// (hipMalloc, a torch CUDA tensor): float atomics on fine-grained or host-mapped memory are not what these kernels issue.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "hispmv_kernels.h"

namespace hispmv {

constexpr int kBlockJacobiThreads = 256;
inline bool block_jacobi_size_ok(int64_t bs) { return bs == 4 || bs == 8 || bs == 16 || bs == 32; }

// The buffer: n_blocks blocks of bs x bs floats, row-major, block k the inverse of diagonal block k (16-byte aligned, the size a
// multiple of 16 bytes); then n_blocks int32 flags, 0 = inverted, 1 = replaced by the identity; the whole rounded up to 16 bytes.
struct BlockJacobiLayout {
    int64_t n_blocks = 0, block_floats = 0, off_flags = 0, pre_bytes = 0;
};
inline BlockJacobiLayout block_jacobi_layout(int64_t n, int64_t bs) {
    BlockJacobiLayout l;
    l.n_blocks = (n + bs - 1) / bs;
    l.block_floats = bs * bs;
    l.off_flags = (l.n_blocks * l.block_floats * 4 + 15) / 16 * 16;
    l.pre_bytes = (l.off_flags + l.n_blocks * 4 + 15) / 16 * 16;
    return l;
}

// blocks = zeros, plus ones on the diagonal of the rows at or beyond n of the last block (slice streams: before the walks)
hipError_t launch_block_jacobi_fill(float* blocks, int64_t n, int bs, hipStream_t s);
// blocks += the stored values of one slice stream (one part of a handle) that lie in a diagonal block, rows and columns below n
hipError_t launch_block_jacobi_walk(const SpmvDeviceMatrix& m, float* blocks, int64_t n, int bs, hipStream_t s);
// blocks = the padded diagonal blocks of W, row-major n x n (fp32, or bfloat16 widened when bf16); no atomics, no fill needed
hipError_t launch_block_jacobi_dense(const void* W, bool bf16, float* blocks, int64_t n, int bs, hipStream_t s);
// blocks[k] = its inverse (or the identity) in place, flags[k] = 0 (or 1), k < n_blocks
hipError_t launch_block_invert(float* blocks, int32_t* flags, int64_t n_blocks, int bs, hipStream_t s);
// z = M^-1 r over n elements on the Krylov layer's grid
hipError_t launch_block_jacobi_apply(const float* blocks, int64_t n, int bs, const float* r, float* z, hipStream_t s);

}  // namespace hispmv
