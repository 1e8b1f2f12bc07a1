// hispmv_krylov_device.h -- the device helpers the vector kernels of hispmv_krylov.hip and hispmv_gmres.hip share: the 4-float accesses
// of a thread, the fixed-order fp64 sums (include/hispmv.h: the dot product) and the walk over a workgroup's chunks.  Included by
// these two kernel files only; everything is internal to the including file.
#pragma once
#include <hip/hip_runtime.h>

#include "hispmv_krylov.h"

namespace hispmv {
namespace {

// the vector at p is 16-byte aligned (i is a multiple of 4): decided per vector, so one 4-byte-aligned operand of the caller's does
// not take the 16-byte accesses from the others of the pass
__device__ __forceinline__ bool aligned16(const float* p) { return ((uintptr_t)p & 15) == 0; }
// v[0 .. m) = p[i .. i + m), the rest +0
__device__ __forceinline__ void ld4(const float* p, int64_t i, int m, float v[4]) {
    if (aligned16(p) && m == 4) {
        const float4 f = *reinterpret_cast<const float4*>(p + i);
        v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = j < m ? p[i + j] : 0.0f;
}
__device__ __forceinline__ void st4(float* p, int64_t i, int m, const float v[4]) {
    if (aligned16(p) && m == 4) {
        *reinterpret_cast<float4*>(p + i) = make_float4(v[0], v[1], v[2], v[3]);
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j < m) p[i + j] = v[j];
}
// the 4 products of a thread, exact in fp64, summed ascending from +0
__device__ __forceinline__ double dot4(const float a[4], const float b[4], int m) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j < m) s += (double)a[j] * (double)b[j];
    return s;
}

// The pairwise tree over the 256 threads: v[t] += v[t + 128], then + 64, 32, ... 1; every thread returns v[0].
__device__ double block_sum(double v, double* sh) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    if (t < 128) sh[t] += sh[t + 128];
    __syncthreads();
    if (t < 64) {
        double w = sh[t] + sh[t + 64];
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) w += __shfl_down(w, s, 64);
        if (t == 0) sh[0] = w;
    }
    __syncthreads();
    const double r = sh[0];
    __syncthreads();
    return r;
}
// The sum of `groups` <= 1024 partials: thread t adds part[4t .. 4t + 3] ascending from +0, then the tree.
[[maybe_unused]] __device__ double sum_partials(const double* part, int64_t groups, double* sh) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t i = 4 * (int64_t)threadIdx.x + j;
        if (i < groups) s += part[i];
    }
    return block_sum(s, sh);
}
__device__ __forceinline__ int64_t groups_of(int64_t n) {
    const int64_t c = (n + kKrylovChunk - 1) / kKrylovChunk;
    return c < kKrylovMaxGroups ? c : kKrylovMaxGroups;
}
__device__ __forceinline__ void load_state(const double* s_in, double S[kKrylovState]) {
#pragma unroll
    for (int i = 0; i < kKrylovState; ++i) S[i] = s_in[i];
}
__device__ __forceinline__ void store_state(double* s_out, const double S[kKrylovState]) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < kKrylovState; ++i) s_out[i] = S[i];
    }
}

// f(i, m) for every chunk of this workgroup, ascending: i = the thread's first element, m = how many of its 4 lie below n
template <class F>
__device__ __forceinline__ void for_chunks(int64_t n, F&& f) {
    const int64_t chunks = (n + kKrylovChunk - 1) / kKrylovChunk;
    for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const int64_t i = c * kKrylovChunk + 4 * (int64_t)threadIdx.x;
        const int64_t left = n - i;
        f(i, left >= 4 ? 4 : left > 0 ? (int)left : 0);
    }
}

inline unsigned grid_of(int64_t n) {
    const int64_t g = krylov_groups(n);
    return (unsigned)(g > 0 ? g : 1);
}

}  // namespace
}  // namespace hispmv
