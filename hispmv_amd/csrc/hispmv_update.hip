// hispmv_update.hip -- the kernels of in-place value updates (hispmv_update.h).  Bandwidth-bound copies: one workgroup of
// 256 threads per chunk of 1024 slots, four consecutive slots per thread (dwordx4 loads and stores).  bf16 handles have kernels of
// their own that round on the way (a half slice takes 8 of a thread's 16 bytes); the fp32 kernels do not know about them.
#include <hip/hip_runtime.h>

#include <climits>

#include "hispmv_format.h"
#include "hispmv_update.h"

namespace hispmv {

namespace {

typedef int i4v __attribute__((ext_vector_type(4)));
typedef float f4v __attribute__((ext_vector_type(4)));

constexpr int kUpdateThreads = kValueChunk / 4;

__global__ __launch_bounds__(kUpdateThreads) void build_value_map_kernel(const ValueChunkDev* __restrict__ table, int32_t* __restrict__ map) {
    const ValueChunkDev ch = table[blockIdx.x];
    const i4v v = *((const i4v*)ch.dst0 + threadIdx.x);
    *((i4v*)(map + ch.map_off) + threadIdx.x) = v;
}

__device__ __forceinline__ float gather_value(int32_t k, const float* __restrict__ values, int64_t n) {
    return (k > 0 && (int64_t)k <= n) ? values[k - 1] : 0.0f;
}

__global__ __launch_bounds__(kUpdateThreads) void update_values_kernel(const ValueChunkDev* __restrict__ table, const int32_t* __restrict__ map,
                                                                      const float* __restrict__ values, int64_t n) {
    const ValueChunkDev ch = table[blockIdx.x];
    const i4v k = __builtin_nontemporal_load((const i4v*)(map + ch.map_off) + threadIdx.x);
    f4v v;
    v.x = gather_value(k.x, values, n);
    v.y = gather_value(k.y, values, n);
    v.z = gather_value(k.z, values, n);
    v.w = gather_value(k.w, values, n);
    __builtin_nontemporal_store(v, (f4v*)ch.dst0 + threadIdx.x);
    if (ch.dst1) __builtin_nontemporal_store(v, (f4v*)ch.dst1 + threadIdx.x);
}

// round_bits_to_bf16 (hispmv_format.h) in its integer form, on the device: nearest, ties to even; +-Inf stay; a finite value above
// the largest bf16 carries into the exponent and becomes Inf; a NaN keeps its sign and upper payload and gets the quiet bit;
// subnormals round like every other value (no flush).  The hardware conversion is not used: it need not agree on NaNs.
__device__ __forceinline__ uint32_t round_bits_to_bf16_device(uint32_t u) {
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u & 0xffff0000u) | 0x00400000u;
    return (u + 0x7fffu + ((u >> 16) & 1u)) & 0xffff0000u;
}
__device__ __forceinline__ uint32_t gather_rounded(int32_t k, const float* __restrict__ values, int64_t n) {
    return round_bits_to_bf16_device(__builtin_bit_cast(uint32_t, gather_value(k, values, n)));
}

typedef unsigned int u4v __attribute__((ext_vector_type(4)));
typedef unsigned int u2v __attribute__((ext_vector_type(2)));

// one destination of a chunk: thread t owns elements 4t .. 4t + 3 -- 16 bytes of fp32 slots, or the value half of piece t of a half slice
__device__ __forceinline__ void store_rounded(float* dst, bool half, u4v r, unsigned t) {
    if (half) __builtin_nontemporal_store(u2v{(r.x >> 16) | r.y, (r.z >> 16) | r.w}, (u2v*)((char*)dst + 16u * t));      // (the lower halves of r are 0)
    else __builtin_nontemporal_store(r, (u4v*)dst + t);
}

__global__ __launch_bounds__(kUpdateThreads) void update_values_bf16_kernel(const ValueChunkDev* __restrict__ table, const int32_t* __restrict__ map,
                                                                           const float* __restrict__ values, int64_t n) {
    const ValueChunkDev ch = table[blockIdx.x];
    const int64_t map_off = ch.map_off & ~(kChunkHalf0 | kChunkHalf1);
    const i4v k = __builtin_nontemporal_load((const i4v*)(map + map_off) + threadIdx.x);
    u4v r;
    r.x = gather_rounded(k.x, values, n);
    r.y = gather_rounded(k.y, values, n);
    r.z = gather_rounded(k.z, values, n);
    r.w = gather_rounded(k.w, values, n);
    store_rounded(ch.dst0, (ch.map_off & kChunkHalf0) != 0, r, threadIdx.x);
    if (ch.dst1) store_rounded(ch.dst1, (ch.map_off & kChunkHalf1) != 0, r, threadIdx.x);
}

// Dense bf16 W: convert and copy.  VEC: thread i takes elements 4i .. 4i + 3 (one 16-byte load, one 8-byte store) of the first n4
// elements; the other instantiation takes one element per thread from `first` on (the tail, or everything when a pointer is not aligned).
template <bool VEC>
__global__ __launch_bounds__(256) void update_dense_bf16_kernel(uint16_t* __restrict__ dst, const float* __restrict__ src, int64_t first, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if constexpr (VEC) {
        if (i * 4 + 3 >= n) return;
        const u4v v = __builtin_nontemporal_load((const u4v*)src + i);
        const u2v o = {(round_bits_to_bf16_device(v.x) >> 16) | round_bits_to_bf16_device(v.y), (round_bits_to_bf16_device(v.z) >> 16) | round_bits_to_bf16_device(v.w)};
        __builtin_nontemporal_store(o, (u2v*)dst + i);
    } else {
        if (first + i >= n) return;
        dst[first + i] = (uint16_t)(round_bits_to_bf16_device(__builtin_bit_cast(uint32_t, src[first + i])) >> 16);
    }
}

}  // namespace

hipError_t launch_build_value_map(const ValueChunkDev* d_table, int64_t n_chunks, int32_t* d_map, hipStream_t s) {
    if (n_chunks <= 0) return hipSuccess;
    if (n_chunks > INT32_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(build_value_map_kernel, dim3((unsigned)n_chunks), dim3(kUpdateThreads), 0, s, d_table, d_map);
    return hipGetLastError();
}

hipError_t launch_update_values(const ValueChunkDev* d_table, int64_t n_chunks, const int32_t* d_map, const float* d_values, int64_t n,
                                hipStream_t s) {
    if (n_chunks <= 0) return hipSuccess;
    if (n_chunks > INT32_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(update_values_kernel, dim3((unsigned)n_chunks), dim3(kUpdateThreads), 0, s, d_table, d_map, d_values, n);
    return hipGetLastError();
}

hipError_t launch_update_values_bf16(const ValueChunkDev* d_table, int64_t n_chunks, const int32_t* d_map, const float* d_values, int64_t n,
                                     hipStream_t s) {
    if (n_chunks <= 0) return hipSuccess;
    if (n_chunks > INT32_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(update_values_bf16_kernel, dim3((unsigned)n_chunks), dim3(kUpdateThreads), 0, s, d_table, d_map, d_values, n);
    return hipGetLastError();
}

hipError_t launch_update_dense_bf16(uint16_t* d_dst, const float* d_src, int64_t n, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (!d_dst || !d_src) return hipErrorInvalidValue;
    // 16-byte loads and 8-byte stores for the whole quads when the pointers allow, single elements for the rest
    const bool vec = ((uintptr_t)d_src & 15) == 0 && ((uintptr_t)d_dst & 7) == 0;
    const int64_t n4 = vec ? n & ~(int64_t)3 : 0;
    const int64_t vec_blocks = (n4 / 4 + 255) / 256, tail_blocks = (n - n4 + 255) / 256;
    if (vec_blocks > INT32_MAX || tail_blocks > INT32_MAX) return hipErrorInvalidValue;
    if (vec_blocks > 0) hipLaunchKernelGGL(update_dense_bf16_kernel<true>, dim3((unsigned)vec_blocks), dim3(256), 0, s, d_dst, d_src, (int64_t)0, n4);
    if (tail_blocks > 0) hipLaunchKernelGGL(update_dense_bf16_kernel<false>, dim3((unsigned)tail_blocks), dim3(256), 0, s, d_dst, d_src, n4, n);
    return hipGetLastError();
}

}  // namespace hispmv
