// hispmv_update.hip -- the kernels of in-place value updates (hispmv_update.h).  Both are bandwidth-bound copies: one workgroup of
// 256 threads per chunk of 1024 slots, four consecutive slots per thread (dwordx4 loads and stores).
#include <hip/hip_runtime.h>

#include <climits>

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

}  // namespace hispmv
