// hispmv_slice_decode.h -- the ONE text of the slice format's decode, for all six kernel files: hispmv_kernels.hip includes it directly,
// the five satellite files through hispmv_slice_walk.h.  The bit casts, the loads of the packed stream, the lane count below a ballot,
// a slice as it arrives (SliceRaw, request_slice) and its metas in wide form (decode_metas).  A change of the slice format
// (hispmv_format.h) is made here once.  Nothing but these small inlined pieces: the walk, the scan and every kernel body stay with
// their files.  Everything sits in an unnamed namespace: every including file gets its own copy, as it had when the
// text was written out in each of them.
#pragma once
#include <hip/hip_runtime.h>

#include "hispmv_format.h"

namespace hispmv {

namespace {

__device__ __forceinline__ int f2i(float f) { return __builtin_bit_cast(int, f); }
__device__ __forceinline__ float i2f(int i) { return __builtin_bit_cast(float, i); }

__device__ __forceinline__ int lanes_below(unsigned long long mask) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

// One 16-byte / 8-byte piece of the packed stream.  The stream is read exactly once per launch: the non-temporal
// hint keeps it from evicting x, y and the fragment tables from L2 (measured: -5..8 % kernel time on
// PFlow_742, soc-Pokec and mouse_gene).
// Every pointer is cast to the GLOBAL address space first: the multi-matrix kernel takes its pointers from a table in
// memory, where hipcc cannot tell global from LDS and would emit FLAT loads -- those count on lgkmcnt as well and return
// out of order, so every wait for an LDS gather would also wait for the prefetch of the next slice.
#define HISPMV_GLOBAL __attribute__((address_space(1)))
__device__ __forceinline__ uint4 load_words(const uint4* p) {
    typedef unsigned int u4v __attribute__((ext_vector_type(4)));
    const u4v v = __builtin_nontemporal_load((const HISPMV_GLOBAL u4v*)p);
    return uint4{v.x, v.y, v.z, v.w};
}
__device__ __forceinline__ uint2 load_words2(const uint2* p) {
    typedef unsigned int u2v __attribute__((ext_vector_type(2)));
    const u2v v = __builtin_nontemporal_load((const HISPMV_GLOBAL u2v*)p);
    return uint2{v.x, v.y};
}
__device__ __forceinline__ int4 load_int4(const int4* p) {
    typedef int i4v __attribute__((ext_vector_type(4)));
    const i4v v = *(const HISPMV_GLOBAL i4v*)p;
    return int4{v.x, v.y, v.z, v.w};
}

// A slice as it arrives: per step 4 values and 4 metas per lane (compact: 4 x u16 in a uint2; wide: 4 x u32).
// HALF (bf16 value storage, hispmv_format.h): per step ONE 16-byte piece per lane, {v0 | v1 << 16, v2 | v3 << 16, m0 | m1 << 16, m2 | m3 << 16}.
template <bool COMPACT, bool HALF = false> struct SliceRaw;
template <> struct SliceRaw<true>  { uint4 v[kSliceSteps]; uint2 m[kSliceSteps]; };
template <> struct SliceRaw<false> { uint4 v[kSliceSteps]; uint4 m[kSliceSteps]; };
template <> struct SliceRaw<true, true> { uint4 q[kSliceSteps]; };
template <bool COMPACT, bool HALF>
__device__ __forceinline__ void request_slice(SliceRaw<COMPACT, HALF>& s, const char* base, int lane) {
    if constexpr (HALF) {
        const uint4* pq = (const uint4*)base + lane;
#pragma unroll
        for (int j = 0; j < kSliceSteps; ++j) s.q[j] = load_words(pq + j * 64);
    } else {
        const uint4* pv = (const uint4*)base + lane;
#pragma unroll
        for (int j = 0; j < kSliceSteps; ++j) s.v[j] = load_words(pv + j * 64);
        if constexpr (COMPACT) {
            const uint2* pm = (const uint2*)(base + kSliceElems * 4) + lane;
#pragma unroll
            for (int j = 0; j < kSliceSteps; ++j) s.m[j] = load_words2(pm + j * 64);
        } else {
            const uint4* pm = (const uint4*)(base + kSliceElems * 4) + lane;
#pragma unroll
            for (int j = 0; j < kSliceSteps; ++j) s.m[j] = load_words(pm + j * 64);
        }
    }
}
// -> metas in wide form (rowEnd << 31 | window index or column), c[4*j + k] = element k of the lane in step j
template <bool COMPACT, bool HALF>
__device__ __forceinline__ void decode_metas(const SliceRaw<COMPACT, HALF>& s, unsigned (&c)[kSliceSteps * kLaneElems]) {
    if constexpr (COMPACT) {
#pragma unroll
        for (int j = 0; j < kSliceSteps; ++j) {
            unsigned a, b;
            if constexpr (HALF) { a = s.q[j].z; b = s.q[j].w; } else { a = s.m[j].x; b = s.m[j].y; }
            c[4 * j + 0] = ((a & 0x8000u) << 16) | (a & 0x7fffu);
            c[4 * j + 1] = (a & 0x80000000u) | ((a >> 16) & 0x7fffu);
            c[4 * j + 2] = ((b & 0x8000u) << 16) | (b & 0x7fffu);
            c[4 * j + 3] = (b & 0x80000000u) | ((b >> 16) & 0x7fffu);
        }
    } else {
#pragma unroll
        for (int j = 0; j < kSliceSteps; ++j) { c[4 * j + 0] = s.m[j].x; c[4 * j + 1] = s.m[j].y; c[4 * j + 2] = s.m[j].z; c[4 * j + 3] = s.m[j].w; }
    }
}

}  // namespace

}  // namespace hispmv
