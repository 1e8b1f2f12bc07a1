// hispmv_wide_lanes.h -- a lane of the wide-batch kernels over the activation type: what hispmv_spmm.hip (the product) and
// hispmv_spmm_grad.hip (the value gradient) need to be written once for fp32 and for bf16 xt, yt and gyt.  A lane owns V consecutive
// vectors of a row: V = 4, 2 or 1 floats, or 8, 4, 2 or 1 bf16 -- 16 bytes at the most, one load per row.  Here: the packed bf16 of a lane
// and their exact widening, the one rounding back, the fp32 workspace access of a bf16 tile, and WideLanes<T, V>, which gives each of the
// two kernels the few lines that differ between the types.  Device code only, in an unnamed namespace like hispmv_slice_walk.h, which it
// sits on; hispmv_kernels.hip includes neither.
#pragma once
#include <hip/hip_runtime.h>

#include "hispmv_slice_walk.h"

namespace hispmv {

namespace {

// ---- bf16 lanes -------------------------------------------------------------------------------------------------------------------
// round_bits_to_bf16 (hispmv_format.h) on the device, -> the 16 bits: nearest, ties to even; +-Inf stay; a finite value above the largest
// bf16 becomes Inf; a NaN keeps its sign and upper payload and gets the quiet bit.  The hardware pack-convert is not used.
__device__ __forceinline__ unsigned bf16_of(float f) {
    const unsigned u = (unsigned)f2i(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x0040u;
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// the VB bf16 of a lane as packed dwords: element 2d in the low half of dword d, 2d + 1 in the high half (VB 1: the low half of d[0]);
// one dwordx4, dwordx2, dword or 16-bit access (the tile rule makes the address a multiple of 2 * VB)
template <int VB> constexpr int kPacked = VB >= 2 ? VB / 2 : 1;
template <int VB> __device__ __forceinline__ void load_packed(const uint16_t* p, unsigned (&d)[kPacked<VB>]) {
    if constexpr (VB == 8) {
        typedef unsigned u4v __attribute__((ext_vector_type(4)));
        const u4v q = *(const HISPMV_GLOBAL u4v*)p;
        d[0] = q.x; d[1] = q.y; d[2] = q.z; d[3] = q.w;
    } else if constexpr (VB == 4) {
        typedef unsigned u2v __attribute__((ext_vector_type(2)));
        const u2v q = *(const HISPMV_GLOBAL u2v*)p;
        d[0] = q.x; d[1] = q.y;
    } else if constexpr (VB == 2) {
        d[0] = *(const HISPMV_GLOBAL unsigned*)p;
    } else {
        d[0] = *(const HISPMV_GLOBAL uint16_t*)p;
    }
}
template <int VB> __device__ __forceinline__ void store_packed(uint16_t* p, const unsigned (&d)[kPacked<VB>]) {
    if constexpr (VB == 8) {
        typedef unsigned u4v __attribute__((ext_vector_type(4)));
        *(HISPMV_GLOBAL u4v*)p = u4v{d[0], d[1], d[2], d[3]};
    } else if constexpr (VB == 4) {
        typedef unsigned u2v __attribute__((ext_vector_type(2)));
        *(HISPMV_GLOBAL u2v*)p = u2v{d[0], d[1]};
    } else if constexpr (VB == 2) {
        *(HISPMV_GLOBAL unsigned*)p = d[0];
    } else {
        *(HISPMV_GLOBAL uint16_t*)p = (uint16_t)d[0];
    }
}
// exact: a bf16 is the upper half of its fp32
template <int VB> __device__ __forceinline__ void widen(const unsigned (&d)[kPacked<VB>], float (&x)[VB]) {
    if constexpr (VB == 1) {
        x[0] = i2f((int)(d[0] << 16));
    } else {
#pragma unroll
        for (int i = 0; i < VB / 2; ++i) {
            x[2 * i] = i2f((int)(d[i] << 16));
            x[2 * i + 1] = i2f((int)(d[i] & 0xffff0000u));
        }
    }
}
// VB consecutive floats of the workspace: two accesses of VB / 2 floats each, since the tile rule aligns the workspace to 2 * VB bytes only
template <int VB> __device__ __forceinline__ void load_f32(const float* p, float (&x)[VB]) {
    if constexpr (VB == 1) {
        load_vl<1>(p, x);
    } else {
        float lo[VB / 2], hi[VB / 2];
        load_vl<VB / 2>(p, lo);
        load_vl<VB / 2>(p + VB / 2, hi);
#pragma unroll
        for (int i = 0; i < VB / 2; ++i) { x[i] = lo[i]; x[VB / 2 + i] = hi[i]; }
    }
}
template <int VB> __device__ __forceinline__ void store_f32(float* p, const float (&x)[VB]) {
    if constexpr (VB == 1) {
        store_vl<1>(p, x);
    } else {
        float lo[VB / 2], hi[VB / 2];
#pragma unroll
        for (int i = 0; i < VB / 2; ++i) { lo[i] = x[i]; hi[i] = x[VB / 2 + i]; }
        store_vl<VB / 2>(p, lo);
        store_vl<VB / 2>(p + VB / 2, hi);
    }
}

// ---- a lane of V elements of type T -----------------------------------------------------------------------------------------------
// For the gradient: a lane's V elements as they are loaded (Word[NP]: the floats, or the packed dwords), `load`, and `widen` to floats
// (a copy for fp32).  kWholeLoad: the V elements are 16 bytes, the widest load there is; both kernels then halve what is in flight.
// For the product: a gather group -- Gathered, G elements of a lane step, with `fetch` and `add` of its element k -- and the fp32
// workspace access of the lane's V partial sums.  kTwoInFlight: two gather groups fit the 128 VGPRs of a 1024-thread workgroup.
// Where a member is an existing function it is NAMED (static constexpr auto), not wrapped: store_work as a forceinline function around
// store_f32 reordered the instructions of the bf16 VB 4 and VB 8 slice kernels.
template <class T, int V> struct WideLanes;

template <int V> struct WideLanes<float, V> {
    static_assert(V == 4 || V == 2 || V == 1, "a lane owns 4, 2 or 1 floats");
    static constexpr bool kWholeLoad = V * sizeof(float) == 16;
    using Word = float;
    static constexpr int NP = V;
    static constexpr auto load = load_vl<V>;
    static __device__ __forceinline__ void widen(const float (&d)[V], float (&x)[V]) {
#pragma unroll
        for (int i = 0; i < V; ++i) x[i] = d[i];
    }

    // The four elements of a lane step.  VL 4, 16 floats per lane and group: a second group in flight spills (128 VGPRs at 1024 threads);
    // four 1-KiB gathers are in flight as it is.
    static constexpr int G = kLaneElems;
    static constexpr bool kTwoInFlight = !kWholeLoad;
    struct Gathered { unsigned m[G]; unsigned keep[G]; float s[G]; float x[G][V]; };
    // element k of the group: broadcast word m, value s, the lane's floats of row m >> 1 of xt.  No branch: an element that is not
    // multiplied reads row 0 and its floats are masked to +0.  The mask is formed HERE, where the gather is issued, and carried: formed
    // at the multiply it moved the VL 1 and VL 2 kernels.
    static __device__ __forceinline__ void fetch(Gathered& q, int k, unsigned m, float s, const float* xlane, long long ld_x) {
        q.m[k] = m;
        q.s[k] = s;
        const bool live = m < kSkipMeta;
        q.keep[k] = live ? 0xffffffffu : 0u;
        load_vl<V>(xlane + (size_t)(live ? m >> 1 : 0u) * (size_t)ld_x, q.x[k]);
    }
    static __device__ __forceinline__ void add(const Gathered& q, int k, float (&acc)[V]) {
#pragma unroll
        for (int i = 0; i < V; ++i) acc[i] += q.s[k] * i2f((int)((unsigned)f2i(q.x[k][i]) & q.keep[k]));
    }
    static constexpr auto load_work = load_vl<V>;
    static constexpr auto store_work = store_vl<V>;
};

template <int V> struct WideLanes<uint16_t, V> {
    static_assert(V == 8 || V == 4 || V == 2 || V == 1, "a lane owns 8, 4, 2 or 1 bf16");
    static constexpr bool kWholeLoad = V * sizeof(uint16_t) == 16;
    // the elements stay PACKED (V / 2 dwords) until they are used and are widened in front of the products
    using Word = unsigned;
    static constexpr int NP = kPacked<V>;
    static constexpr auto load = load_packed<V>;
    static constexpr auto widen = hispmv::widen<V>;

    // VB <= 2: the four elements of a lane step, two groups in flight, as fp32 VL <= 2.  VB 4 and 8: two elements (the packed dwords of
    // four did not fit 128 VGPRs beside the unpacked halves: scratch) -- VB 4 with two groups in flight, VB 8 with one.
    static constexpr int G = V >= 4 ? 2 : kLaneElems;
    static constexpr bool kTwoInFlight = !kWholeLoad;
    struct Gathered { unsigned m[G]; float s[G]; unsigned x[G][NP]; };
    // as for fp32, but the keep-mask is formed at the multiply and applied to the packed dwords before they are widened: a skipped
    // element adds s * +0
    static __device__ __forceinline__ void fetch(Gathered& q, int k, unsigned m, float s, const uint16_t* xlane, long long ld_x) {
        q.m[k] = m;
        q.s[k] = s;
        load_packed<V>(xlane + (size_t)(m < kSkipMeta ? m >> 1 : 0u) * (size_t)ld_x, q.x[k]);
    }
    static __device__ __forceinline__ void add(const Gathered& q, int k, float (&acc)[V]) {
        const unsigned keep = q.m[k] < kSkipMeta ? 0xffffffffu : 0u;
        unsigned d[NP];
#pragma unroll
        for (int i = 0; i < NP; ++i) d[i] = q.x[k][i] & keep;
        float x[V];
        hispmv::widen<V>(d, x);
#pragma unroll
        for (int i = 0; i < V; ++i) acc[i] += q.s[k] * x[i];
    }
    static constexpr auto load_work = load_f32<V>;
    static constexpr auto store_work = store_f32<V>;
};

}  // namespace

}  // namespace hispmv
