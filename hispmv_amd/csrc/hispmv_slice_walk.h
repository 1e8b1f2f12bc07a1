// hispmv_slice_walk.h -- what the satellite kernel files share: hispmv_transpose.hip, hispmv_value_grad.hip, hispmv_tts_transpose.hip,
// hispmv_spmm.hip and hispmv_spmm_grad.hip (the last two through hispmv_wide_lanes.h as well, which sits on this file), and nobody else.
// The buffer and vector-width helpers, the metas of a slice alone and the satellites' slice_values, the walk of a wavefront over the
// slices of its group (GroupWalk, local_rows, the column-number window), and the few host helpers of their launches (the LDS limit, the
// geometry checks, the (USE_LDS, STRAYS, HALF) choice).  (What stays written out in the five files, and why: DESIGN.md 2.14.)
//
// The slice format's decode itself -- the bit casts, the stream loads, SliceRaw, request_slice, decode_metas -- is hispmv_slice_decode.h's,
// which hispmv_kernels.hip includes as well: one text for all six kernel files.  hispmv_kernels.hip does NOT include this file: the walk
// and the bodies of the forward kernels stay written out there, and nothing in here may move a forward kernel's
// instructions.  Everything sits in an unnamed namespace: every including file gets its own copy, as it had when the text was written
// out in each of them.
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <type_traits>

#include "hispmv_format.h"
#include "hispmv_kernels.h"
#include "hispmv_slice_decode.h"

namespace hispmv {

namespace {

// ---- buffers and vector widths (the bit casts and the stream loads: hispmv_slice_decode.h) ---------------------------------------
// a dword through a buffer descriptor: an offset past the descriptor's bytes (kNoAccess among them) reads 0
constexpr unsigned kNoAccess = 0xffffffffu;
__device__ __forceinline__ float buffer_float(__amdgpu_buffer_rsrc_t r, unsigned byte_off) {
    return i2f((int)__builtin_amdgcn_raw_buffer_load_b32(r, byte_off, 0, 0));
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t float_buffer(const float* p, int n_floats) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)p, 0, n_floats * 4, 0x00020000);
}
// global_atomic_add_f32 without a return value
__device__ __forceinline__ void y_add(float* y, unsigned col, float v) { (void)atomicAdd(y + col, v); }

// VL consecutive floats of a lane: one dword, dwordx2 or dwordx4 access (the tile rule makes the address a multiple of 4 * VL)
template <int VL> __device__ __forceinline__ void load_vl(const float* p, float (&x)[VL]) {
    if constexpr (VL == 4) {
        typedef float f4v __attribute__((ext_vector_type(4)));
        const f4v q = *(const HISPMV_GLOBAL f4v*)p;
        x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
    } else if constexpr (VL == 2) {
        typedef float f2v __attribute__((ext_vector_type(2)));
        const f2v q = *(const HISPMV_GLOBAL f2v*)p;
        x[0] = q.x; x[1] = q.y;
    } else {
        x[0] = *(const HISPMV_GLOBAL float*)p;
    }
}
template <int VL> __device__ __forceinline__ void store_vl(float* p, const float (&x)[VL]) {
    if constexpr (VL == 4) {
        typedef float f4v __attribute__((ext_vector_type(4)));
        *(HISPMV_GLOBAL f4v*)p = f4v{x[0], x[1], x[2], x[3]};
    } else if constexpr (VL == 2) {
        typedef float f2v __attribute__((ext_vector_type(2)));
        *(HISPMV_GLOBAL f2v*)p = f2v{x[0], x[1]};
    } else {
        *(HISPMV_GLOBAL float*)p = x[0];
    }
}

// grad[q - 1] = alpha * s + beta * grad[q - 1] for a map word q that names an input entry; this lane is its only writer
__device__ __forceinline__ void store_grad(float* grad, long long n, int q, float s, float alpha, float beta) {
    if (q < 1 || (long long)q > n) return;
    float* const p = grad + (q - 1);
    float r = alpha * s;
    if (beta != 0.0f) r = r + beta * *p;
    *p = r;
}

// ---- the metas of a slice alone, and the values of a whole one (SliceRaw, request_slice: hispmv_slice_decode.h) --------------------
// SliceMetas: the metas alone (the gradients multiply no values).  They begin at byte 4096 of a compact (2 KiB) and of a wide (4 KiB)
// slice; the 4 KiB of values before them are not requested.  HALF (bf16 storage): the compact metas of step j, lane l are dwords 2 and 3
// of the 16-byte piece at (j * 64 + l) * 16; only those 8 bytes are requested, the bf16 values in dwords 0 and 1 are not.
template <bool COMPACT> struct SliceMetas;
template <> struct SliceMetas<true>  { uint2 m[kSliceSteps]; };
template <> struct SliceMetas<false> { uint4 m[kSliceSteps]; };
template <bool COMPACT, bool HALF = false>
__device__ __forceinline__ void request_metas(SliceMetas<COMPACT>& s, const char* base, int lane) {
    static_assert(COMPACT || !HALF, "only a compact group has a half form");
    if constexpr (HALF) {
        const uint2* pm = (const uint2*)(base + 8) + 2 * lane;
#pragma unroll
        for (int j = 0; j < kSliceSteps; ++j) s.m[j] = load_words2(pm + j * 128);
    } else if constexpr (COMPACT) {
        const uint2* pm = (const uint2*)(base + kSliceElems * 4) + lane;
#pragma unroll
        for (int j = 0; j < kSliceSteps; ++j) s.m[j] = load_words2(pm + j * 64);
    } else {
        const uint4* pm = (const uint4*)(base + kSliceElems * 4) + lane;
#pragma unroll
        for (int j = 0; j < kSliceSteps; ++j) s.m[j] = load_words(pm + j * 64);
    }
}
// the fp32 bits of the lane's 16 values: as stored, or the bf16 halves of a dword widened
template <bool COMPACT, bool HALF>
__device__ __forceinline__ void slice_values(const SliceRaw<COMPACT, HALF>& s, float (&v)[kSliceSteps * kLaneElems]) {
#pragma unroll
    for (int j = 0; j < kSliceSteps; ++j) {
        if constexpr (HALF) {
            v[4 * j + 0] = i2f((int)(s.q[j].x << 16)); v[4 * j + 1] = i2f((int)(s.q[j].x & 0xffff0000u));
            v[4 * j + 2] = i2f((int)(s.q[j].y << 16)); v[4 * j + 3] = i2f((int)(s.q[j].y & 0xffff0000u));
        } else {
            v[4 * j + 0] = i2f((int)s.v[j].x); v[4 * j + 1] = i2f((int)s.v[j].y); v[4 * j + 2] = i2f((int)s.v[j].z); v[4 * j + 3] = i2f((int)s.v[j].w);
        }
    }
}
// -> metas in wide form, as decode_metas(SliceRaw) of hispmv_slice_decode.h gives them for a whole slice: of its metas alone
template <bool COMPACT>
__device__ __forceinline__ void decode_metas(const SliceMetas<COMPACT>& s, unsigned (&c)[kSliceSteps * kLaneElems]) {
    if constexpr (COMPACT) {
#pragma unroll
        for (int j = 0; j < kSliceSteps; ++j) {
            const unsigned a = s.m[j].x, b = s.m[j].y;
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

// ---- the walk of a wavefront over the slices of its group -------------------------------------------------------------------------
// Group `group` of a slice stream holds slices first .. first + n_here - 1, stored COMPACT (6 B per element), HALF (4 B) or wide (8 B)
// from gbase on.  The forward kernel's walk: a rotated start, and wavefront `wave` of n_waves takes every n_waves-th slice; `local` is
// the one it is at.  win_floats: the window without the wavefronts' stray areas (its last floats in a plan with STRAYS); strays: THIS
// group uses them (bit 2 of its group word); in_lds: the group has fragments (0: its metas are plain columns).
template <bool USE_LDS, bool COMPACT, bool STRAYS, bool HALF>
struct GroupWalk {
    static constexpr int slice_bytes = HALF ? kHalfSliceBytes : COMPACT ? kCompactSliceBytes : kWideSliceBytes;
    long long first;
    int n_here;
    const char* gbase;
    bool in_lds, strays;
    int win_floats;
    int rot, n_waves, k_slice, local;

    // wavefront `wave` at its first slice of group `group`, whose group word is g (zeros in a plan without a window)
    static __device__ __forceinline__ GroupWalk at(const char* stream, long long n_slices, int group_slices, int lds_floats, long long group, int4 g, int wave, int n_waves) {
        const long long first = group * group_slices;
        const long long last = (first + group_slices < n_slices) ? first + group_slices : n_slices;
        const int n_here = (int)(last > first ? last - first : 0);
        const char* const gbase = stream + (USE_LDS ? (size_t)(unsigned)__builtin_amdgcn_readfirstlane(g.z) * kSliceUnit : (size_t)first * kWideSliceBytes);
        const bool in_lds = USE_LDS && __builtin_amdgcn_readfirstlane(g.y) > 0;
        const bool strays = STRAYS && COMPACT && (__builtin_amdgcn_readfirstlane(g.w) & kGroupStrays) != 0;
        const int win_floats = lds_floats - (STRAYS ? n_waves * kStraySlots : 0);
        const int rot = n_here == 0 ? 0 : (int)((unsigned long long)group * 29ull % (unsigned)n_here);
        GroupWalk w{first, n_here, gbase, in_lds, strays, win_floats, rot, n_waves, wave, 0};
        w.local = w.place();
        return w;
    }
    __device__ __forceinline__ int place() const { return k_slice < n_here ? (k_slice + rot >= n_here ? k_slice + rot - n_here : k_slice + rot) : n_here; }
    __device__ __forceinline__ bool live() const { return local < n_here; }
    __device__ __forceinline__ long long cur() const { return first + local; }                                   // the slice in the stream: its header, strays, map chunk
    __device__ __forceinline__ const char* slice() const { return gbase + (size_t)local * slice_bytes; }         // its bytes
    __device__ __forceinline__ void advance() { k_slice += n_waves; local = place(); }
};

// lr[4*j + k] = the local row of element k of the lane in step j = the row ends before it in the slice, from the row-end bits of the
// wide metas c (the forward kernel's ballots, plus the lane's own ends)
__device__ __forceinline__ void local_rows(const unsigned (&c)[kSliceSteps * kLaneElems], int (&lr)[kSliceSteps * kLaneElems]) {
    int row = 0;
#pragma unroll
    for (int j = 0; j < kSliceSteps; ++j) {
        int below = 0, total = 0;
#pragma unroll
        for (int k = 0; k < kLaneElems; ++k) {
            const unsigned long long m = __builtin_amdgcn_ballot_w64((c[4 * j + k] & kRowEndBit) != 0);
            below += lanes_below(m);
            total += __builtin_popcountll(m);
        }
        int r = row + below;
#pragma unroll
        for (int k = 0; k < kLaneElems; ++k) {
            lr[4 * j + k] = r;
            r += (c[4 * j + k] & kRowEndBit) ? 1 : 0;
        }
        row += total;
    }
}

// ---- the window of the wide-batch kernels holds column numbers --------------------------------------------------------------------
constexpr unsigned kNoCol = 0xffffffffu;           // a window slot, stray slot or meta that names no column of xt
constexpr unsigned kSkipMeta = 0xfffffffeu;        // broadcast word of an element that is not multiplied: column << 1 | row end otherwise

// the window in column numbers: for every fragment {col_start, len, lds_off} of the group, col_start + i at lds_off + i; no column elsewhere
__device__ __forceinline__ void fill_column_window(unsigned* colwin, const int4* frags, int4 g, bool in_lds, int lds_floats, int win_floats, int lane, int wave,
                                                   int n_waves) {
    for (int i = (int)threadIdx.x; i < lds_floats; i += (int)blockDim.x) colwin[i] = kNoCol;
    __syncthreads();
    const int f0 = __builtin_amdgcn_readfirstlane(g.x), nf = in_lds ? __builtin_amdgcn_readfirstlane(g.y) : 0;
    for (int f = wave; f < nf; f += n_waves) {
        const int4 fr = load_int4(frags + f0 + f);
        const int col0 = __builtin_amdgcn_readfirstlane(fr.x), len = __builtin_amdgcn_readfirstlane(fr.y), off = __builtin_amdgcn_readfirstlane(fr.z);
        for (int i = lane; i < len; i += 64)
            if (off + i >= 0 && off + i < win_floats) colwin[off + i] = (unsigned)(col0 + i);
    }
    __syncthreads();
}
// every wide meta c[i] -> meta[i] = column << 1 | row end, or kSkipMeta | row end for an element that is not `live(column, i)`: the column
// comes from the window, from the wavefront's stray area (filled with the slice's stray columns) or from the meta itself
template <bool USE_LDS, bool COMPACT, bool STRAYS, class Live>
__device__ __forceinline__ void resolve_columns(const unsigned (&c)[kSliceSteps * kLaneElems], unsigned (&meta)[kSliceSteps * kLaneElems], const unsigned* colwin,
                                                const unsigned* stray_area, bool in_lds, bool strays, int win_floats, int lds_floats, Live&& live) {
#pragma unroll
    for (int i = 0; i < kSliceSteps * kLaneElems; ++i) {
        const unsigned end = c[i] >> 31;
        unsigned col;
        if constexpr (COMPACT) {
            const int idx = (int)(c[i] & 0x7fffu);
            if (STRAYS && strays && idx >= win_floats) col = stray_area[(idx - win_floats) & (kStraySlots - 1)];
            else col = idx < lds_floats ? colwin[idx] : kNoCol;
        } else {
            const unsigned ci = c[i] & ~kRowEndBit;
            if (USE_LDS && in_lds && !(ci & kGlobalColBit)) col = ci < (unsigned)win_floats ? colwin[ci] : kNoCol;
            else col = ci & ~kGlobalColBit;
        }
        meta[i] = (live(col, i) ? col << 1 : kSkipMeta) | end;
    }
}

// ---- host: the launches -----------------------------------------------------------------------------------------------------------
// every kernel with dynamic LDS may take kDynLdsMax of it; asked for once per kernel
template <auto Kernel>
hipError_t raise_lds_limit() {
    static std::once_flag once;
    static hipError_t status = hipSuccess;
    std::call_once(once, [] { status = hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kDynLdsMax); });
    return status;
}

// What every slice launch checks of a plan before it starts a grid of m.n_groups workgroups with lds_bytes of dynamic LDS.
inline bool slice_geometry_ok(const SpmvDeviceMatrix& m, size_t lds_bytes) {
    if (m.n_groups > 0x7fffffffLL || m.block_threads < 64 || m.block_threads > 1024 || (m.block_threads & 63) || lds_bytes > (size_t)kDynLdsMax) return false;
    // stray slots and half groups exist only in plans with a window (hispmv_load.cpp)
    if (m.lds_floats <= 0 && (m.has_strays || m.has_half)) return false;
    return !m.has_strays || m.lds_floats >= (m.block_threads / 64) * kStraySlots;
}

// The plan's (USE_LDS, STRAYS, HALF) as template arguments: f(std::bool_constant<USE_LDS>{}, ...) for the five combinations that have a
// kernel -- without a window there are neither stray areas nor half groups (slice_geometry_ok).
template <class F>
hipError_t with_slice_flags(const SpmvDeviceMatrix& m, F&& f) {
    constexpr std::true_type yes{};
    constexpr std::false_type no{};
    if (m.lds_floats <= 0) return f(no, no, no);
    if (m.has_strays) return m.has_half ? f(yes, yes, yes) : f(yes, yes, no);
    return m.has_half ? f(yes, no, yes) : f(yes, no, no);
}

}  // namespace

}  // namespace hispmv
