// hispmv_spmm.hip -- the kernels of the wide-batch product (hispmv_spmm.h): yt[rows, B] = alpha * A * xt[cols, B] + beta * bias on the
// slice stream of a loaded handle, operands feature-major.  Stands on its own like hispmv_transpose.hip: the few decode helpers of
// the slice format it needs (the slice request, decode_metas, the bf16 widening) are its own copies, so that hispmv_kernels.hip --
// and with it every forward kernel -- is untouched by this file.
//
// Roles, against the forward slice kernel (hispmv_kernels.hip: slices_group):
//   forward                                           wide batch
//   a lane owns 16 elements of the slice              a lane owns VL vectors; the wavefront walks the 1024 elements one after the other
//   x window of the group in the LDS (staged)         the same words hold the COLUMN NUMBER of each window slot (no global read)
//   stray area of a wavefront (x of <= 64 strays)     the columns of the slice's strays
//   segmented scan over the lanes                     none: a lane's sum of a row is sequential, in stream order
//   carry[slice] + fix-up launch (y += alpha * chain) work[slice] + fix-up launch that is the ONLY writer of a cut row
// Every yt element has one writer per launch and a fixed order of adds: its bits depend neither on the batch, nor on the tile or
// VL that carried it, nor on the run.  A stored slot whose value is +-0 contributes nothing, whatever xt holds.
#include <hip/hip_runtime.h>

#include <mutex>

#include "hispmv_format.h"
#include "hispmv_spmm.h"

namespace hispmv {

namespace {

#define HISPMV_M_GLOBAL __attribute__((address_space(1)))
__device__ __forceinline__ int f2i(float f) { return __builtin_bit_cast(int, f); }
__device__ __forceinline__ float i2f(int i) { return __builtin_bit_cast(float, i); }
__device__ __forceinline__ uint4 load_words(const uint4* p) {
    typedef unsigned int u4v __attribute__((ext_vector_type(4)));
    const u4v v = __builtin_nontemporal_load((const HISPMV_M_GLOBAL u4v*)p);
    return uint4{v.x, v.y, v.z, v.w};
}
__device__ __forceinline__ uint2 load_words2(const uint2* p) {
    typedef unsigned int u2v __attribute__((ext_vector_type(2)));
    const u2v v = __builtin_nontemporal_load((const HISPMV_M_GLOBAL u2v*)p);
    return uint2{v.x, v.y};
}
__device__ __forceinline__ int4 load_int4(const int4* p) {
    typedef int i4v __attribute__((ext_vector_type(4)));
    const i4v v = *(const HISPMV_M_GLOBAL i4v*)p;
    return int4{v.x, v.y, v.z, v.w};
}

// A slice as it arrives (hispmv_format.h; the forward kernel's SliceRaw): per step 4 values and 4 metas per lane, or -- HALF -- one
// 16-byte piece {v0 | v1 << 16, v2 | v3 << 16, m0 | m1 << 16, m2 | m3 << 16}.
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

// VL consecutive floats of a lane: one dword, dwordx2 or dwordx4 access (the tile rule makes the address a multiple of 4 * VL)
template <int VL> __device__ __forceinline__ void load_vl(const float* p, float (&x)[VL]) {
    if constexpr (VL == 4) {
        typedef float f4v __attribute__((ext_vector_type(4)));
        const f4v q = *(const HISPMV_M_GLOBAL f4v*)p;
        x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
    } else if constexpr (VL == 2) {
        typedef float f2v __attribute__((ext_vector_type(2)));
        const f2v q = *(const HISPMV_M_GLOBAL f2v*)p;
        x[0] = q.x; x[1] = q.y;
    } else {
        x[0] = *(const HISPMV_M_GLOBAL float*)p;
    }
}
template <int VL> __device__ __forceinline__ void store_vl(float* p, const float (&x)[VL]) {
    if constexpr (VL == 4) {
        typedef float f4v __attribute__((ext_vector_type(4)));
        *(HISPMV_M_GLOBAL f4v*)p = f4v{x[0], x[1], x[2], x[3]};
    } else if constexpr (VL == 2) {
        typedef float f2v __attribute__((ext_vector_type(2)));
        *(HISPMV_M_GLOBAL f2v*)p = f2v{x[0], x[1]};
    } else {
        *(HISPMV_M_GLOBAL float*)p = x[0];
    }
}

// yt[row, lane's vectors] = alpha * acc + beta * bias: the one expression every finished row goes through, in the slice kernel and in
// the fix-up alike.  A lane stores only its vectors below n_vecs (the pad floats n_vecs .. ld_y - 1 of a row are never written); it
// reads the bias of exactly the floats it writes, so bias may be yt.
template <int VL>
__device__ __forceinline__ void store_row(const SpmmOperands& a, int row, int lane_vec, const float (&acc)[VL]) {
    const int live = a.n_vecs - lane_vec;
    if (live <= 0) return;
    float* const yp = a.yt + (size_t)row * (size_t)a.ld_y + lane_vec;
    float out[VL];
    if (a.beta != 0.0f) {
        float b[VL];
        if (a.bias_stride == 0) {
            const float s = ((const HISPMV_M_GLOBAL float*)a.bias)[row];
#pragma unroll
            for (int i = 0; i < VL; ++i) b[i] = s;
        } else {
            const float* const bp = a.bias + (size_t)row * (size_t)a.bias_stride + lane_vec;
            if (live >= VL) {
                load_vl<VL>(bp, b);
            } else {
#pragma unroll
                for (int i = 0; i < VL; ++i) b[i] = i < live ? ((const HISPMV_M_GLOBAL float*)bp)[i] : 0.0f;
            }
        }
#pragma unroll
        for (int i = 0; i < VL; ++i) out[i] = a.alpha * acc[i] + a.beta * b[i];
    } else {
#pragma unroll
        for (int i = 0; i < VL; ++i) out[i] = a.alpha * acc[i];
    }
    if (live >= VL) {
        store_vl<VL>(yp, out);
    } else {
#pragma unroll
        for (int i = 0; i < VL; ++i)
            if (i < live) ((HISPMV_M_GLOBAL float*)yp)[i] = out[i];
    }
}

constexpr unsigned kNoCol = 0xffffffffu;           // a window slot, stray slot or meta that names no column of xt
constexpr unsigned kSkipMeta = 0xfffffffeu;        // broadcast word of an element that is not multiplied: column << 1 | row end otherwise

// The work of one workgroup on group `group` of a slice stream, for a group stored COMPACT (6 B per element), HALF (4 B) or wide (8 B).
// LDS: the forward launch's window of lds_floats words (the wavefronts' stray areas are its last words), holding column numbers.
// work: [n_slices][64 * VL] partial sums of the slices' open last rows, then [n_slices][64 * VL] raw sums of first rows that continue
// a chain (written only by the slices whose header says so: exactly the rows of the fix tables).
template <int VL, bool USE_LDS, bool COMPACT, bool STRAYS, bool HALF>
__device__ __forceinline__ void spmm_group(
    const char* __restrict__ stream, const int4* __restrict__ hdr, const int4* __restrict__ frags, const SpmmOperands& a,
    long long n_slices, int group_slices, int lds_floats, int cols, int rows, long long group, int4 g) {
    extern __shared__ unsigned colwin[];
    constexpr int kE = kSliceSteps * kLaneElems;
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6), n_waves = (int)(blockDim.x >> 6);
    const long long first = group * group_slices;
    const long long last = (first + group_slices < n_slices) ? first + group_slices : n_slices;
    const int n_here = (int)(last > first ? last - first : 0);
    constexpr int slice_bytes = HALF ? kHalfSliceBytes : COMPACT ? kCompactSliceBytes : kWideSliceBytes;
    const char* const gbase = stream + (USE_LDS ? (size_t)(unsigned)__builtin_amdgcn_readfirstlane(g.z) * kSliceUnit : (size_t)first * kWideSliceBytes);
    const bool in_lds = USE_LDS && __builtin_amdgcn_readfirstlane(g.y) > 0;      // 0 fragments: the metas of this group are plain columns
    const bool strays = STRAYS && COMPACT && (__builtin_amdgcn_readfirstlane(g.w) & kGroupStrays) != 0;
    const int win_floats = lds_floats - (STRAYS ? n_waves * kStraySlots : 0);
    unsigned* const stray_area = colwin + win_floats + wave * kStraySlots;
    // the columns of every slice's strays live behind the headers (hispmv_abi.cpp), 64 per slice, 0xffffffff = none
    const unsigned* const stray_cols = (const unsigned*)(hdr + n_slices);

    // the forward kernel's walk (rotated start, a wavefront takes every n_waves-th slice); the first request leaves before the window is filled
    const int rot = n_here == 0 ? 0 : (int)((unsigned long long)group * 29ull % (unsigned)n_here);
    int k_slice = wave;
    int local = k_slice < n_here ? (k_slice + rot >= n_here ? k_slice + rot - n_here : k_slice + rot) : n_here;
    SliceRaw<COMPACT, HALF> w;
    int4 h = int4{0, 0, 0, 0};
    if (local < n_here) {
        h = load_int4(hdr + first + local);
        request_slice<COMPACT, HALF>(w, gbase + (size_t)local * slice_bytes, lane);
    }
    if (USE_LDS) {
        // the window in column numbers: for every fragment {col_start, len, lds_off}, col_start + i at lds_off + i; no column elsewhere
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

    // a lane past the batch gathers the floats of lane 0 (always inside the row) and stores nothing
    const int lane_vec = a.tile0 + lane * VL;
    const float* const xlane = a.xt + a.tile0 + (lane_vec < a.n_vecs ? lane * VL : 0);
    float* const open_w = a.work;
    float* const head_w = a.work + (size_t)n_slices * (64 * VL);

    while (local < n_here) {
        const int row_first = __builtin_amdgcn_readfirstlane(h.x);      // first row that ends in this slice
        const int chain_len = __builtin_amdgcn_readfirstlane(h.y);      // > 0: that row began chain_len slices earlier (a row of the fix tables)
        const long long cur = first + local;
        unsigned c[kE];
        float v[kE];
        decode_metas<COMPACT, HALF>(w, c);
        slice_values<COMPACT, HALF>(w, v);
        if (STRAYS && strays) {
            stray_area[lane] = ((const HISPMV_M_GLOBAL unsigned*)stray_cols)[cur * kStraySlots + lane];
            __builtin_amdgcn_wave_barrier();      // (LDS operations of one wavefront execute in order)
        }
        // every meta -> column << 1 | row end, or kSkipMeta | row end for a +-0 value or a column outside xt
        unsigned meta[kE];
#pragma unroll
        for (int i = 0; i < kE; ++i) {
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
            const bool live = col < (unsigned)cols && (f2i(v[i]) & 0x7fffffff) != 0;
            meta[i] = (live ? col << 1 : kSkipMeta) | end;
        }
        // the next slice of this wavefront, into the registers the copies above have left
        k_slice += n_waves;
        local = k_slice < n_here ? (k_slice + rot >= n_here ? k_slice + rot - n_here : k_slice + rot) : n_here;
        if (local < n_here) {
            h = load_int4(hdr + first + local);
            request_slice<COMPACT, HALF>(w, gbase + (size_t)local * slice_bytes, lane);
        }

        // the 1024 elements in stream order: step j, lane L, element k.  Value and meta of an element are wave-uniform (readlane);
        // every lane gathers its VL floats of that column's row of xt.  The gathers carry no branch: an element that is not
        // multiplied reads row 0 of xt and its floats are masked to +0, so -- VL 1 and 2 -- the four gathers of lane L + 1's elements leave
        // before the four of lane L are consumed (eight in flight per wavefront; with a branch per gather hipcc drained them four by four).
        float acc[VL];
#pragma unroll
        for (int i = 0; i < VL; ++i) acc[i] = 0.0f;
        int r = 0;                                   // row ends passed in this slice
        struct Gathered { unsigned m[kLaneElems]; unsigned keep[kLaneElems]; float s[kLaneElems]; float x[kLaneElems][VL]; };
        const auto gather = [&](Gathered& q, int j, int L) {
#pragma unroll
            for (int k = 0; k < kLaneElems; ++k) {
                q.m[k] = (unsigned)__builtin_amdgcn_readlane((int)meta[4 * j + k], L);
                q.s[k] = i2f(__builtin_amdgcn_readlane(f2i(v[4 * j + k]), L));
                const bool live = q.m[k] < kSkipMeta;
                q.keep[k] = live ? 0xffffffffu : 0u;
                load_vl<VL>(xlane + (size_t)(live ? q.m[k] >> 1 : 0u) * (size_t)a.ld_x, q.x[k]);
            }
        };
        const auto consume = [&](const Gathered& q) {
#pragma unroll
            for (int k = 0; k < kLaneElems; ++k) {
#pragma unroll
                for (int i = 0; i < VL; ++i) acc[i] += q.s[k] * i2f((int)((unsigned)f2i(q.x[k][i]) & q.keep[k]));
                if (q.m[k] & 1u) {                   // the row ends here (wave-uniform)
                    if (r == 0 && chain_len > 0) {
                        store_vl<VL>(head_w + ((size_t)cur * 64 + lane) * VL, acc);      // finished by the fix-up launch
                    } else if (row_first + r < rows) {
                        store_row<VL>(a, row_first + r, lane_vec, acc);
                    }
#pragma unroll
                    for (int i = 0; i < VL; ++i) acc[i] = 0.0f;
                    r += 1;
                }
            }
        };
#pragma unroll
        for (int j = 0; j < kSliceSteps; ++j) {
            if constexpr (VL < 4) {
                Gathered qa, qb;
                gather(qa, j, 0);
#pragma unroll 1
                for (int L = 0; L < 64; L += 2) {
                    gather(qb, j, L + 1);
                    consume(qa);
                    gather(qa, j, L + 2 < 64 ? L + 2 : 63);      // (behind lane 62 the elements of lane 63 once more: dropped)
                    consume(qb);
                }
            } else {      // 16 floats per lane and group: a second group in flight spills (128 VGPRs at 1024 threads); four 1-KiB gathers are in flight as it is
                Gathered q;
#pragma unroll 1
                for (int L = 0; L < 64; ++L) {
                    gather(q, j, L);
                    consume(q);
                }
            }
        }
        store_vl<VL>(open_w + ((size_t)cur * 64 + lane) * VL, acc);      // the open last row (zeros when the slice has none)
        if (STRAYS && strays) __builtin_amdgcn_wave_barrier();           // the stray area is read: the next slice may fill it
    }
}

// HALF: the handle stores bf16 values and has half groups; the group word of every group decides which body decodes it.
template <int VL, bool USE_LDS, bool STRAYS, bool HALF>
__global__ __launch_bounds__(1024) void spmm_slices_kernel(
    const char* __restrict__ words, const int4* __restrict__ hdr, const int4* __restrict__ groups, const int4* __restrict__ frags,
    SpmmOperands a, long long n_slices, int group_slices, int lds_floats, int cols, int rows) {
    const long long group = (long long)blockIdx.x;
    if constexpr (USE_LDS) {
        const int4 g = load_int4(groups + group);
        const int gw = __builtin_amdgcn_readfirstlane(g.w);
        if constexpr (HALF) {
            if (gw & kGroupHalf) {
                spmm_group<VL, true, true, STRAYS, true>(words, hdr, frags, a, n_slices, group_slices, lds_floats, cols, rows, group, g);
                return;
            }
        }
        if (gw & kGroupCompact)
            spmm_group<VL, true, true, STRAYS, false>(words, hdr, frags, a, n_slices, group_slices, lds_floats, cols, rows, group, g);
        else
            spmm_group<VL, true, false, false, false>(words, hdr, frags, a, n_slices, group_slices, lds_floats, cols, rows, group, g);
    } else {
        spmm_group<VL, false, false, false, false>(words, hdr, frags, a, n_slices, group_slices, lds_floats, cols, rows, group, int4{0, 0, 0, 0});
    }
}

// The cut rows: one wavefront per entry {row, first_slice, len} of the fix tables, lanes across vectors.  The row's sum is the open
// partials of slices first .. first + len - 1 in ascending order, then the raw first-row sum of slice first + len, where the row ends.
template <int VL>
__global__ __launch_bounds__(256) void spmm_fix_kernel(const int4* __restrict__ fix_short, int n_short, const int4* __restrict__ fix_long, int n_long,
                                                      SpmmOperands a, long long n_slices, int rows) {
    const int lane = (int)(threadIdx.x & 63);
    const long long id = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (id >= (long long)n_short + n_long) return;
    const int4 f = load_int4(id < n_short ? fix_short + id : fix_long + (id - n_short));
    const int row = __builtin_amdgcn_readfirstlane(f.x), first = __builtin_amdgcn_readfirstlane(f.y), len = __builtin_amdgcn_readfirstlane(f.z);
    if (row < 0 || row >= rows || first < 0 || len < 1 || (long long)first + len >= n_slices) return;
    const float* const open_w = a.work;
    const float* const head_w = a.work + (size_t)n_slices * (64 * VL);
    float acc[VL], p[VL];
#pragma unroll
    for (int i = 0; i < VL; ++i) acc[i] = 0.0f;
    for (int k = 0; k < len; ++k) {
        load_vl<VL>(open_w + ((size_t)(first + k) * 64 + lane) * VL, p);
#pragma unroll
        for (int i = 0; i < VL; ++i) acc[i] += p[i];
    }
    load_vl<VL>(head_w + ((size_t)(first + len) * 64 + lane) * VL, p);
#pragma unroll
    for (int i = 0; i < VL; ++i) acc[i] += p[i];
    store_row<VL>(a, row, a.tile0 + lane * VL, acc);
}

// yt = beta * bias for every vector of the call (alpha == 0); a thread per float, reading what it writes
__global__ __launch_bounds__(256) void spmm_bias_kernel(SpmmOperands a, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long row = i / a.n_vecs, v = i % a.n_vecs;
    float* const yp = a.yt + row * a.ld_y + v;
    *yp = a.beta != 0.0f ? a.beta * (a.bias_stride == 0 ? a.bias[row] : a.bias[row * a.bias_stride + v]) : 0.0f;
}

template <auto Kernel>
hipError_t raise_lds_limit() {
    static std::once_flag once;
    static hipError_t status = hipSuccess;
    std::call_once(once, [] { status = hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kDynLdsMax); });
    return status;
}

template <int VL>
hipError_t launch_slices(const SpmvDeviceMatrix& m, const SpmmOperands& a, hipStream_t stream) {
    const auto go = [&](auto kernel) {
        const hipError_t e = raise_lds_limit<kernel()>();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kernel(), dim3((unsigned)m.n_groups), dim3((unsigned)m.block_threads), (size_t)m.lds_floats * 4, stream, (const char*)m.words, m.hdr,
                           m.groups, m.frags, a, (long long)m.n_slices, m.group_slices, m.lds_floats, m.cols, m.rows);
        return hipGetLastError();
    };
#define HISPMV_M_KERNEL(L, S, H) go([] { return spmm_slices_kernel<VL, L, S, H>; })
    if (m.lds_floats <= 0) return HISPMV_M_KERNEL(false, false, false);
    if (m.has_strays) return m.has_half ? HISPMV_M_KERNEL(true, true, true) : HISPMV_M_KERNEL(true, true, false);
    return m.has_half ? HISPMV_M_KERNEL(true, false, true) : HISPMV_M_KERNEL(true, false, false);
#undef HISPMV_M_KERNEL
}

template <int VL>
hipError_t launch_part(const SpmvDeviceMatrix& m, const SpmmOperands& a, hipStream_t stream) {
    hipError_t e = launch_slices<VL>(m, a, stream);
    if (e != hipSuccess) return e;
    const long long n_fix = (long long)m.n_fix_short + m.n_fix_long;
    if (n_fix <= 0) return hipSuccess;
    hipLaunchKernelGGL(spmm_fix_kernel<VL>, dim3((unsigned)((n_fix + 3) / 4)), dim3(256), 0, stream, m.fix_short, (int)m.n_fix_short, m.fix_long, (int)m.n_fix_long, a,
                       (long long)m.n_slices, (int)m.rows);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_spmm_part(const SpmvDeviceMatrix& m, int vl, const SpmmOperands& a, hipStream_t stream) {
    (void)hipGetLastError();
    if (m.n_slices <= 0 || m.n_groups <= 0) return hipSuccess;
    if (m.n_groups > 0x7fffffffLL || m.block_threads < 64 || m.block_threads > 1024 || (m.block_threads & 63) || (size_t)m.lds_floats * 4 > (size_t)kDynLdsMax)
        return hipErrorInvalidValue;
    // stray slots and half groups exist only in plans with a window (hispmv_abi.cpp)
    if (m.lds_floats <= 0 && (m.has_strays || m.has_half)) return hipErrorInvalidValue;
    if (m.has_strays && m.lds_floats < (m.block_threads / 64) * kStraySlots) return hipErrorInvalidValue;
    if (!a.xt || !a.yt || !a.work || a.n_vecs < 1 || a.tile0 < 0 || a.tile0 >= a.n_vecs || a.ld_x < a.n_vecs || a.ld_y < a.n_vecs) return hipErrorInvalidValue;
    if (a.beta != 0.0f && (!a.bias || (a.bias_stride != 0 && a.bias_stride != a.ld_y))) return hipErrorInvalidValue;
    switch (vl) {
        case 4: return launch_part<4>(m, a, stream);
        case 2: return launch_part<2>(m, a, stream);
        case 1: return launch_part<1>(m, a, stream);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_spmm_bias(const SpmmOperands& a, int32_t rows, hipStream_t stream) {
    (void)hipGetLastError();
    if (rows <= 0 || a.n_vecs <= 0) return hipSuccess;
    if (!a.yt || a.ld_y < a.n_vecs || (a.beta != 0.0f && (!a.bias || (a.bias_stride != 0 && a.bias_stride != a.ld_y)))) return hipErrorInvalidValue;
    const long long total = (long long)rows * a.n_vecs;
    if (total >= (1LL << 39)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(spmm_bias_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, a, total);
    return hipGetLastError();
}

}  // namespace hispmv
