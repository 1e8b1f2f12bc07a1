// hispmv_spmm_bf16.hip -- the kernels of the wide-batch product with bf16 activations (hispmv_spmm_bf16.h): hispmv_spmm.hip with 2-byte
// xt and yt.  The sixth satellite on hispmv_slice_walk.h; hispmv_spmm.hip and hispmv_kernels.hip are not touched from here.
//
// What is kept from hispmv_spmm.hip: grid, groups and walk; the element-serial multiply with fp32 accumulators, unfused; the branch-free
// masked gather and the +-0 skip rule; the fp32 workspace of open and head partials; the fix-up launch as the only writer of a cut row.
// What differs:
//   a lane owns VB = 8, 4, 2 or 1 bf16 of a row of xt: one dwordx4, dwordx2, dword or 16-bit load per stored element.  The keep-mask is
//   applied to the packed dwords, then the halves are widened exactly (bits << 16, bits & 0xffff0000): a skipped element adds +0.
//   a finished row is alpha * acc + beta * bias in fp32 -- store_row's expression, the bias widened -- and is then rounded ONCE to bf16
//   (nearest, ties to even: round_bits_to_bf16 of hispmv_format.h in its device form, as in hispmv_update.hip).
//   a handle of several parts keeps the row in an fp32 tile accumulator [rows, 64 * VB] between the parts; only the last part rounds.
// The value before the rounding has the fixed order of adds of the fp32 entry: it is bit for bit what hispmv_spmm_device stores for the
// widened operands, whatever the batch, the tile or VB.
#include <hip/hip_runtime.h>

#include "hispmv_slice_walk.h"
#include "hispmv_spmm_bf16.h"

namespace hispmv {

namespace {

// round_bits_to_bf16 (hispmv_format.h) on the device, -> the 16 bits: nearest, ties to even; +-Inf stay; a finite value above the largest
// bf16 becomes Inf; a NaN keeps its sign and upper payload and gets the quiet bit.  The hardware pack-convert is not used.
__device__ __forceinline__ unsigned bf16_of(float f) {
    const unsigned u = (unsigned)f2i(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x0040u;
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// the VB bf16 of a lane as packed dwords: element 2d in the low half of dword d, 2d + 1 in the high half (VB 1: the low half of d[0])
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

// A finished row, in the slice kernel and in the fix-up alike: alpha * acc + beta * bias in fp32 (store_row of hispmv_spmm.hip), then
// either kept in fp32 in the tile accumulator (a part that is not the last) or rounded once and stored to yt.  A lane stores only its
// vectors below n_vecs -- element by element where its VB vectors straddle n_vecs: the pad elements n_vecs .. ld_y - 1 of a row are never
// written -- and reads the bias of exactly the elements it writes, so a matrix bias may be yt.
template <int VB>
__device__ __forceinline__ void store_row_bf16(const SpmmBf16Operands& a, int row, int lane, int lane_vec, const float (&acc)[VB]) {
    const int live = a.n_vecs - lane_vec;
    if (live <= 0) return;
    float* const accp = a.acc + ((size_t)row * 64 + lane) * VB;      // (formed, not used, when there is no accumulator)
    float out[VB];
    if (a.beta != 0.0f) {
        float b[VB];
        if (a.bias_kind == kBf16BiasShared) {
            const float s = ((const HISPMV_GLOBAL float*)a.bias)[row];
#pragma unroll
            for (int i = 0; i < VB; ++i) b[i] = s;
        } else if (a.bias_kind == kBf16BiasAcc) {
            load_f32<VB>(accp, b);
        } else {
            const uint16_t* const bp = (const uint16_t*)a.bias + (size_t)row * (size_t)a.ld_y + lane_vec;
            if (live >= VB) {
                unsigned d[kPacked<VB>];
                load_packed<VB>(bp, d);
                widen<VB>(d, b);
            } else {
#pragma unroll
                for (int i = 0; i < VB; ++i) b[i] = i < live ? i2f((int)((unsigned)((const HISPMV_GLOBAL uint16_t*)bp)[i] << 16)) : 0.0f;
            }
        }
#pragma unroll
        for (int i = 0; i < VB; ++i) out[i] = a.alpha * acc[i] + a.beta * b[i];
    } else {
#pragma unroll
        for (int i = 0; i < VB; ++i) out[i] = a.alpha * acc[i];
    }
    if (a.to_acc) {
        store_f32<VB>(accp, out);
        return;
    }
    uint16_t* const yp = a.yt + (size_t)row * (size_t)a.ld_y + lane_vec;
    if (live >= VB) {
        unsigned d[kPacked<VB>];
        if constexpr (VB == 1) {
            d[0] = bf16_of(out[0]);
        } else {
#pragma unroll
            for (int i = 0; i < VB / 2; ++i) d[i] = bf16_of(out[2 * i]) | (bf16_of(out[2 * i + 1]) << 16);
        }
        store_packed<VB>(yp, d);
    } else {
#pragma unroll
        for (int i = 0; i < VB; ++i)
            if (i < live) ((HISPMV_GLOBAL uint16_t*)yp)[i] = (uint16_t)bf16_of(out[i]);
    }
}

// spmm_group of hispmv_spmm.hip for lanes of VB bf16.  LDS: the forward launch's window of lds_floats words, holding column numbers.
// work: [n_slices][64 * VB] fp32 partial sums of the slices' open last rows, then [n_slices][64 * VB] raw sums of first rows that
// continue a chain.
template <int VB, bool USE_LDS, bool COMPACT, bool STRAYS, bool HALF>
__device__ __forceinline__ void spmm_bf16_group(
    const char* __restrict__ stream, const int4* __restrict__ hdr, const int4* __restrict__ frags, const SpmmBf16Operands& a,
    long long n_slices, int group_slices, int lds_floats, int cols, int rows, long long group, int4 g) {
    extern __shared__ unsigned colwin[];
    constexpr int kE = kSliceSteps * kLaneElems;
    constexpr int NP = kPacked<VB>;
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6), n_waves = (int)(blockDim.x >> 6);
    auto wk = GroupWalk<USE_LDS, COMPACT, STRAYS, HALF>::at(stream, n_slices, group_slices, lds_floats, group, g, wave, n_waves);
    const bool strays = wk.strays;
    unsigned* const stray_area = colwin + wk.win_floats + wave * kStraySlots;
    const unsigned* const stray_cols = (const unsigned*)(hdr + n_slices);

    SliceRaw<COMPACT, HALF> w;
    int4 h = int4{0, 0, 0, 0};
    if (wk.live()) {
        h = load_int4(hdr + wk.cur());
        request_slice<COMPACT, HALF>(w, wk.slice(), lane);
    }
    if (USE_LDS) fill_column_window(colwin, frags, g, wk.in_lds, lds_floats, wk.win_floats, lane, wave, n_waves);

    // a lane past the batch gathers the halves of lane 0 (always inside the row) and stores nothing
    const int lane_vec = a.tile0 + lane * VB;
    const uint16_t* const xlane = a.xt + a.tile0 + (lane_vec < a.n_vecs ? lane * VB : 0);
    float* const open_w = a.work;
    float* const head_w = a.work + (size_t)n_slices * (64 * VB);

    while (wk.live()) {
        const int row_first = __builtin_amdgcn_readfirstlane(h.x);      // first row that ends in this slice
        const int chain_len = __builtin_amdgcn_readfirstlane(h.y);      // > 0: that row began chain_len slices earlier (a row of the fix tables)
        const long long cur = wk.cur();
        unsigned c[kE];
        float v[kE];
        decode_metas<COMPACT, HALF>(w, c);
        slice_values<COMPACT, HALF>(w, v);
        if (STRAYS && strays) {
            stray_area[lane] = ((const HISPMV_GLOBAL unsigned*)stray_cols)[cur * kStraySlots + lane];
            __builtin_amdgcn_wave_barrier();
        }
        unsigned meta[kE];
        resolve_columns<USE_LDS, COMPACT, STRAYS>(c, meta, colwin, stray_area, wk.in_lds, strays, wk.win_floats, lds_floats,
                                                  [&](unsigned col, int i) { return col < (unsigned)cols && (f2i(v[i]) & 0x7fffffff) != 0; });
        wk.advance();
        if (wk.live()) {
            h = load_int4(hdr + wk.cur());
            request_slice<COMPACT, HALF>(w, wk.slice(), lane);
        }

        // the 1024 elements in stream order: step j, lane L, element k, value and meta wave-uniform (readlane); every lane gathers its VB
        // halves of that column's row of xt.  No branch per gather: an element that is not multiplied reads row 0 and its packed dwords are
        // masked to zero before they are widened, so it adds s * +0.
        float acc[VB];
#pragma unroll
        for (int i = 0; i < VB; ++i) acc[i] = 0.0f;
        int r = 0;                                   // row ends passed in this slice
        // A gather group is G elements of one lane step.  VB <= 2: the four elements of a step, two groups in flight, as fp32 VL <= 2.
        // VB 4 and 8: two elements (the packed dwords of four did not fit 128 VGPRs beside the unpacked halves: scratch) -- VB 4 with two
        // groups in flight, VB 8 with one.
        constexpr int G = VB >= 4 ? 2 : kLaneElems;
        constexpr std::integral_constant<int, 0> first{};
        constexpr std::integral_constant<int, kLaneElems - G> second{};      // (G = 4: the one group of a lane step once more, never asked for)
        struct Gathered { unsigned m[G]; float s[G]; unsigned x[G][NP]; };
        const auto gather = [&](Gathered& q, int j, int L, auto k0) {      // elements k0 .. k0 + G - 1 of lane L in step j
#pragma unroll
            for (int k = 0; k < G; ++k) {
                q.m[k] = (unsigned)__builtin_amdgcn_readlane((int)meta[4 * j + k0() + k], L);
                q.s[k] = i2f(__builtin_amdgcn_readlane(f2i(v[4 * j + k0() + k]), L));
                load_packed<VB>(xlane + (size_t)(q.m[k] < kSkipMeta ? q.m[k] >> 1 : 0u) * (size_t)a.ld_x, q.x[k]);
            }
        };
        const auto consume = [&](const Gathered& q) {
#pragma unroll
            for (int k = 0; k < G; ++k) {
                const unsigned keep = q.m[k] < kSkipMeta ? 0xffffffffu : 0u;
                unsigned d[NP];
#pragma unroll
                for (int i = 0; i < NP; ++i) d[i] = q.x[k][i] & keep;
                float x[VB];
                widen<VB>(d, x);
#pragma unroll
                for (int i = 0; i < VB; ++i) acc[i] += q.s[k] * x[i];
                if (q.m[k] & 1u) {                   // the row ends here (wave-uniform)
                    if (r == 0 && chain_len > 0) {
                        store_f32<VB>(head_w + ((size_t)cur * 64 + lane) * VB, acc);      // finished by the fix-up launch
                    } else if (row_first + r < rows) {
                        store_row_bf16<VB>(a, row_first + r, lane, lane_vec, acc);
                    }
#pragma unroll
                    for (int i = 0; i < VB; ++i) acc[i] = 0.0f;
                    r += 1;
                }
            }
        };
#pragma unroll
        for (int j = 0; j < kSliceSteps; ++j) {
            Gathered qa, qb;
            if constexpr (G == kLaneElems) {      // qa: an even lane's elements, qb: an odd lane's
                gather(qa, j, 0, first);
#pragma unroll 1
                for (int L = 0; L < 64; L += 2) {
                    gather(qb, j, L + 1, first);
                    consume(qa);
                    gather(qa, j, L + 2 < 64 ? L + 2 : 63, first);      // (behind lane 62 the elements of lane 63 once more: dropped)
                    consume(qb);
                }
            } else if constexpr (VB < 8) {        // qa: the first two elements of a lane, qb: its last two
                gather(qa, j, 0, first);
#pragma unroll 1
                for (int L = 0; L < 64; ++L) {
                    gather(qb, j, L, second);
                    consume(qa);
                    gather(qa, j, L + 1 < 64 ? L + 1 : 63, first);      // (behind lane 63 its first two once more: dropped)
                    consume(qb);
                }
            } else {
#pragma unroll 1
                for (int L = 0; L < 64; ++L) {
                    gather(qa, j, L, first);
                    consume(qa);
                    gather(qa, j, L, second);
                    consume(qa);
                }
            }
        }
        store_f32<VB>(open_w + ((size_t)cur * 64 + lane) * VB, acc);      // the open last row (zeros when the slice has none)
        if (STRAYS && strays) __builtin_amdgcn_wave_barrier();
    }
}

template <int VB, bool USE_LDS, bool STRAYS, bool HALF>
__global__ __launch_bounds__(1024) void spmm_bf16_slices_kernel(
    const char* __restrict__ words, const int4* __restrict__ hdr, const int4* __restrict__ groups, const int4* __restrict__ frags,
    SpmmBf16Operands a, long long n_slices, int group_slices, int lds_floats, int cols, int rows) {
    const long long group = (long long)blockIdx.x;
    if constexpr (USE_LDS) {
        const int4 g = load_int4(groups + group);
        const int gw = __builtin_amdgcn_readfirstlane(g.w);
        if constexpr (HALF) {
            if (gw & kGroupHalf) {
                spmm_bf16_group<VB, true, true, STRAYS, true>(words, hdr, frags, a, n_slices, group_slices, lds_floats, cols, rows, group, g);
                return;
            }
        }
        if (gw & kGroupCompact)
            spmm_bf16_group<VB, true, true, STRAYS, false>(words, hdr, frags, a, n_slices, group_slices, lds_floats, cols, rows, group, g);
        else
            spmm_bf16_group<VB, true, false, false, false>(words, hdr, frags, a, n_slices, group_slices, lds_floats, cols, rows, group, g);
    } else {
        spmm_bf16_group<VB, false, false, false, false>(words, hdr, frags, a, n_slices, group_slices, lds_floats, cols, rows, group, int4{0, 0, 0, 0});
    }
}

// The cut rows: one wavefront per entry {row, first_slice, len} of the fix tables, lanes across vectors (spmm_fix_kernel of hispmv_spmm.hip).
template <int VB>
__global__ __launch_bounds__(256) void spmm_bf16_fix_kernel(const int4* __restrict__ fix_short, int n_short, const int4* __restrict__ fix_long, int n_long,
                                                           SpmmBf16Operands a, long long n_slices, int rows) {
    const int lane = (int)(threadIdx.x & 63);
    const long long id = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (id >= (long long)n_short + n_long) return;
    const int4 f = load_int4(id < n_short ? fix_short + id : fix_long + (id - n_short));
    const int row = __builtin_amdgcn_readfirstlane(f.x), first = __builtin_amdgcn_readfirstlane(f.y), len = __builtin_amdgcn_readfirstlane(f.z);
    if (row < 0 || row >= rows || first < 0 || len < 1 || (long long)first + len >= n_slices) return;
    const float* const open_w = a.work;
    const float* const head_w = a.work + (size_t)n_slices * (64 * VB);
    float acc[VB], p[VB];
#pragma unroll
    for (int i = 0; i < VB; ++i) acc[i] = 0.0f;
    for (int k = 0; k < len; ++k) {
        load_f32<VB>(open_w + ((size_t)(first + k) * 64 + lane) * VB, p);
#pragma unroll
        for (int i = 0; i < VB; ++i) acc[i] += p[i];
    }
    load_f32<VB>(head_w + ((size_t)(first + len) * 64 + lane) * VB, p);
#pragma unroll
    for (int i = 0; i < VB; ++i) acc[i] += p[i];
    store_row_bf16<VB>(a, row, lane, a.tile0 + lane * VB, acc);
}

// yt = bf16(beta * bias) for every vector of the call (alpha == 0); a thread per element, reading what it writes
__global__ __launch_bounds__(256) void spmm_bf16_bias_kernel(SpmmBf16Operands a, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long row = i / a.n_vecs, v = i % a.n_vecs;
    uint16_t* const yp = a.yt + row * a.ld_y + v;
    float out = 0.0f;
    if (a.beta != 0.0f) {
        const float b = a.bias_kind == kBf16BiasShared ? ((const float*)a.bias)[row] : i2f((int)((unsigned)((const uint16_t*)a.bias)[row * a.ld_y + v] << 16));
        out = a.beta * b;
    }
    *yp = (uint16_t)bf16_of(out);
}

template <int VB>
hipError_t launch_slices(const SpmvDeviceMatrix& m, const SpmmBf16Operands& a, hipStream_t stream) {
    return with_slice_flags(m, [&](auto USE_LDS, auto STRAYS, auto HALF) {
        constexpr auto kernel = spmm_bf16_slices_kernel<VB, USE_LDS(), STRAYS(), HALF()>;
        const hipError_t e = raise_lds_limit<kernel>();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kernel, dim3((unsigned)m.n_groups), dim3((unsigned)m.block_threads), (size_t)m.lds_floats * 4, stream, (const char*)m.words, m.hdr,
                           m.groups, m.frags, a, (long long)m.n_slices, m.group_slices, m.lds_floats, m.cols, m.rows);
        return hipGetLastError();
    });
}

template <int VB>
hipError_t launch_part(const SpmvDeviceMatrix& m, const SpmmBf16Operands& a, hipStream_t stream) {
    hipError_t e = launch_slices<VB>(m, a, stream);
    if (e != hipSuccess) return e;
    const long long n_fix = (long long)m.n_fix_short + m.n_fix_long;
    if (n_fix <= 0) return hipSuccess;
    hipLaunchKernelGGL(spmm_bf16_fix_kernel<VB>, dim3((unsigned)((n_fix + 3) / 4)), dim3(256), 0, stream, m.fix_short, (int)m.n_fix_short, m.fix_long, (int)m.n_fix_long,
                       a, (long long)m.n_slices, (int)m.rows);
    return hipGetLastError();
}

bool bias_ok(const SpmmBf16Operands& a) {
    if (a.beta == 0.0f) return true;
    if (a.bias_kind == kBf16BiasAcc) return a.acc != nullptr;
    return a.bias != nullptr && (a.bias_kind == kBf16BiasShared || a.bias_kind == kBf16BiasMatrix);
}

}  // namespace

hipError_t launch_spmm_bf16_part(const SpmvDeviceMatrix& m, int vb, const SpmmBf16Operands& a, hipStream_t stream) {
    (void)hipGetLastError();
    if (m.n_slices <= 0 || m.n_groups <= 0) return hipSuccess;
    if (!slice_geometry_ok(m, (size_t)m.lds_floats * 4)) return hipErrorInvalidValue;
    if (!a.xt || !a.yt || !a.work || a.n_vecs < 1 || a.tile0 < 0 || a.tile0 >= a.n_vecs || a.ld_x < a.n_vecs || a.ld_y < a.n_vecs) return hipErrorInvalidValue;
    if (!bias_ok(a) || (a.to_acc && !a.acc)) return hipErrorInvalidValue;
    switch (vb) {
        case 8: return launch_part<8>(m, a, stream);
        case 4: return launch_part<4>(m, a, stream);
        case 2: return launch_part<2>(m, a, stream);
        case 1: return launch_part<1>(m, a, stream);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_spmm_bf16_bias(const SpmmBf16Operands& a, int32_t rows, hipStream_t stream) {
    (void)hipGetLastError();
    if (rows <= 0 || a.n_vecs <= 0) return hipSuccess;
    if (!a.yt || a.ld_y < a.n_vecs || a.bias_kind == kBf16BiasAcc || !bias_ok(a)) return hipErrorInvalidValue;
    const long long total = (long long)rows * a.n_vecs;
    if (total >= (1LL << 39)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(spmm_bf16_bias_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, a, total);
    return hipGetLastError();
}

}  // namespace hispmv
