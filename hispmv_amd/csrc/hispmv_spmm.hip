// hispmv_spmm.hip -- the kernels of the wide-batch product (hispmv_spmm.h): yt[rows, B] = alpha * A * xt[cols, B] + beta * bias on the
// slice stream of a loaded handle, operands feature-major, xt and yt fp32 or bf16: one text over the activation type.  What it needs of
// the slice format (the slice request, decode_metas, the bf16 widening, the launch checks) it shares with the other four satellite
// files: hispmv_slice_walk.h; the gather and multiply of one element, which is what differs between the types: hispmv_wide_lanes.h.
// hispmv_kernels.hip takes no part in that and keeps its own text, so that no forward kernel is touched from here.
//
// Roles, against the forward slice kernel (hispmv_kernels.hip: slices_group):
//   forward                                           wide batch
//   a lane owns 16 elements of the slice              a lane owns V vectors; the wavefront walks the 1024 elements one after the other
//   x window of the group in the LDS (staged)         the same words hold the COLUMN NUMBER of each window slot (no global read)
//   stray area of a wavefront (x of <= 64 strays)     the columns of the slice's strays
//   segmented scan over the lanes                     none: a lane's sum of a row is sequential, in stream order
//   carry[slice] + fix-up launch (y += alpha * chain) work[slice] + fix-up launch that is the ONLY writer of a cut row
// Every yt element has one writer per launch and a fixed order of adds: its bits depend neither on the batch, nor on the tile or
// V that carried it, nor on the run.  A stored slot whose value is +-0 contributes nothing, whatever xt holds.
// bf16 activations: a lane owns VB = 8, 4, 2 or 1 bf16 of a row of xt; the multiply stays element-serial with fp32 accumulators, unfused,
// and the workspace of open and head partials stays fp32.  A finished row is alpha * acc + beta * bias in fp32 -- the fp32 expression,
// the bias widened -- and is then rounded ONCE to bf16 (bf16_of).  A handle of several parts keeps the row in an fp32 tile accumulator
// [rows, 64 * VB] between the parts; only the last part rounds.  So the value before the rounding is bit for bit what the fp32 entry
// stores for the widened operands, whatever the batch, the tile or VB.
#include <hip/hip_runtime.h>

#include "hispmv_slice_walk.h"
#include "hispmv_wide_lanes.h"
#include "hispmv_spmm.h"

namespace hispmv {

namespace {

// yt[row, lane's vectors] = alpha * acc + beta * bias: the one expression every finished row goes through, in the slice kernel and in
// the fix-up alike.  A lane stores only its vectors below n_vecs (the pad floats n_vecs .. ld_y - 1 of a row are never written); it
// reads the bias of exactly the floats it writes, so bias may be yt.
template <int VL>
__device__ __forceinline__ void store_row(const SpmmOperands& a, int row, int /*lane*/, int lane_vec, const float (&acc)[VL]) {
    const int live = a.n_vecs - lane_vec;
    if (live <= 0) return;
    float* const yp = a.yt + (size_t)row * (size_t)a.ld_y + lane_vec;
    float out[VL];
    if (a.beta != 0.0f) {
        float b[VL];
        if (a.bias_stride == 0) {
            const float s = ((const HISPMV_GLOBAL float*)a.bias)[row];
#pragma unroll
            for (int i = 0; i < VL; ++i) b[i] = s;
        } else {
            const float* const bp = a.bias + (size_t)row * (size_t)a.bias_stride + lane_vec;
            if (live >= VL) {
                load_vl<VL>(bp, b);
            } else {
#pragma unroll
                for (int i = 0; i < VL; ++i) b[i] = i < live ? ((const HISPMV_GLOBAL float*)bp)[i] : 0.0f;
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
            if (i < live) ((HISPMV_GLOBAL float*)yp)[i] = out[i];
    }
}

// The same for bf16 yt: alpha * acc + beta * bias in fp32 as above, then either kept in fp32 in the tile accumulator (a part that is not
// the last) or rounded once and stored to yt.  A lane stores only its vectors below n_vecs -- element by element where its VB vectors
// straddle n_vecs: the pad elements n_vecs .. ld_y - 1 of a row are never written -- and reads the bias of exactly the elements it
// writes, so a matrix bias may be yt.
template <int VB>
__device__ __forceinline__ void store_row(const SpmmBf16Operands& a, int row, int lane, int lane_vec, const float (&acc)[VB]) {
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

// The work of one workgroup on group `group` of a slice stream, for a group stored COMPACT (6 B per element), HALF (4 B) or wide (8 B).
// A: SpmmOperands or SpmmBf16Operands; a lane owns V elements of A::Elem.
// LDS: the forward launch's window of lds_floats words (the wavefronts' stray areas are its last words), holding column numbers.
// work: [n_slices][64 * V] fp32 partial sums of the slices' open last rows, then [n_slices][64 * V] raw sums of first rows that continue
// a chain (written only by the slices whose header says so: exactly the rows of the fix tables).
template <class A, int V, bool USE_LDS, bool COMPACT, bool STRAYS, bool HALF>
__device__ __forceinline__ void spmm_group(
    const char* __restrict__ stream, const int4* __restrict__ hdr, const int4* __restrict__ frags, const A& a,
    long long n_slices, int group_slices, int lds_floats, int cols, int rows, long long group, int4 g) {
    extern __shared__ unsigned colwin[];
    constexpr int kE = kSliceSteps * kLaneElems;
    using T = typename A::Elem;
    using Lanes = WideLanes<T, V>;
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6), n_waves = (int)(blockDim.x >> 6);
    // the forward kernel's walk; the first request leaves before the window is filled
    auto wk = GroupWalk<USE_LDS, COMPACT, STRAYS, HALF>::at(stream, n_slices, group_slices, lds_floats, group, g, wave, n_waves);
    const bool strays = wk.strays;
    unsigned* const stray_area = colwin + wk.win_floats + wave * kStraySlots;
    // the columns of every slice's strays live behind the headers (hispmv_load.cpp: upload_slice_layout), 64 per slice, 0xffffffff = none
    const unsigned* const stray_cols = (const unsigned*)(hdr + n_slices);

    SliceRaw<COMPACT, HALF> w;
    int4 h = int4{0, 0, 0, 0};
    if (wk.live()) {
        h = load_int4(hdr + wk.cur());
        request_slice<COMPACT, HALF>(w, wk.slice(), lane);
    }
    if (USE_LDS) fill_column_window(colwin, frags, g, wk.in_lds, lds_floats, wk.win_floats, lane, wave, n_waves);

    // a lane past the batch gathers the elements of lane 0 (always inside the row) and stores nothing
    const int lane_vec = a.tile0 + lane * V;
    const T* const xlane = a.xt + a.tile0 + (lane_vec < a.n_vecs ? lane * V : 0);
    float* const open_w = a.work;
    float* const head_w = a.work + (size_t)n_slices * (64 * V);

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
            __builtin_amdgcn_wave_barrier();      // (LDS operations of one wavefront execute in order)
        }
        // every meta -> column << 1 | row end, or kSkipMeta | row end for a +-0 value or a column outside xt
        unsigned meta[kE];
        resolve_columns<USE_LDS, COMPACT, STRAYS>(c, meta, colwin, stray_area, wk.in_lds, strays, wk.win_floats, lds_floats,
                                                  [&](unsigned col, int i) { return col < (unsigned)cols && (f2i(v[i]) & 0x7fffffff) != 0; });
        // the next slice of this wavefront, into the registers the copies above have left
        wk.advance();
        if (wk.live()) {
            h = load_int4(hdr + wk.cur());
            request_slice<COMPACT, HALF>(w, wk.slice(), lane);
        }

        // the 1024 elements in stream order: step j, lane L, element k.  Value and meta of an element are wave-uniform (readlane);
        // every lane gathers its V elements of that column's row of xt.  The gathers carry no branch (Lanes::fetch): an element that is
        // not multiplied reads row 0 of xt and is masked to +0, so -- two groups in flight -- the gathers of the next group leave before
        // those of this one are consumed (eight in flight per wavefront at VL 1 and 2; with a branch per gather hipcc drained them four by four).
        float acc[V];
#pragma unroll
        for (int i = 0; i < V; ++i) acc[i] = 0.0f;
        int r = 0;                                   // row ends passed in this slice
        // A gather group is G elements of one lane step: all four, or its first and its second two (Lanes::G, and why).
        constexpr int G = Lanes::G;
        constexpr std::integral_constant<int, 0> first{};
        constexpr std::integral_constant<int, kLaneElems - G> second{};      // (G = 4: the one group of a lane step once more, never asked for)
        using Gathered = typename Lanes::Gathered;
        const auto gather = [&](Gathered& q, int j, int L, auto k0) {      // elements k0 .. k0 + G - 1 of lane L in step j
#pragma unroll
            for (int k = 0; k < G; ++k)
                Lanes::fetch(q, k, (unsigned)__builtin_amdgcn_readlane((int)meta[4 * j + k0() + k], L), i2f(__builtin_amdgcn_readlane(f2i(v[4 * j + k0() + k]), L)), xlane,
                             a.ld_x);
        };
        const auto consume = [&](const Gathered& q) {
#pragma unroll
            for (int k = 0; k < G; ++k) {
                Lanes::add(q, k, acc);
                if (q.m[k] & 1u) {                   // the row ends here (wave-uniform)
                    if (r == 0 && chain_len > 0) {
                        Lanes::store_work(head_w + ((size_t)cur * 64 + lane) * V, acc);      // finished by the fix-up launch
                    } else if (row_first + r < rows) {
                        store_row<V>(a, row_first + r, lane, lane_vec, acc);
                    }
#pragma unroll
                    for (int i = 0; i < V; ++i) acc[i] = 0.0f;
                    r += 1;
                }
            }
        };
#pragma unroll
        for (int j = 0; j < kSliceSteps; ++j) {
            Gathered qa, qb;
            if constexpr (G == kLaneElems && Lanes::kTwoInFlight) {      // qa: an even lane's elements, qb: an odd lane's
                gather(qa, j, 0, first);
#pragma unroll 1
                for (int L = 0; L < 64; L += 2) {
                    gather(qb, j, L + 1, first);
                    consume(qa);
                    gather(qa, j, L + 2 < 64 ? L + 2 : 63, first);      // (behind lane 62 the elements of lane 63 once more: dropped)
                    consume(qb);
                }
            } else if constexpr (G == kLaneElems) {      // one group in flight
#pragma unroll 1
                for (int L = 0; L < 64; ++L) {
                    gather(qa, j, L, first);
                    consume(qa);
                }
            } else if constexpr (Lanes::kTwoInFlight) {      // qa: the first two elements of a lane, qb: its last two
                gather(qa, j, 0, first);
#pragma unroll 1
                for (int L = 0; L < 64; ++L) {
                    gather(qb, j, L, second);
                    consume(qa);
                    gather(qa, j, L + 1 < 64 ? L + 1 : 63, first);      // (behind lane 63 its first two once more: dropped)
                    consume(qb);
                }
            } else {                                         // the two halves of a lane one after the other
#pragma unroll 1
                for (int L = 0; L < 64; ++L) {
                    gather(qa, j, L, first);
                    consume(qa);
                    gather(qa, j, L, second);
                    consume(qa);
                }
            }
        }
        Lanes::store_work(open_w + ((size_t)cur * 64 + lane) * V, acc);      // the open last row (zeros when the slice has none)
        if (STRAYS && strays) __builtin_amdgcn_wave_barrier();           // the stray area is read: the next slice may fill it
    }
}

// HALF: the handle stores bf16 values and has half groups; the group word of every group decides which body decodes it.
template <class A, int V, bool USE_LDS, bool STRAYS, bool HALF>
__global__ __launch_bounds__(1024) void spmm_slices_kernel(
    const char* __restrict__ words, const int4* __restrict__ hdr, const int4* __restrict__ groups, const int4* __restrict__ frags,
    A a, long long n_slices, int group_slices, int lds_floats, int cols, int rows) {
    const long long group = (long long)blockIdx.x;
    if constexpr (USE_LDS) {
        const int4 g = load_int4(groups + group);
        const int gw = __builtin_amdgcn_readfirstlane(g.w);
        if constexpr (HALF) {
            if (gw & kGroupHalf) {
                spmm_group<A, V, true, true, STRAYS, true>(words, hdr, frags, a, n_slices, group_slices, lds_floats, cols, rows, group, g);
                return;
            }
        }
        if (gw & kGroupCompact)
            spmm_group<A, V, true, true, STRAYS, false>(words, hdr, frags, a, n_slices, group_slices, lds_floats, cols, rows, group, g);
        else
            spmm_group<A, V, true, false, false, false>(words, hdr, frags, a, n_slices, group_slices, lds_floats, cols, rows, group, g);
    } else {
        spmm_group<A, V, false, false, false, false>(words, hdr, frags, a, n_slices, group_slices, lds_floats, cols, rows, group, int4{0, 0, 0, 0});
    }
}

// The cut rows: one wavefront per entry {row, first_slice, len} of the fix tables, lanes across vectors.  The row's sum is the open
// partials of slices first .. first + len - 1 in ascending order, then the raw first-row sum of slice first + len, where the row ends.
template <class A, int V>
__global__ __launch_bounds__(256) void spmm_fix_kernel(const int4* __restrict__ fix_short, int n_short, const int4* __restrict__ fix_long, int n_long,
                                                      A a, long long n_slices, int rows) {
    using Lanes = WideLanes<typename A::Elem, V>;
    const int lane = (int)(threadIdx.x & 63);
    const long long id = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (id >= (long long)n_short + n_long) return;
    const int4 f = load_int4(id < n_short ? fix_short + id : fix_long + (id - n_short));
    const int row = __builtin_amdgcn_readfirstlane(f.x), first = __builtin_amdgcn_readfirstlane(f.y), len = __builtin_amdgcn_readfirstlane(f.z);
    if (row < 0 || row >= rows || first < 0 || len < 1 || (long long)first + len >= n_slices) return;
    const float* const open_w = a.work;
    const float* const head_w = a.work + (size_t)n_slices * (64 * V);
    float acc[V], p[V];
#pragma unroll
    for (int i = 0; i < V; ++i) acc[i] = 0.0f;
    for (int k = 0; k < len; ++k) {
        Lanes::load_work(open_w + ((size_t)(first + k) * 64 + lane) * V, p);
#pragma unroll
        for (int i = 0; i < V; ++i) acc[i] += p[i];
    }
    Lanes::load_work(head_w + ((size_t)(first + len) * 64 + lane) * V, p);
#pragma unroll
    for (int i = 0; i < V; ++i) acc[i] += p[i];
    store_row<V>(a, row, lane, a.tile0 + lane * V, acc);
}

// yt = beta * bias for every vector of the call (alpha == 0); a thread per float, reading what it writes
__global__ __launch_bounds__(256) void spmm_bias_kernel(SpmmOperands a, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long row = i / a.n_vecs, v = i % a.n_vecs;
    float* const yp = a.yt + row * a.ld_y + v;
    *yp = a.beta != 0.0f ? a.beta * (a.bias_stride == 0 ? a.bias[row] : a.bias[row * a.bias_stride + v]) : 0.0f;
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

template <class A, int V>
hipError_t launch_slices(const SpmvDeviceMatrix& m, const A& a, hipStream_t stream) {
    return with_slice_flags(m, [&](auto USE_LDS, auto STRAYS, auto HALF) {
        constexpr auto kernel = spmm_slices_kernel<A, V, USE_LDS(), STRAYS(), HALF()>;
        const hipError_t e = raise_lds_limit<kernel>();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kernel, dim3((unsigned)m.n_groups), dim3((unsigned)m.block_threads), (size_t)m.lds_floats * 4, stream, (const char*)m.words, m.hdr,
                           m.groups, m.frags, a, (long long)m.n_slices, m.group_slices, m.lds_floats, m.cols, m.rows);
        return hipGetLastError();
    });
}

template <class A, int V>
hipError_t launch_tile(const SpmvDeviceMatrix& m, const A& a, hipStream_t stream) {
    hipError_t e = launch_slices<A, V>(m, a, stream);
    if (e != hipSuccess) return e;
    const long long n_fix = (long long)m.n_fix_short + m.n_fix_long;
    if (n_fix <= 0) return hipSuccess;
    hipLaunchKernelGGL((spmm_fix_kernel<A, V>), dim3((unsigned)((n_fix + 3) / 4)), dim3(256), 0, stream, m.fix_short, (int)m.n_fix_short, m.fix_long, (int)m.n_fix_long, a,
                       (long long)m.n_slices, (int)m.rows);
    return hipGetLastError();
}

// What both entries check (each adds its bias rules), then the kernels of lanes of v elements.
template <class A>
hipError_t launch_part(const SpmvDeviceMatrix& m, int v, const A& a, bool bias_ok, hipStream_t stream) {
    (void)hipGetLastError();
    if (m.n_slices <= 0 || m.n_groups <= 0) return hipSuccess;
    if (!slice_geometry_ok(m, (size_t)m.lds_floats * 4)) return hipErrorInvalidValue;
    if (!a.xt || !a.yt || !a.work || a.n_vecs < 1 || a.tile0 < 0 || a.tile0 >= a.n_vecs || a.ld_x < a.n_vecs || a.ld_y < a.n_vecs) return hipErrorInvalidValue;
    if (!bias_ok) return hipErrorInvalidValue;
    switch (v) {
        case 4: return launch_tile<A, 4>(m, a, stream);
        case 2: return launch_tile<A, 2>(m, a, stream);
        case 1: return launch_tile<A, 1>(m, a, stream);
        case 8:
            if constexpr (sizeof(typename A::Elem) == 2) return launch_tile<A, 8>(m, a, stream);
            [[fallthrough]];
        default: return hipErrorInvalidValue;
    }
}

bool bias_ok(const SpmmOperands& a) { return a.beta == 0.0f || (a.bias && (a.bias_stride == 0 || a.bias_stride == a.ld_y)); }
bool bias_ok(const SpmmBf16Operands& a) {
    if (a.beta == 0.0f) return true;
    if (a.bias_kind == kBf16BiasAcc) return a.acc != nullptr;
    return a.bias != nullptr && (a.bias_kind == kBf16BiasShared || a.bias_kind == kBf16BiasMatrix);
}

}  // namespace

hipError_t launch_spmm_part(const SpmvDeviceMatrix& m, int vl, const SpmmOperands& a, hipStream_t stream) { return launch_part(m, vl, a, bias_ok(a), stream); }
hipError_t launch_spmm_bf16_part(const SpmvDeviceMatrix& m, int vb, const SpmmBf16Operands& a, hipStream_t stream) {
    return launch_part(m, vb, a, bias_ok(a) && (!a.to_acc || a.acc), stream);
}

hipError_t launch_spmm_bias(const SpmmOperands& a, int32_t rows, hipStream_t stream) {
    (void)hipGetLastError();
    if (rows <= 0 || a.n_vecs <= 0) return hipSuccess;
    if (!a.yt || a.ld_y < a.n_vecs || !bias_ok(a)) return hipErrorInvalidValue;
    const long long total = (long long)rows * a.n_vecs;
    if (total >= (1LL << 39)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(spmm_bias_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, a, total);
    return hipGetLastError();
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
