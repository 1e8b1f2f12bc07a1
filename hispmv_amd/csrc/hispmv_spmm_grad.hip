// hispmv_spmm_grad.hip -- the kernels of the wide-batch value gradient (hispmv_spmm_grad.h): grad[k] = alpha * sum_v gyt[row_k, v] *
// xt[col_k, v] + beta * grad[k] on the slice stream of a loaded, updatable handle, operands feature-major, fp32 or bf16: one text over
// the activation type T.  What it needs of the slice format (the meta request, decode_metas, store_grad, the launch checks) it shares
// with the other satellite files: hispmv_slice_walk.h; a lane's elements as they are loaded and widened: hispmv_wide_lanes.h; the sum
// over the lanes: hispmv_lane_tree.h.  hispmv_kernels.hip takes no part in that and keeps its own text, so that no forward kernel is
// touched from here.
//
// Roles, against the wide-batch product (hispmv_spmm.hip: spmm_group) and the value gradient of 4 vectors (hispmv_value_grad.hip):
//   wide-batch product                          value gradient (4-2-1)                     wide-batch value gradient
//   a lane owns V vectors                       a lane owns 16 elements of the slice       a lane owns V vectors
//   values and metas of a slice                 the metas only                             the metas only
//   window words hold COLUMN NUMBERS            x window staged per vector                 window words hold column numbers
//   a lane sums a row sequentially              16 products per lane, summed over vectors  V products per lane and element, then the sum
//                                                                                          over the 64 lanes: a butterfly over 64 elements
//   carry + fix-up launch for cut rows          none                                       none: every element is independent
// An explicit zero of the input has a map word like every other entry and gets its gradient; a slot whose map word is 0 (fillers,
// row extensions, padding) writes nothing.
// A lane owns V = 4, 2 or 1 floats, or 8, 4, 2 or 1 bf16, of a row: one dwordx4, dwordx2, dword or 16-bit load per element for xt and per
// row for gyt.  bf16: the gathered halves and the row of gyt requested one row end ahead stay PACKED (V / 2 dwords) until they are used;
// they are widened exactly (bits << 16, bits & 0xffff0000) in front of the products.
#include <hip/hip_runtime.h>

#include "hispmv_slice_walk.h"
#include "hispmv_wide_lanes.h"
#include "hispmv_lane_tree.h"
#include "hispmv_spmm_grad.h"
#include "hispmv_update.h"

namespace hispmv {

namespace {

// The work of one workgroup on group `group` of a slice stream, for a group stored COMPACT (6 B per element), HALF (4 B) or wide (8 B).
// LDS: the forward launch's window of lds_floats words (the wavefronts' stray areas are its last words), holding column numbers.
template <class T, int V, bool USE_LDS, bool COMPACT, bool STRAYS, bool HALF>
__device__ __forceinline__ void spmm_grad_group(
    const char* __restrict__ stream, const int4* __restrict__ hdr, const int4* __restrict__ frags, const int32_t* __restrict__ map,
    const SpmmGradOperandsOf<T>& a, long long n_slices, int group_slices, int lds_floats, int cols, int rows, long long group, int4 g) {
    extern __shared__ unsigned colwin[];
    constexpr int kE = kSliceSteps * kLaneElems;
    using Lanes = WideLanes<T, V>;
    using Word = typename Lanes::Word;      // a lane's V elements as loaded: NP floats, or NP packed dwords
    constexpr int NP = Lanes::NP;
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6), n_waves = (int)(blockDim.x >> 6);
    // the forward kernel's walk; the first request leaves before the window is filled
    auto wk = GroupWalk<USE_LDS, COMPACT, STRAYS, HALF>::at(stream, n_slices, group_slices, lds_floats, group, g, wave, n_waves);
    const bool strays = wk.strays;
    unsigned* const stray_area = colwin + wk.win_floats + wave * kStraySlots;
    // the columns of every slice's strays live behind the headers (hispmv_load.cpp: upload_slice_layout), 64 per slice, 0xffffffff = none
    const unsigned* const stray_cols = (const unsigned*)(hdr + n_slices);

    SliceMetas<COMPACT> w;
    int4 h = int4{0, 0, 0, 0};
    if (wk.live()) {
        h = load_int4(hdr + wk.cur());
        request_metas<COMPACT, HALF>(w, wk.slice(), lane);
    }
    if (USE_LDS) fill_column_window(colwin, frags, g, wk.in_lds, lds_floats, wk.win_floats, lane, wave, n_waves);

    // A lane past the batch reads the elements of lane 0 (always inside the row).  keep[i]: the lane's vector i is below n_vecs; the
    // PRODUCT of every other one is masked to +0, so that neither a pad element of gyt nor one of xt (NaN, say) gets into a sum.
    const int lane_vec = a.tile0 + lane * V;
    const unsigned lane_bytes = lane_vec < a.n_vecs ? (unsigned)(lane * V * sizeof(T)) : 0u;      // (a uniform row address + these 32 bits: one scalar-base load)
    const T* const xtile = a.xt + a.tile0;
    const T* const gtile = a.gyt + a.tile0;
    bool keep[V];
#pragma unroll
    for (int i = 0; i < V; ++i) keep[i] = lane_vec + i < a.n_vecs;
    // gyt[row, the lane's vectors], as loaded; a row past the matrix (elements of padding behind the last row) reads row 0: its map word is 0
    const auto load_gy = [&](Word (&d)[NP], int row) {
        const int rc = (row >= 0 && row < rows) ? row : 0;
        Lanes::load((const T*)((const char*)(gtile + (size_t)rc * (size_t)a.ld_gy) + lane_bytes), d);
    };

    while (wk.live()) {
        // the row of the slice's first element, even when that row began slices earlier; an element's row is this plus the row ends
        // passed so far in the slice, in stream order (the decode of value_grad_group)
        int row = __builtin_amdgcn_readfirstlane(h.x);
        const long long cur = wk.cur();
        float gy[V];                    // of `row`, widened
        Word gy_next[NP];               // of row + 1, requested one row end ahead, as loaded until it becomes gy
        {
            Word d[NP];
            load_gy(d, row);
            Lanes::widen(d, gy);
        }
        load_gy(gy_next, row + 1);
        unsigned c[kE];
        decode_metas<COMPACT>(w, c);
        if (STRAYS && strays) {
            stray_area[lane] = ((const HISPMV_GLOBAL unsigned*)stray_cols)[cur * kStraySlots + lane];
            __builtin_amdgcn_wave_barrier();      // (LDS operations of one wavefront execute in order)
        }
        // every meta -> column << 1 | row end, or kSkipMeta | row end for a column outside xt (padding, fillers, kNoCol)
        unsigned meta[kE];
        resolve_columns<USE_LDS, COMPACT, STRAYS>(c, meta, colwin, stray_area, wk.in_lds, strays, wk.win_floats, lds_floats,
                                                  [&](unsigned col, int) { return col < (unsigned)cols; });

        // the 1024 elements in stream order: step j, lane L, element k.  The meta of an element is wave-uniform (readlane); every lane
        // gathers its V elements of that column's row of xt.  The gathers carry no branch: an element without a column reads row 0 of
        // xt (its sum is dropped at the store: its map word is 0).
        // NK elements per gather: the four of a lane, or -- 16 bytes per lane and element: VL 4, VB 8 -- its two halves one after the other
        constexpr int NK = Lanes::kWholeLoad ? kLaneElems / 2 : kLaneElems;
        struct Gathered { unsigned m[NK]; Word x[NK][NP]; };
        const auto gather = [&](Gathered& q, int j, int L, int k0) {
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                q.m[k] = (unsigned)__builtin_amdgcn_readlane((int)meta[4 * j + k0 + k], L);
                Lanes::load((const T*)((const char*)(xtile + (size_t)(q.m[k] < kSkipMeta ? q.m[k] >> 1 : 0u) * (size_t)a.ld_x) + lane_bytes), q.x[k]);
            }
        };
        // -> the lane's partial of each of the four elements; behind a row end (wave-uniform) gyt of the next row
        const auto consume = [&](const Gathered& q, float (&p)[kLaneElems], int k0) {
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                float x[V];
                Lanes::widen(q.x[k], x);
                float s = 0.0f;
#pragma unroll
                for (int i = 0; i < V; ++i) s = s + (keep[i] ? gy[i] * x[i] : 0.0f);
                asm volatile("" : "+v"(s));      // the sum is formed HERE: left alone, hipcc sinks the products below the row-end branches and keeps every gathered element live
                p[k0 + k] = s;
                if (q.m[k] & 1u) {
                    row += 1;
                    Lanes::widen(gy_next, gy);
                    load_gy(gy_next, row + 1);
                }
            }
        };
        const int4* const mp = (const int4*)(map + (size_t)cur * kValueChunk) + lane;
#pragma unroll
        for (int j = 0; j < kSliceSteps; ++j) {
            // (slots and totals begin defined: read-before-write cannot be ruled out at compile time, and an undefined slot would be
            //  live around the whole slice loop -- 20 registers through the decode)
            Counter cnt[kLaneElems] = {};
            float total[kLaneElems] = {0.0f, 0.0f, 0.0f, 0.0f};
            float pa[kLaneElems], pb[kLaneElems];
            if (j == kSliceSteps - 1) {
                // the next slice of this wavefront, requested a quarter of a slice ahead: by now the metas of the first three steps are
                // dead, so the request costs no register at the peak (the 256 elements of this step hide it)
                wk.advance();
                if (wk.live()) {
                    h = load_int4(hdr + wk.cur());
                    request_metas<COMPACT, HALF>(w, wk.slice(), lane);
                }
            }
            if constexpr (NK == kLaneElems) {
                Gathered qa, qb;
                gather(qa, j, 0, 0);
#pragma unroll 1
                for (int P = 0; P < 32; ++P) {
                    gather(qb, j, 2 * P + 1, 0);
                    consume(qa, pa, 0);
                    gather(qa, j, P < 31 ? 2 * P + 2 : 63, 0);      // (behind lane 62 the elements of lane 63 once more: dropped)
                    consume(qb, pb, 0);
#pragma unroll
                    for (int k = 0; k < kLaneElems; ++k) total[k] = counter_push(cnt[k], merge<0>(pa[k], pb[k], lane), P, lane);
                }
            } else {      // the same in halves of a lane's elements: two gathers of two 16-byte elements in flight
                Gathered qa, qb;
                gather(qa, j, 0, 0);
#pragma unroll 1
                for (int P = 0; P < 32; ++P) {
                    gather(qb, j, 2 * P, 2);
                    consume(qa, pa, 0);
                    gather(qa, j, 2 * P + 1, 0);
                    consume(qb, pa, 2);
                    gather(qb, j, 2 * P + 1, 2);
                    consume(qa, pb, 0);
                    gather(qa, j, P < 31 ? 2 * P + 2 : 63, 0);      // (behind lane 63 its first two elements once more: dropped)
                    consume(qb, pb, 2);
#pragma unroll
                    for (int k = 0; k < kLaneElems; ++k) total[k] = counter_push(cnt[k], merge<0>(pa[k], pb[k], lane), P, lane);
                }
            }
            // lane L holds the totals of its own elements (j, L, 0 .. 3): the four map words of slot j * 64 + L, loaded only now
            const int4 q = load_int4(mp + j * 64);
            store_grad(a.grad, a.n, q.x, total[0], a.alpha, a.beta);
            store_grad(a.grad, a.n, q.y, total[1], a.alpha, a.beta);
            store_grad(a.grad, a.n, q.z, total[2], a.alpha, a.beta);
            store_grad(a.grad, a.n, q.w, total[3], a.alpha, a.beta);
        }
        if (STRAYS && strays) __builtin_amdgcn_wave_barrier();           // the stray area is read: the next slice may fill it
    }
}

// HALF: the handle stores bf16 values and has half groups; the group word of every group decides which body decodes it.
template <class T, int V, bool USE_LDS, bool STRAYS, bool HALF>
__global__ __launch_bounds__(1024) void spmm_grad_slices_kernel(
    const char* __restrict__ words, const int4* __restrict__ hdr, const int4* __restrict__ groups, const int4* __restrict__ frags,
    const int32_t* __restrict__ map, SpmmGradOperandsOf<T> a, long long n_slices, int group_slices, int lds_floats, int cols, int rows) {
    const long long group = (long long)blockIdx.x;
    if constexpr (USE_LDS) {
        const int4 g = load_int4(groups + group);
        const int gw = __builtin_amdgcn_readfirstlane(g.w);
        if constexpr (HALF) {
            if (gw & kGroupHalf) {
                spmm_grad_group<T, V, true, true, STRAYS, true>(words, hdr, frags, map, a, n_slices, group_slices, lds_floats, cols, rows, group, g);
                return;
            }
        }
        if (gw & kGroupCompact)
            spmm_grad_group<T, V, true, true, STRAYS, false>(words, hdr, frags, map, a, n_slices, group_slices, lds_floats, cols, rows, group, g);
        else
            spmm_grad_group<T, V, true, false, false, false>(words, hdr, frags, map, a, n_slices, group_slices, lds_floats, cols, rows, group, g);
    } else {
        spmm_grad_group<T, V, false, false, false, false>(words, hdr, frags, map, a, n_slices, group_slices, lds_floats, cols, rows, group, int4{0, 0, 0, 0});
    }
}

template <class T, int V>
hipError_t launch_slices(const SpmvDeviceMatrix& m, const int32_t* map, const SpmmGradOperandsOf<T>& a, hipStream_t stream) {
    return with_slice_flags(m, [&](auto USE_LDS, auto STRAYS, auto HALF) {
        constexpr auto kernel = spmm_grad_slices_kernel<T, V, USE_LDS(), STRAYS(), HALF()>;
        const hipError_t e = raise_lds_limit<kernel>();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kernel, dim3((unsigned)m.n_groups), dim3((unsigned)m.block_threads), (size_t)m.lds_floats * 4, stream, (const char*)m.words, m.hdr,
                           m.groups, m.frags, map, a, (long long)m.n_slices, m.group_slices, m.lds_floats, m.cols, m.rows);
        return hipGetLastError();
    });
}

// The checks of either entry, then the kernel of lanes of v elements of T.
template <class T>
hipError_t launch_part(const SpmvDeviceMatrix& m, int v, const int32_t* map, const SpmmGradOperandsOf<T>& a, hipStream_t stream) {
    (void)hipGetLastError();
    if (m.n_slices <= 0 || m.n_groups <= 0 || a.n <= 0) return hipSuccess;
    if (!map) return hipErrorInvalidValue;
    if (!slice_geometry_ok(m, (size_t)m.lds_floats * 4)) return hipErrorInvalidValue;
    if (m.rows <= 0 || m.cols <= 0) return hipErrorInvalidValue;          // (rows 0 and columns 0 of gyt and xt are read for elements without a place)
    if (!a.gyt || !a.xt || !a.grad || a.n_vecs < 1 || a.tile0 < 0 || a.tile0 >= a.n_vecs || a.ld_x < a.n_vecs || a.ld_gy < a.n_vecs) return hipErrorInvalidValue;
    if (v != 1 && v != 2 && v != 4 && (v != 8 || sizeof(T) != 2)) return hipErrorInvalidValue;
    // A lane's v elements are one aligned load that ends inside the row: the tile rule's (c), checked where the loads are issued.  It
    // refuses no call of the C ABI, fp32 or bf16: v comes from that rule with these leading dimensions and the smaller alignment of
    // the two addresses, and tile0 is a sum of earlier tiles of 64 * v' vectors with v' a multiple of v ((a) only narrows as the batch runs out).
    if (a.tile0 % v || a.ld_x % v || a.ld_gy % v || ((uintptr_t)a.gyt | (uintptr_t)a.xt) % (uintptr_t)(sizeof(T) * v)) return hipErrorInvalidValue;
    switch (v) {
        case 4: return launch_slices<T, 4>(m, map, a, stream);
        case 2: return launch_slices<T, 2>(m, map, a, stream);
        case 1: return launch_slices<T, 1>(m, map, a, stream);
        default:
            if constexpr (sizeof(T) == 2) return launch_slices<T, 8>(m, map, a, stream);
            return hipErrorInvalidValue;
    }
}

}  // namespace

hipError_t launch_spmm_grad_part(const SpmvDeviceMatrix& m, int vl, const int32_t* map, const SpmmGradOperands& a, hipStream_t stream) {
    return launch_part<float>(m, vl, map, a, stream);
}
hipError_t launch_spmm_grad_bf16_part(const SpmvDeviceMatrix& m, int vb, const int32_t* map, const SpmmGradBf16Operands& a, hipStream_t stream) {
    return launch_part<uint16_t>(m, vb, map, a, stream);
}

}  // namespace hispmv
