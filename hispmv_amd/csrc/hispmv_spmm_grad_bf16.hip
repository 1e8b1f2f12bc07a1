// hispmv_spmm_grad_bf16.hip -- the kernels of the wide-batch value gradient with bf16 activations (hispmv_spmm_grad_bf16.h):
// spmm_grad_group of hispmv_spmm_grad.hip with 2-byte gyt and xt.  The seventh satellite on hispmv_slice_walk.h; the lane tree is the one
// of the fp32 kernel (hispmv_lane_tree.h).  No other kernel file is touched from here.
//
// What is kept from hispmv_spmm_grad.hip: grid, groups and walk; metas only, never values; column numbers in the LDS window; stray areas;
// in-bounds loads without a branch (row 0 or column 0 for an element without a place, lane 0's address for a lane past the batch); the
// PRODUCT mask; the asm volatile that forms the lane sum where it is written; the next-slice request before the last step; store_grad
// through the value map, plain stores, one writer per entry.
// What differs:
//   a lane owns VB = 8, 4, 2 or 1 bf16 of a row: one dwordx4, dwordx2, dword or 16-bit load per element for xt and per row for gyt.  The
//   gathered halves and the row of gyt requested one row end ahead stay PACKED (VB / 2 dwords) until they are used; they are widened
//   exactly (bits << 16, bits & 0xffff0000) in front of the products.
//   VB 8 gathers in halves of a lane's elements (two 16-byte elements per gather), as fp32 VL 4 does; VB <= 4 gathers all four.
// load_packed and widen are a second copy of those of hispmv_spmm_bf16.hip, which stays as it is: a shared header would have meant an
// edit of that file.
#include <hip/hip_runtime.h>

#include "hispmv_slice_walk.h"
#include "hispmv_lane_tree.h"
#include "hispmv_spmm_grad_bf16.h"
#include "hispmv_update.h"

namespace hispmv {

namespace {

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

// The work of one workgroup on group `group` of a slice stream, for a group stored COMPACT (6 B per element), HALF (4 B) or wide (8 B).
// LDS: the forward launch's window of lds_floats words (the wavefronts' stray areas are its last words), holding column numbers.
template <int VB, bool USE_LDS, bool COMPACT, bool STRAYS, bool HALF>
__device__ __forceinline__ void spmm_grad_bf16_group(
    const char* __restrict__ stream, const int4* __restrict__ hdr, const int4* __restrict__ frags, const int32_t* __restrict__ map,
    const SpmmGradBf16Operands& a, long long n_slices, int group_slices, int lds_floats, int cols, int rows, long long group, int4 g) {
    extern __shared__ unsigned colwin[];
    constexpr int kE = kSliceSteps * kLaneElems;
    constexpr int NP = kPacked<VB>;
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6), n_waves = (int)(blockDim.x >> 6);
    // the forward kernel's walk; the first request leaves before the window is filled
    auto wk = GroupWalk<USE_LDS, COMPACT, STRAYS, HALF>::at(stream, n_slices, group_slices, lds_floats, group, g, wave, n_waves);
    const bool strays = wk.strays;
    unsigned* const stray_area = colwin + wk.win_floats + wave * kStraySlots;
    // the columns of every slice's strays live behind the headers (hispmv_abi.cpp), 64 per slice, 0xffffffff = none
    const unsigned* const stray_cols = (const unsigned*)(hdr + n_slices);

    SliceMetas<COMPACT> w;
    int4 h = int4{0, 0, 0, 0};
    if (wk.live()) {
        h = load_int4(hdr + wk.cur());
        request_metas<COMPACT, HALF>(w, wk.slice(), lane);
    }
    if (USE_LDS) fill_column_window(colwin, frags, g, wk.in_lds, lds_floats, wk.win_floats, lane, wave, n_waves);

    // A lane past the batch reads the halves of lane 0 (always inside the row).  keep[i]: the lane's vector i is below n_vecs; the
    // PRODUCT of every other one is masked to +0, so that neither a pad half of gyt nor one of xt (NaN, say) gets into a sum.
    const int lane_vec = a.tile0 + lane * VB;
    const unsigned lane_bytes = lane_vec < a.n_vecs ? (unsigned)(lane * VB * 2) : 0u;      // (a uniform row address + these 32 bits: one scalar-base load)
    const uint16_t* const xtile = a.xt + a.tile0;
    const uint16_t* const gtile = a.gyt + a.tile0;
    bool keep[VB];
#pragma unroll
    for (int i = 0; i < VB; ++i) keep[i] = lane_vec + i < a.n_vecs;
    // gyt[row, the lane's vectors], packed; a row past the matrix (elements of padding behind the last row) reads row 0: its map word is 0
    const auto load_gy = [&](unsigned (&d)[NP], int row) {
        const int rc = (row >= 0 && row < rows) ? row : 0;
        load_packed<VB>((const uint16_t*)((const char*)(gtile + (size_t)rc * (size_t)a.ld_gy) + lane_bytes), d);
    };

    while (wk.live()) {
        // the row of the slice's first element, even when that row began slices earlier; an element's row is this plus the row ends
        // passed so far in the slice, in stream order (the decode of value_grad_group)
        int row = __builtin_amdgcn_readfirstlane(h.x);
        const long long cur = wk.cur();
        float gy[VB];                   // of `row`, widened
        unsigned gy_next[NP];           // of row + 1, requested one row end ahead, packed until it becomes gy
        {
            unsigned d[NP];
            load_gy(d, row);
            widen<VB>(d, gy);
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
        // gathers its VB halves of that column's row of xt.  The gathers carry no branch: an element without a column reads row 0 of
        // xt (its sum is dropped at the store: its map word is 0).
        // NK elements per gather: the four of a lane, or -- VB 8, 16 bytes per lane and element -- its two halves one after the other
        constexpr int NK = VB == 8 ? kLaneElems / 2 : kLaneElems;
        struct Gathered { unsigned m[NK]; unsigned x[NK][NP]; };
        const auto gather = [&](Gathered& q, int j, int L, int k0) {
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                q.m[k] = (unsigned)__builtin_amdgcn_readlane((int)meta[4 * j + k0 + k], L);
                load_packed<VB>((const uint16_t*)((const char*)(xtile + (size_t)(q.m[k] < kSkipMeta ? q.m[k] >> 1 : 0u) * (size_t)a.ld_x) + lane_bytes), q.x[k]);
            }
        };
        // -> the lane's partial of each of the four elements; behind a row end (wave-uniform) gyt of the next row
        const auto consume = [&](const Gathered& q, float (&p)[kLaneElems], int k0) {
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                float x[VB];
                widen<VB>(q.x[k], x);
                float s = 0.0f;
#pragma unroll
                for (int i = 0; i < VB; ++i) s = s + (keep[i] ? gy[i] * x[i] : 0.0f);
                asm volatile("" : "+v"(s));      // the sum is formed HERE: left alone, hipcc sinks the products below the row-end branches and keeps every gathered half live
                p[k0 + k] = s;
                if (q.m[k] & 1u) {
                    row += 1;
                    widen<VB>(gy_next, gy);
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
template <int VB, bool USE_LDS, bool STRAYS, bool HALF>
__global__ __launch_bounds__(1024) void spmm_grad_bf16_slices_kernel(
    const char* __restrict__ words, const int4* __restrict__ hdr, const int4* __restrict__ groups, const int4* __restrict__ frags,
    const int32_t* __restrict__ map, SpmmGradBf16Operands a, long long n_slices, int group_slices, int lds_floats, int cols, int rows) {
    const long long group = (long long)blockIdx.x;
    if constexpr (USE_LDS) {
        const int4 g = load_int4(groups + group);
        const int gw = __builtin_amdgcn_readfirstlane(g.w);
        if constexpr (HALF) {
            if (gw & kGroupHalf) {
                spmm_grad_bf16_group<VB, true, true, STRAYS, true>(words, hdr, frags, map, a, n_slices, group_slices, lds_floats, cols, rows, group, g);
                return;
            }
        }
        if (gw & kGroupCompact)
            spmm_grad_bf16_group<VB, true, true, STRAYS, false>(words, hdr, frags, map, a, n_slices, group_slices, lds_floats, cols, rows, group, g);
        else
            spmm_grad_bf16_group<VB, true, false, false, false>(words, hdr, frags, map, a, n_slices, group_slices, lds_floats, cols, rows, group, g);
    } else {
        spmm_grad_bf16_group<VB, false, false, false, false>(words, hdr, frags, map, a, n_slices, group_slices, lds_floats, cols, rows, group, int4{0, 0, 0, 0});
    }
}

template <int VB>
hipError_t launch_slices(const SpmvDeviceMatrix& m, const int32_t* map, const SpmmGradBf16Operands& a, hipStream_t stream) {
    return with_slice_flags(m, [&](auto USE_LDS, auto STRAYS, auto HALF) {
        constexpr auto kernel = spmm_grad_bf16_slices_kernel<VB, USE_LDS(), STRAYS(), HALF()>;
        const hipError_t e = raise_lds_limit<kernel>();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kernel, dim3((unsigned)m.n_groups), dim3((unsigned)m.block_threads), (size_t)m.lds_floats * 4, stream, (const char*)m.words, m.hdr,
                           m.groups, m.frags, map, a, (long long)m.n_slices, m.group_slices, m.lds_floats, m.cols, m.rows);
        return hipGetLastError();
    });
}

}  // namespace

hipError_t launch_spmm_grad_bf16_part(const SpmvDeviceMatrix& m, int vb, const int32_t* map, const SpmmGradBf16Operands& a, hipStream_t stream) {
    (void)hipGetLastError();
    if (m.n_slices <= 0 || m.n_groups <= 0 || a.n <= 0) return hipSuccess;
    if (!map) return hipErrorInvalidValue;
    if (!slice_geometry_ok(m, (size_t)m.lds_floats * 4)) return hipErrorInvalidValue;
    if (m.rows <= 0 || m.cols <= 0) return hipErrorInvalidValue;          // (rows 0 and columns 0 of gyt and xt are read for elements without a place)
    if (!a.gyt || !a.xt || !a.grad || a.n_vecs < 1 || a.tile0 < 0 || a.tile0 >= a.n_vecs || a.ld_x < a.n_vecs || a.ld_gy < a.n_vecs) return hipErrorInvalidValue;
    if (vb != 8 && vb != 4 && vb != 2 && vb != 1) return hipErrorInvalidValue;
    // a lane's vb halves are one aligned load that ends inside the row: the tile rule's (c), checked where the loads are issued
    if (a.tile0 % vb || a.ld_x % vb || a.ld_gy % vb || ((uintptr_t)a.gyt | (uintptr_t)a.xt) % (uintptr_t)(2 * vb)) return hipErrorInvalidValue;
    switch (vb) {
        case 8: return launch_slices<8>(m, map, a, stream);
        case 4: return launch_slices<4>(m, map, a, stream);
        case 2: return launch_slices<2>(m, map, a, stream);
        default: return launch_slices<1>(m, map, a, stream);
    }
}

}  // namespace hispmv
