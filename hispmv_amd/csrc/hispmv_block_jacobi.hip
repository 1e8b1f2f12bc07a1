// hispmv_block_jacobi.hip -- the kernels of the block-Jacobi preconditioner (hispmv_block_jacobi.h; include/hispmv.h: "Block-Jacobi
// preconditioner"): the extraction of the diagonal blocks of a loaded handle, the batched in-place inversion, and the multiply
// z = M^-1 r.  A satellite like the transposed product: what it needs of the slice format (the slice request, decode_metas, the walk of
// a wavefront over its group, the window in column numbers) is hispmv_slice_walk.h's, and hispmv_kernels.hip takes no part in it.
//
// Roles of the extraction, against the transposed product (hispmv_transpose.hip: slices_group_t):
//   transposed product                                   extraction
//   the window holds accumulators of y, flushed per       the window holds COLUMN NUMBERS (the wide-batch kernels' fill_column_window):
//   fragment                                              every element needs its own column to know its block
//   y_add(y, col, alpha * v * x[row])                     an add of v into word (row / bs, row % bs, col % bs) where row / bs == col / bs
//   x of the slice's rows in a tile                       nothing is multiplied: no tile
#include <hip/hip_runtime.h>

#include "hispmv_block_jacobi.h"
#include "hispmv_block_jacobi_device.h"
#include "hispmv_krylov_device.h"
#include "hispmv_slice_walk.h"

namespace hispmv {

namespace {

// ---- extraction ------------------------------------------------------------------------------------------------------------------------
// word (k, i, j) of the block area <- 1 where row k bs + i is absent (at or beyond n) and i == j, 0 elsewhere; 4 words of a row per thread
__global__ __launch_bounds__(kBlockJacobiThreads) void block_jacobi_fill_kernel(float* blocks, long long n, int sh, long long words) {
    const long long w0 = ((long long)blockIdx.x * kBlockJacobiThreads + threadIdx.x) * 4;
    if (w0 >= words) return;
    const int bs = 1 << sh;
    const long long row = w0 >> sh;                       // k bs + i
    const int j0 = (int)(w0 & (bs - 1)), i = (int)(row & (bs - 1));
    const bool absent = row >= n;
    *reinterpret_cast<float4*>(blocks + w0) = make_float4(absent && i == j0 ? 1.0f : 0.0f, absent && i == j0 + 1 ? 1.0f : 0.0f,
                                                          absent && i == j0 + 2 ? 1.0f : 0.0f, absent && i == j0 + 3 ? 1.0f : 0.0f);
}

// The work of one workgroup on group `group` of a slice stream, for a group stored COMPACT (6 B per element), HALF (4 B) or wide (8 B).
// LDS: the forward launch's window of lds_floats words (the wavefronts' stray areas are its last words), holding column numbers.
template <bool USE_LDS, bool COMPACT, bool STRAYS, bool HALF>
__device__ __forceinline__ void block_jacobi_group(const char* __restrict__ stream, const int4* __restrict__ hdr, const int4* __restrict__ frags, float* blocks,
                                                   int n, int sh, long long n_slices, int group_slices, int lds_floats, long long group, int4 g) {
    extern __shared__ unsigned colwin[];
    constexpr int kE = kSliceSteps * kLaneElems;
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

    const unsigned bs = 1u << sh;
    while (wk.live()) {
        // the row of the slice's first element, even when that row began slices earlier; an element's row is this plus the row ends
        // before it in the slice (local_rows)
        const int row0 = __builtin_amdgcn_readfirstlane(h.x);
        const long long cur = wk.cur();
        unsigned c[kE];
        float v[kE];
        decode_metas<COMPACT, HALF>(w, c);
        slice_values<COMPACT, HALF>(w, v);
        if (STRAYS && strays) {
            stray_area[lane] = ((const HISPMV_GLOBAL unsigned*)stray_cols)[cur * kStraySlots + lane];
            __builtin_amdgcn_wave_barrier();      // (LDS operations of one wavefront execute in order)
        }
        // every meta -> column << 1 | row end, or kSkipMeta | row end for a column at or beyond n (padding, fillers, kNoCol)
        unsigned meta[kE];
        resolve_columns<USE_LDS, COMPACT, STRAYS>(c, meta, colwin, stray_area, wk.in_lds, strays, wk.win_floats, lds_floats,
                                                  [&](unsigned col, int) { return col < (unsigned)n; });
        int lr[kE];
        local_rows(c, lr);
        // the next slice of this wavefront, into the registers the copies above have left
        wk.advance();
        if (wk.live()) {
            h = load_int4(hdr + wk.cur());
            request_slice<COMPACT, HALF>(w, wk.slice(), lane);
        }
#pragma unroll
        for (int i = 0; i < kE; ++i) {
            if (meta[i] >= kSkipMeta) continue;
            if ((f2i(v[i]) & 0x7fffffff) == 0) continue;          // a +-0 slot changes no value
            const unsigned col = meta[i] >> 1;
            const long long row = (long long)row0 + lr[i];
            if (row < 0 || row >= n) continue;                     // (elements of padding behind the last row)
            const unsigned r = (unsigned)row;
            if ((r >> sh) != (col >> sh)) continue;
            const size_t word = ((size_t)(r >> sh) << (2 * sh)) + (size_t)((r & (bs - 1)) << sh) + (col & (bs - 1));
            (void)atomicAdd(blocks + word, v[i]);                  // global_atomic_add_f32 without a return value
        }
        if (STRAYS && strays) __builtin_amdgcn_wave_barrier();           // the stray area is read: the next slice may fill it
    }
}

// HALF: the handle stores bf16 values and has half groups; the group word of every group decides which body decodes it.
template <bool USE_LDS, bool STRAYS, bool HALF>
__global__ __launch_bounds__(1024) void block_jacobi_slices_kernel(const char* __restrict__ words, const int4* __restrict__ hdr, const int4* __restrict__ groups,
                                                                   const int4* __restrict__ frags, float* blocks, int n, int sh, long long n_slices,
                                                                   int group_slices, int lds_floats) {
    const long long group = (long long)blockIdx.x;
    if constexpr (USE_LDS) {
        const int4 g = load_int4(groups + group);
        const int gw = __builtin_amdgcn_readfirstlane(g.w);
        if constexpr (HALF) {
            if (gw & kGroupHalf) {
                block_jacobi_group<true, true, STRAYS, true>(words, hdr, frags, blocks, n, sh, n_slices, group_slices, lds_floats, group, g);
                return;
            }
        }
        if (gw & kGroupCompact)
            block_jacobi_group<true, true, STRAYS, false>(words, hdr, frags, blocks, n, sh, n_slices, group_slices, lds_floats, group, g);
        else
            block_jacobi_group<true, false, false, false>(words, hdr, frags, blocks, n, sh, n_slices, group_slices, lds_floats, group, g);
    } else {
        block_jacobi_group<false, false, false, false>(words, hdr, frags, blocks, n, sh, n_slices, group_slices, lds_floats, group, int4{0, 0, 0, 0});
    }
}

// Dense: one thread per word of the block area reads its element of W (or writes the padding); no atomics.
template <bool BF16>
__global__ __launch_bounds__(kBlockJacobiThreads) void block_jacobi_dense_kernel(const void* __restrict__ Wv, float* blocks, long long n, int sh, long long words) {
    const long long w = (long long)blockIdx.x * kBlockJacobiThreads + threadIdx.x;
    if (w >= words) return;
    const int bs = 1 << sh;
    const long long row = w >> sh;                        // k bs + i
    const long long col = ((row >> sh) << sh) + (w & (bs - 1));
    float val = row == col ? 1.0f : 0.0f;
    if (row < n && col < n) {
        const size_t at = (size_t)row * (size_t)n + (size_t)col;
        if constexpr (BF16) val = i2f((int)((unsigned)((const uint16_t*)Wv)[at] << 16));
        else val = ((const float*)Wv)[at];
    }
    blocks[w] = val;
}

// ---- inversion -------------------------------------------------------------------------------------------------------------------------
// Gauss-Jordan in place with partial pivoting as include/hispmv.h writes it down.  One lane per row, BS lanes per block, 64 / BS blocks
// per wavefront; the row lives in BS registers with compile-time indices.  The pivoting is implicit: no row moves between lanes; lane
// sig[k] is the pivot row of column k, and on the way out the lane that was pivot of column s stores row s of the inverse with its
// word j going to column sig[j].  The pivot search is a maximum over the lanes of the block (__shfl_xor) and a ballot; the pivot row
// comes to every lane through __shfl.  A block past n_blocks (the last wavefront) computes on an identity and stores nothing.
template <int BS>
__global__ __launch_bounds__(kBlockJacobiThreads) void block_invert_kernel(float* blocks, int32_t* flags, long long n_blocks) {
    const long long gid = (long long)blockIdx.x * kBlockJacobiThreads + threadIdx.x;
    const long long blk = gid / BS;
    const int row = (int)(threadIdx.x & (BS - 1));
    const int gbase = (int)(threadIdx.x & 63) & ~(BS - 1);          // the block's first lane in the wavefront
    const bool live = blk < n_blocks;
    float* const base = blocks + blk * (BS * BS);
    float a[BS];
#pragma unroll
    for (int j = 0; j < BS; j += 4) {
        float4 q = make_float4(j == row ? 1.0f : 0.0f, j + 1 == row ? 1.0f : 0.0f, j + 2 == row ? 1.0f : 0.0f, j + 3 == row ? 1.0f : 0.0f);
        if (live) q = *reinterpret_cast<const float4*>(base + row * BS + j);
        a[j] = q.x; a[j + 1] = q.y; a[j + 2] = q.z; a[j + 3] = q.w;
    }
    bool used = false, bad = false;
    int step_of = 0;
    int sig[BS];
#pragma unroll
    for (int k = 0; k < BS; ++k) {
        // the pivot: the unused row of largest |a[k]| (compared as the bits without the sign, so a NaN counts above Inf), lowest row on ties
        const int key = used ? -1 : (f2i(a[k]) & 0x7fffffff);
        int mx = key;
#pragma unroll
        for (int s = BS / 2; s >= 1; s >>= 1) {
            const int o = __shfl_xor(mx, s, BS);
            mx = o > mx ? o : mx;
        }
        const unsigned long long bal = __builtin_amdgcn_ballot_w64(key == mx);          // (mx >= 0: a used row never matches)
        unsigned grp = (unsigned)(bal >> gbase);
        if (BS < 32) grp &= (1u << BS) - 1u;
        const int p = __builtin_ctz(grp);
        sig[k] = p;
        const float pv = __shfl(a[k], p, BS);
        const int pb = f2i(pv) & 0x7fffffff;
        if (pb == 0 || pb >= 0x7f800000) bad = true;                // zero or not finite
        const float inv = 1.0f / pv;
        const bool is_p = row == p;
        const float f = a[k];
#pragma unroll
        for (int j = 0; j < BS; ++j) {
            float nj = inv;                                          // the new pivot row: a_p[j] * inv, and inv in column k
            if (j != k) {
                const float pj = __shfl(a[j], p, BS);
                nj = pj * inv;
            }
            const float t = f * nj;
            const float old = j == k ? 0.0f : a[j];
            a[j] = is_p ? nj : old - t;
        }
        if (is_p) { used = true; step_of = k; }
    }
    bool inf = false;
#pragma unroll
    for (int j = 0; j < BS; ++j) inf = inf || (f2i(a[j]) & 0x7fffffff) >= 0x7f800000;
    unsigned any = (unsigned)(__builtin_amdgcn_ballot_w64(inf) >> gbase);
    if (BS < 32) any &= (1u << BS) - 1u;
    bad = bad || any != 0u;
    if (!live) return;
    if (bad) {
#pragma unroll
        for (int j = 0; j < BS; j += 4)
            *reinterpret_cast<float4*>(base + row * BS + j) =
                make_float4(j == row ? 1.0f : 0.0f, j + 1 == row ? 1.0f : 0.0f, j + 2 == row ? 1.0f : 0.0f, j + 3 == row ? 1.0f : 0.0f);
    } else {
#pragma unroll
        for (int j = 0; j < BS; ++j) base[step_of * BS + sig[j]] = a[j];
    }
    if (row == 0) flags[blk] = bad ? 1 : 0;
}

// ---- the multiply ----------------------------------------------------------------------------------------------------------------------
template <int BS>
__global__ __launch_bounds__(kKrylovThreads) void block_jacobi_apply_kernel(const float* blocks, int64_t n, const float* r, float* z) {
    for_chunks(n, [&](int64_t i, int m) {
        float vr[4], vz[4];
        ld4(r, i, m, vr);
        block_jacobi_mul4<BS>(blocks, i, m, vr, vz);
        st4(z, i, m, vz);
    });
}

int shift_of(int bs) { return bs == 4 ? 2 : bs == 8 ? 3 : bs == 16 ? 4 : bs == 32 ? 5 : -1; }

// f(std::integral_constant<int, BS>{}) for the four block sizes
template <class F>
hipError_t with_block_size(int bs, F&& f) {
    switch (bs) {
        case 4: return f(std::integral_constant<int, 4>{});
        case 8: return f(std::integral_constant<int, 8>{});
        case 16: return f(std::integral_constant<int, 16>{});
        case 32: return f(std::integral_constant<int, 32>{});
        default: return hipErrorInvalidValue;
    }
}

}  // namespace

hipError_t launch_block_jacobi_fill(float* blocks, int64_t n, int bs, hipStream_t s) {
    (void)hipGetLastError();
    const int sh = shift_of(bs);
    if (sh < 0 || n < 0) return hipErrorInvalidValue;
    const int64_t words = block_jacobi_layout(n, bs).n_blocks * bs * bs;
    if (words <= 0) return hipSuccess;
    const int64_t grid = (words / 4 + kBlockJacobiThreads - 1) / kBlockJacobiThreads;
    if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(block_jacobi_fill_kernel, dim3((unsigned)grid), dim3(kBlockJacobiThreads), 0, s, blocks, (long long)n, sh, (long long)words);
    return hipGetLastError();
}

hipError_t launch_block_jacobi_walk(const SpmvDeviceMatrix& m, float* blocks, int64_t n, int bs, hipStream_t s) {
    (void)hipGetLastError();
    const int sh = shift_of(bs);
    if (sh < 0 || n < 0 || n > 0x7fffffffLL) return hipErrorInvalidValue;
    if (m.n_slices <= 0 || m.n_groups <= 0) return hipSuccess;
    if (!slice_geometry_ok(m, (size_t)m.lds_floats * 4)) return hipErrorInvalidValue;
    return with_slice_flags(m, [&](auto USE_LDS, auto STRAYS, auto HALF) {
        constexpr auto kernel = block_jacobi_slices_kernel<USE_LDS(), STRAYS(), HALF()>;
        const hipError_t e = raise_lds_limit<kernel>();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kernel, dim3((unsigned)m.n_groups), dim3((unsigned)m.block_threads), (size_t)m.lds_floats * 4, s, (const char*)m.words, m.hdr, m.groups,
                           m.frags, blocks, (int)n, sh, (long long)m.n_slices, m.group_slices, m.lds_floats);
        return hipGetLastError();
    });
}

hipError_t launch_block_jacobi_dense(const void* W, bool bf16, float* blocks, int64_t n, int bs, hipStream_t s) {
    (void)hipGetLastError();
    const int sh = shift_of(bs);
    if (sh < 0 || n < 0) return hipErrorInvalidValue;
    const int64_t words = block_jacobi_layout(n, bs).n_blocks * bs * bs;
    if (words <= 0) return hipSuccess;
    const int64_t grid = (words + kBlockJacobiThreads - 1) / kBlockJacobiThreads;
    if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
    if (bf16) hipLaunchKernelGGL(block_jacobi_dense_kernel<true>, dim3((unsigned)grid), dim3(kBlockJacobiThreads), 0, s, W, blocks, (long long)n, sh, (long long)words);
    else hipLaunchKernelGGL(block_jacobi_dense_kernel<false>, dim3((unsigned)grid), dim3(kBlockJacobiThreads), 0, s, W, blocks, (long long)n, sh, (long long)words);
    return hipGetLastError();
}

hipError_t launch_block_invert(float* blocks, int32_t* flags, int64_t n_blocks, int bs, hipStream_t s) {
    (void)hipGetLastError();
    if (n_blocks < 0) return hipErrorInvalidValue;
    if (n_blocks == 0) return block_jacobi_size_ok(bs) ? hipSuccess : hipErrorInvalidValue;
    const int64_t grid = (n_blocks * bs + kBlockJacobiThreads - 1) / kBlockJacobiThreads;
    if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
    return with_block_size(bs, [&](auto BS) {
        hipLaunchKernelGGL(block_invert_kernel<BS()>, dim3((unsigned)grid), dim3(kBlockJacobiThreads), 0, s, blocks, flags, (long long)n_blocks);
        return hipGetLastError();
    });
}

hipError_t launch_block_jacobi_apply(const float* blocks, int64_t n, int bs, const float* r, float* z, hipStream_t s) {
    (void)hipGetLastError();
    if (n <= 0) return block_jacobi_size_ok(bs) ? hipSuccess : hipErrorInvalidValue;
    return with_block_size(bs, [&](auto BS) {
        hipLaunchKernelGGL(block_jacobi_apply_kernel<BS()>, dim3(grid_of(n)), dim3(kKrylovThreads), 0, s, blocks, n, r, z);
        return hipGetLastError();
    });
}

}  // namespace hispmv
