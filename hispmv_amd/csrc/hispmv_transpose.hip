// hispmv_transpose.hip -- the kernels of the transposed product (hispmv_transpose.h): y[cols] = alpha * A^T * x[rows] + beta * bias[cols]
// on the slice streams and dense layouts of loaded handles.  What it needs of the slice format (the slice request, decode_metas, the bf16
// widening, the launch checks) it shares with the other four satellite files: hispmv_slice_walk.h.
// hispmv_kernels.hip takes no part in that and keeps its own text, so that no forward kernel is touched from here.
//
// Roles, against the forward slice kernel (hispmv_kernels.hip: slices_group):
//   forward                                           transposed
//   x window of the group in the LDS (staged)         the same floats ZEROED: accumulators of y, flushed per fragment at the end
//   row-total tile of a wavefront (one slice's y)     x[row_first .. row_first + n_rows] of the slice (its rows are consecutive)
//   stray area of a wavefront (x of <= 64 strays)     accumulators of the slice's strays, flushed per slice to the stray columns
//   gather through L2 (wide metas, no-window plans)   one global float atomic per element (the expensive shape: 64 lanes, 64 lines)
// A stored slot whose value is +-0 adds nothing, whatever x holds (fillers of empty rows, row extensions, tail padding, explicit zeros).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "hispmv_slice_walk.h"
#include "hispmv_transpose.h"

namespace hispmv {

namespace {

// The float adds: ds_add_f32 into the LDS here, global_atomic_add_f32 (no return value) into y with y_add.
__device__ __forceinline__ void lds_add(float* p, float v) { (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// y = beta * bias, 4 consecutive floats per thread.  Each thread reads what it writes: bias may be y.
// Several vectors are ONE array of n floats to this kernel (y of vector v begins at v * cols); `period` > 0: they share one bias of
// `period` floats (y[i] = beta * bias[i % period]; `vec` then requires period % 4 == 0), 0: bias is as long as y.
__global__ __launch_bounds__(256) void transpose_prologue_kernel(const float* bias, float* y, int n, float beta, int vec, int period) {
    const long long i0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i0 >= n) return;
    if (vec && i0 + 3 < n) {
        float4 b = float4{0.0f, 0.0f, 0.0f, 0.0f};
        if (beta != 0.0f) { b = *(const float4*)(bias + (period ? i0 % period : i0)); b.x *= beta; b.y *= beta; b.z *= beta; b.w *= beta; }
        *(float4*)(y + i0) = b;
    } else {
        for (long long i = i0; i < i0 + 4 && i < n; ++i) y[i] = beta != 0.0f ? beta * bias[period ? i % period : i] : 0.0f;
    }
}

// The work of one workgroup on group `group` of a slice stream, for a group stored COMPACT (6 B per element), HALF (4 B) or wide (8 B),
// on NV vectors in one pass over the stream (NV > 1: hispmv_linear_device_t; the roles batched_group has against slices_group in the
// forward file).  Vector v reads x + v * rows and adds into y + v * cols.  A slice's words are decoded ONCE -- metas c, values v, local
// rows lr stay in registers -- and the NV vectors then go through the element loop one after the other.
// STRAYS: the plan has stray areas behind the window (m.has_strays); whether THIS group uses them is bit 2 of its group word.
// LDS, slice_lds_bytes(m, NV) in all: [NV accumulator windows of lds_floats each (the wavefronts' stray areas are a window's last
// floats): window v at xs + v * lds_floats][ONE x tile of ytile_floats per wavefront]; with NV = 1 that is the forward launch's.
// x is reached through a buffer descriptor over `rows` floats, one per vector: a row past the end (the open row behind the last slice)
// reads as 0 and not as the next vector's x[0].
// Where the tile is filled differs, and each order is the one its kernels were measured with:
//   NV == 1  descriptor ahead of the walk; the whole tile and the open row are loaded BEFORE the next slice is requested
//   NV > 1   descriptor after the request; the first 64 floats of a vector's tile and its open row (t_head, t_open) are requested one
//            vector ahead, before the current vector's elements are multiplied
// `if constexpr (NV == 1) break;` at the end of a loop over the vectors: with one vector there is no loop for the compiler to hoist out
// of, and the instructions stay where the one-vector text had them (2.30).
template <int NV, bool USE_LDS, bool COMPACT, bool STRAYS, bool HALF>
__device__ __forceinline__ void slices_group_t(
    const char* __restrict__ stream, const int4* __restrict__ hdr, const int4* __restrict__ frags, const float* __restrict__ x, float* y,
    float alpha, long long n_slices, int group_slices, int lds_floats, int ytile_floats, int cols, int rows, long long group, int4 g) {
    extern __shared__ float xs[];
    constexpr int kE = kSliceSteps * kLaneElems;
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6), n_waves = (int)(blockDim.x >> 6);
    __amdgpu_buffer_rsrc_t rx;
    if constexpr (NV == 1) rx = __builtin_amdgcn_make_buffer_rsrc((void*)x, 0, rows * 4, 0x00020000);
    float* const xtile = xs + (USE_LDS ? lds_floats * NV : 0) + wave * ytile_floats;
    // the forward kernel's walk; the first request leaves before the windows are zeroed
    auto wk = GroupWalk<USE_LDS, COMPACT, STRAYS, HALF>::at(stream, n_slices, group_slices, lds_floats, group, g, wave, n_waves);
    const bool in_lds = wk.in_lds, strays = wk.strays;
    const int win_floats = wk.win_floats;
    // this wavefront's stray area: a pointer for one vector, formed here; an offset into every vector's window for NV > 1
    float* const stray_one = xs + win_floats + wave * kStraySlots;
    const int stray_at = win_floats + wave * kStraySlots;
    // the columns of every slice's strays live behind the headers (hispmv_load.cpp: upload_slice_layout), 64 per slice, 0xffffffff = none
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(hdr + n_slices), 0, strays ? (int)(n_slices * (kStraySlots * 4)) : 0, 0x00020000);

    SliceRaw<COMPACT, HALF> w;
    int4 h = int4{0, 0, 0, 0};
    if (wk.live()) {
        h = load_int4(hdr + wk.cur());
        request_slice<COMPACT, HALF>(w, wk.slice(), lane);
    }
    if (USE_LDS) {
        for (int i = (int)threadIdx.x; i < lds_floats * NV; i += (int)blockDim.x) xs[i] = 0.0f;
        __syncthreads();
    }

    while (wk.live()) {
        const int row_first = __builtin_amdgcn_readfirstlane(h.x);      // first row that ends in this slice
        const int n_rows = __builtin_amdgcn_readfirstlane(h.z);         // rows that end in it; its elements lie in rows row_first .. row_first + n_rows
        const long long cur = wk.cur();
        unsigned c[kE];
        float v[kE];
        decode_metas<COMPACT, HALF>(w, c);
        slice_values<COMPACT, HALF>(w, v);
        // x of the slice's rows -> this wavefront's tile, coalesced; the open last row has no place in a full tile and is kept in a register
        float x_open, t_head, t_open;
        if constexpr (NV == 1) {
            for (int i = lane; i <= n_rows && i < ytile_floats; i += 64)
                xtile[i] = i2f((int)__builtin_amdgcn_raw_buffer_load_b32(rx, (unsigned)(row_first + i) << 2, 0, 0));
            x_open = i2f((int)__builtin_amdgcn_raw_buffer_load_b32(rx, (unsigned)(row_first + n_rows) << 2, 0, 0));
        }
        unsigned sc = kNoAccess;
        if (strays) sc = __builtin_amdgcn_raw_buffer_load_b32(rs, (unsigned)(cur * kStraySlots + lane) << 2, 0, 0);
        int lr[kE];
        local_rows(c, lr);
        // the next slice of this wavefront, into the registers the copies above have left
        wk.advance();
        if (wk.live()) {
            h = load_int4(hdr + wk.cur());
            request_slice<COMPACT, HALF>(w, wk.slice(), lane);
        }
        if constexpr (NV > 1) {       // vector 0: the head of its tile (rows row_first + lane) and its open row
            rx = __builtin_amdgcn_make_buffer_rsrc((void*)x, 0, rows * 4, 0x00020000);
            t_head = i2f((int)__builtin_amdgcn_raw_buffer_load_b32(rx, (unsigned)(row_first + lane) << 2, 0, 0));
            t_open = i2f((int)__builtin_amdgcn_raw_buffer_load_b32(rx, (unsigned)(row_first + n_rows) << 2, 0, 0));
        }
#pragma unroll 1
        for (int vv = 0; vv < NV; ++vv) {
            float* const win = xs + vv * lds_floats;
            float* const yv = y + (size_t)vv * (size_t)cols;
            float* const stray_area = NV == 1 ? stray_one : win + stray_at;
            if constexpr (NV > 1) {
                if (lane <= n_rows && lane < ytile_floats) xtile[lane] = t_head;
                for (int i = lane + 64; i <= n_rows && i < ytile_floats; i += 64)
                    xtile[i] = i2f((int)__builtin_amdgcn_raw_buffer_load_b32(rx, (unsigned)(row_first + i) << 2, 0, 0));
                x_open = t_open;
                if (vv + 1 < NV) {
                    rx = __builtin_amdgcn_make_buffer_rsrc((void*)(x + (size_t)(vv + 1) * (size_t)rows), 0, rows * 4, 0x00020000);
                    t_head = i2f((int)__builtin_amdgcn_raw_buffer_load_b32(rx, (unsigned)(row_first + lane) << 2, 0, 0));
                    t_open = i2f((int)__builtin_amdgcn_raw_buffer_load_b32(rx, (unsigned)(row_first + n_rows) << 2, 0, 0));
                }
            }
            __builtin_amdgcn_wave_barrier();      // (LDS operations of one wavefront execute in order: the tile is complete for every lane)
#pragma unroll
            for (int i = 0; i < kE; ++i) {
                const int li = lr[i] < ytile_floats ? lr[i] : ytile_floats - 1;
                const float xt = xtile[li];
                const float xr = lr[i] < ytile_floats ? xt : x_open;
                if ((f2i(v[i]) & 0x7fffffff) == 0) continue;          // a +-0 slot adds nothing, whatever x holds
                const float p = v[i] * xr;
                if constexpr (COMPACT) {
                    const int idx = (int)(c[i] & 0x7fffu);
                    if (STRAYS && strays && idx >= win_floats) lds_add(stray_area + ((idx - win_floats) & (kStraySlots - 1)), p);
                    else lds_add(win + idx, p);
                } else {
                    const unsigned ci = c[i] & ~kRowEndBit;
                    if (USE_LDS && in_lds && !(ci & kGlobalColBit)) {
                        if (ci < (unsigned)win_floats) lds_add(win + ci, p);
                    } else {
                        const unsigned col = ci & ~kGlobalColBit;
                        if (col < (unsigned)cols) y_add(yv, col, alpha * p);
                    }
                }
            }
            if (STRAYS && strays) {       // this vector's strays of the slice leave for their columns; its area is zero again for the wavefront's next slice
                __builtin_amdgcn_wave_barrier();
                const float a = stray_area[lane];
                stray_area[lane] = 0.0f;
                if (sc != kNoAccess && sc < (unsigned)cols) y_add(yv, sc, alpha * a);
            }
            __builtin_amdgcn_wave_barrier();      // the tile is read: the next vector (or slice) may fill it
            if constexpr (NV == 1) break;
        }
    }
    if (USE_LDS) {
        __syncthreads();
        // the flush: per fragment {col_start, len, lds_off} one wave-instruction per 64 consecutive floats of y, vector after vector
        const int f0 = __builtin_amdgcn_readfirstlane(g.x), nf = in_lds ? __builtin_amdgcn_readfirstlane(g.y) : 0;
        for (int f = wave; f < nf; f += n_waves) {
            const int4 fr = load_int4(frags + f0 + f);
            const int col0 = __builtin_amdgcn_readfirstlane(fr.x), len = __builtin_amdgcn_readfirstlane(fr.y), off = __builtin_amdgcn_readfirstlane(fr.z);
#pragma unroll
            for (int vv = 0; vv < NV; ++vv)
                for (int i = lane; i < len; i += 64)
                    if (col0 + i < cols && off + i < win_floats) y_add(y + (size_t)vv * (size_t)cols, (unsigned)(col0 + i), alpha * xs[vv * lds_floats + off + i]);
        }
    }
}

// HALF: the handle stores bf16 values and has half groups; the group word of every group decides which body decodes it.
template <int NV, bool USE_LDS, bool STRAYS, bool HALF>
__global__ __launch_bounds__(1024) void spmv_slices_t_kernel(
    const char* __restrict__ words, const int4* __restrict__ hdr, const int4* __restrict__ groups, const int4* __restrict__ frags,
    const float* __restrict__ x, float* y, float alpha, long long n_slices, int group_slices, int lds_floats, int ytile_floats, int cols, int rows) {
    const long long group = (long long)blockIdx.x;
    if constexpr (USE_LDS) {
        const int4 g = load_int4(groups + group);
        const int gw = __builtin_amdgcn_readfirstlane(g.w);
        if constexpr (HALF) {
            if (gw & kGroupHalf) {
                slices_group_t<NV, true, true, STRAYS, true>(words, hdr, frags, x, y, alpha, n_slices, group_slices, lds_floats, ytile_floats, cols, rows, group, g);
                return;
            }
        }
        // (a compact group that is not half does not exist in a bf16 handle today; should a packer ever make one, it is decoded as what
        // its group word says it is)
        if (gw & kGroupCompact)
            slices_group_t<NV, true, true, STRAYS, false>(words, hdr, frags, x, y, alpha, n_slices, group_slices, lds_floats, ytile_floats, cols, rows, group, g);
        else
            slices_group_t<NV, true, false, false, false>(words, hdr, frags, x, y, alpha, n_slices, group_slices, lds_floats, ytile_floats, cols, rows, group, g);
    } else {
        slices_group_t<NV, false, false, false, false>(words, hdr, frags, x, y, alpha, n_slices, group_slices, lds_floats, ytile_floats, cols, rows, group, int4{0, 0, 0, 0});
    }
}

// W[r][c0 .. c0 + 3] as fp32 (gemv_t_kernel's loads): zeros past `cols`
template <bool BF16, bool VEC>
__device__ __forceinline__ float4 gemv_t_load_w(const void* __restrict__ Wv, size_t at, int c0, int cols) {
    float4 w = float4{0.0f, 0.0f, 0.0f, 0.0f};
    if constexpr (BF16) {
        const uint16_t* W = (const uint16_t*)Wv;
        if constexpr (VEC) {
            const uint2 q = *(const uint2*)(W + at);
            w.x = i2f((int)(q.x << 16)); w.y = i2f((int)(q.x & 0xffff0000u)); w.z = i2f((int)(q.y << 16)); w.w = i2f((int)(q.y & 0xffff0000u));
        } else {
            w.x = i2f((int)((unsigned)W[at] << 16));
            if (c0 + 1 < cols) w.y = i2f((int)((unsigned)W[at + 1] << 16));
            if (c0 + 2 < cols) w.z = i2f((int)((unsigned)W[at + 2] << 16));
            if (c0 + 3 < cols) w.w = i2f((int)((unsigned)W[at + 3] << 16));
        }
    } else {
        const float* W = (const float*)Wv;
        if constexpr (VEC) {
            w = *(const float4*)(W + at);
        } else {
            w.x = W[at];
            if (c0 + 1 < cols) w.y = W[at + 1];
            if (c0 + 2 < cols) w.z = W[at + 2];
            if (c0 + 3 < cols) w.w = W[at + 3];
        }
    }
    return w;
}

// Dense: a workgroup of 256 threads takes rows [r0, r1) x kGemvTCols columns.  A thread owns 4 consecutive columns (one 16-byte load of
// fp32 W per row, 8 bytes of bf16 W) and sums over the rows in registers, x[row] wave-uniform; the sums cross the LDS so that every
// wave-instruction of the output covers 64 consecutive floats of y.  VEC: cols % 4 == 0 and W aligned; otherwise element loads (odd
// cols, where a row of W starts at any 4-byte -- bf16: 2-byte -- boundary).
// NV vectors per pass over W (NV > 1: hispmv_linear_device_t): vector v reads x + v * rows and adds into y + v * cols.  A thread owns
// 4 columns x NV sums, x[v * rows + r] is wave-uniform, W is read once; the LDS transposition holds NV x kGemvTCols floats.  Per vector
// the sum of a column is the one a pass of one vector forms (same row blocks, same order inside a block).
// (`if constexpr (NV == 1) break;`: as in slices_group_t)
template <bool BF16, bool VEC, int NV>
__global__ __launch_bounds__(256) void gemv_t_kernel(const void* __restrict__ Wv, int rows, int cols, const float* __restrict__ x, float* y,
                                                    float alpha, int rows_per_block, int atomic) {
    __shared__ float out[NV][kGemvTCols];
    const int tid = (int)threadIdx.x;
    const int cb = (int)blockIdx.x * kGemvTCols;
    const int c0 = cb + tid * 4;
    const int r0 = (int)blockIdx.y * rows_per_block;
    const int r1 = r0 + rows_per_block < rows ? r0 + rows_per_block : rows;
    float4 a[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) { a[v] = float4{0.0f, 0.0f, 0.0f, 0.0f}; if constexpr (NV == 1) break; }
    if (c0 < cols) {
#pragma unroll 4
        for (int r = r0; r < r1; ++r) {
            float x_first;
            if constexpr (NV == 1) x_first = x[r];          // one vector: x[r] is requested ahead of W, the order its kernels were measured with
            const float4 w = gemv_t_load_w<BF16, VEC>(Wv, (size_t)r * (size_t)cols + (size_t)c0, c0, cols);
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                const float xr = NV == 1 ? x_first : x[(size_t)v * (size_t)rows + (size_t)r];
                a[v].x += w.x * xr; a[v].y += w.y * xr; a[v].z += w.z * xr; a[v].w += w.w * xr;
                if constexpr (NV == 1) break;
            }
        }
    }
#pragma unroll
    for (int v = 0; v < NV; ++v) { out[v][tid * 4 + 0] = a[v].x; out[v][tid * 4 + 1] = a[v].y; out[v][tid * 4 + 2] = a[v].z; out[v][tid * 4 + 3] = a[v].w; }
    __syncthreads();
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        float* const yv = y + (size_t)v * (size_t)cols;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int col = cb + tid + 256 * k;
            if (col >= cols) continue;
            const float s = alpha * out[v][tid + 256 * k];
            if (atomic) y_add(yv, (unsigned)col, s);
            else yv[col] = yv[col] + s;            // one row block: this thread is the only writer of the column
        }
    }
}

template <int NV>
hipError_t launch_slices_t(const SpmvDeviceMatrix& m, const float* x, float* y, float alpha, hipStream_t stream) {
    return with_slice_flags(m, [&](auto USE_LDS, auto STRAYS, auto HALF) {
        constexpr auto kernel = spmv_slices_t_kernel<NV, USE_LDS(), STRAYS(), HALF()>;
        const hipError_t e = raise_lds_limit<kernel>();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kernel, dim3((unsigned)m.n_groups), dim3((unsigned)m.block_threads), slice_lds_bytes(m, NV), stream, (const char*)m.words, m.hdr,
                           m.groups, m.frags, x, y, alpha, (long long)m.n_slices, m.group_slices, m.lds_floats, m.ytile_floats, m.cols, m.rows);
        return hipGetLastError();
    });
}

// the dense kernel of a pass of NV vectors, by weight type and by whether W takes vector loads
template <int NV>
auto gemv_t_kernel_of(bool bf16, bool vec) {
    return bf16 ? (vec ? gemv_t_kernel<true, true, NV> : gemv_t_kernel<true, false, NV>) : (vec ? gemv_t_kernel<false, true, NV> : gemv_t_kernel<false, false, NV>);
}

}  // namespace

hipError_t launch_transpose_prologue(const float* bias, float* y, int32_t n, float beta, hipStream_t stream, int64_t vecs, int64_t bias_stride) {
    (void)hipGetLastError();
    if (n <= 0 || vecs <= 0) return hipSuccess;
    const int64_t total = (int64_t)n * vecs;
    if (total >= (1LL << 30) || (bias_stride != 0 && bias_stride != n)) return hipErrorInvalidValue;
    const bool shared = vecs > 1 && bias_stride == 0 && beta != 0.0f;        // one bias of n floats under every vector
    const bool aligned = ((uintptr_t)y & 15) == 0 && (beta == 0.0f || ((uintptr_t)bias & 15) == 0) && (!shared || (n & 3) == 0);
    hipLaunchKernelGGL(transpose_prologue_kernel, dim3((unsigned)((total + 1023) / 1024)), dim3(256), 0, stream, bias, y, (int)total, beta, aligned ? 1 : 0,
                       shared ? (int)n : 0);
    return hipGetLastError();
}

// Plan classes of the multi-vector pass; spmv_t_width is where a class that a measurement shows no faster than single calls is narrowed.
int spmv_t_width(const SpmvDeviceMatrix& m, int64_t vecs) {
    for (int nv = kMaxBatch; nv >= 2; nv >>= 1) {
        if (nv > vecs) continue;
        if ((int64_t)m.cols * nv >= (1 << 30) || (int64_t)m.rows * nv >= (1 << 30)) continue;
        if (slice_lds_bytes(m, nv) <= (size_t)kDynLdsMax) return nv;
    }
    return 1;
}

hipError_t launch_spmv_t(const SpmvDeviceMatrix& m, int nv, const float* x, float* y, float alpha, hipStream_t stream) {
    (void)hipGetLastError();
    if (nv != 1 && nv != 2 && nv != 4) return hipErrorInvalidValue;
    if (m.n_slices <= 0 || m.n_groups <= 0) return hipSuccess;
    if (!slice_geometry_ok(m, slice_lds_bytes(m, nv)) || (nv > 1 && spmv_t_width(m, nv) != nv)) return hipErrorInvalidValue;
    switch (nv) {
        case 4: return launch_slices_t<4>(m, x, y, alpha, stream);
        case 2: return launch_slices_t<2>(m, x, y, alpha, stream);
        default: return launch_slices_t<1>(m, x, y, alpha, stream);
    }
}

// Row blocks per column block: enough workgroups to fill the chip twice over (1024 in all) while a block keeps at least 16 rows,
// so that a small layer still spreads over the CUs and the atomic bytes stay a small multiple of y.
int gemv_t_row_blocks(int32_t rows, int32_t cols) {
    if (rows <= 0 || cols <= 0) return 0;
    const int64_t col_blocks = ((int64_t)cols + kGemvTCols - 1) / kGemvTCols;
    const int64_t want = std::max<int64_t>(1, (1024 + col_blocks - 1) / col_blocks);
    const int64_t most = ((int64_t)rows + 15) / 16;
    const int64_t nb = std::min(want, most);
    const int64_t per = ((int64_t)rows + nb - 1) / nb;
    return (int)(((int64_t)rows + per - 1) / per);
}

int gemv_t_width(int64_t vecs) { return vecs >= 8 ? 8 : vecs >= 4 ? 4 : vecs >= 2 ? 2 : 1; }

hipError_t launch_gemv_t(const void* W, int32_t rows, int32_t cols, bool bf16, int nv, const float* x, float* y, float alpha, hipStream_t stream) {
    (void)hipGetLastError();
    if (nv != 1 && nv != 2 && nv != 4 && nv != 8) return hipErrorInvalidValue;
    if (nv > 1 && ((int64_t)rows * nv >= (1 << 30) || (int64_t)cols * nv >= (1 << 30))) return hipErrorInvalidValue;
    const int nb = gemv_t_row_blocks(rows, cols);
    if (nb <= 0) return hipSuccess;
    const int per = (rows + nb - 1) / nb;
    const dim3 grid((unsigned)(((int64_t)cols + kGemvTCols - 1) / kGemvTCols), (unsigned)nb);
    const bool vec = (cols & 3) == 0 && ((uintptr_t)W & (bf16 ? 7 : 15)) == 0;
    const int atomic = nb > 1 ? 1 : 0;
    const auto kernel = nv == 8 ? gemv_t_kernel_of<8>(bf16, vec) : nv == 4 ? gemv_t_kernel_of<4>(bf16, vec) : nv == 2 ? gemv_t_kernel_of<2>(bf16, vec) : gemv_t_kernel_of<1>(bf16, vec);
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, W, (int)rows, (int)cols, x, y, alpha, per, atomic);
    return hipGetLastError();
}

}  // namespace hispmv
