// hispmv_value_grad.hip -- the kernels of the value gradient (hispmv_value_grad.h): grad[k] = alpha * sum_v gy[v, row_k] * x[v, col_k]
// + beta * grad[k] for every entry k of the creation input, on the slice streams and dense layouts of loaded, updatable handles.
// What it needs of the slice format (the meta request, decode_metas, store_grad, the buffer loads, the launch
// checks) it shares with the other four satellite files: hispmv_slice_walk.h.  hispmv_kernels.hip shares only the slice decode under it
// (hispmv_slice_decode.h) and keeps its own text of the rest, so that no forward kernel is touched from here.
//
// Roles, against the forward slice kernel (hispmv_kernels.hip: slices_group / batched_group) and the transposed one (slices_group_t):
//   forward                                  transposed                                 value gradient
//   x window of the group in the LDS         the same floats as accumulators of y       x window, staged per vector (dword loads)
//   row-total tile of a wavefront            x[row_first ..] of the slice's rows        gy[row_first ..] of the slice's rows
//   stray area of a wavefront                accumulators of the slice's strays         x of the slice's <= 64 strays, per vector
//   gather through L2                        one global float atomic per element        the same bounds-checked gather of x
//   values x products -> row sums            values x products -> column sums           NO values: 16 products per lane summed over the
//                                                                                       vectors, stored through the value map
// A slot whose map word is 0 (fillers of empty rows, row extensions, padding) writes nothing; an explicit zero of the input has a map
// word like every other entry and gets its gradient.
#include <hip/hip_runtime.h>

#include "hispmv_slice_walk.h"
#include "hispmv_update.h"
#include "hispmv_value_grad.h"

namespace hispmv {

namespace {

// The work of one workgroup on group `group` of a slice stream for a pass of NV vectors, for a group stored COMPACT (6 B per element),
// HALF (a compact group of a bf16 handle, 4 B) or wide (8 B).  STRAYS: the plan has stray areas behind the window; whether THIS group uses them is bit 2 of its group word.
// LDS: [NV x windows of lds_floats each (the wavefronts' stray areas are a window's last floats): window v at xs + v * lds_floats]
// [ONE gy tile of ytile_floats per wavefront], slice_lds_bytes(m, NV) in all.  Vector v reads gy + v * rows and x + v * cols, each
// through its own buffer descriptor, so a row or column past the end reads 0 and not the next vector's first float.
template <int NV, bool USE_LDS, bool COMPACT, bool STRAYS, bool HALF = false>
__device__ __forceinline__ void value_grad_group(
    const char* __restrict__ stream, const int4* __restrict__ hdr, const int4* __restrict__ frags, const int32_t* __restrict__ map,
    const float* __restrict__ gy, const float* __restrict__ x, float* grad, long long n, float alpha, float beta, long long n_slices,
    int group_slices, int lds_floats, int ytile_floats, int cols, int rows, long long group, int4 g) {
    extern __shared__ float xs[];
    constexpr int kE = kSliceSteps * kLaneElems;
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6), n_waves = (int)(blockDim.x >> 6);
    float* const tile = xs + (USE_LDS ? lds_floats * NV : 0) + wave * ytile_floats;
    const long long first = group * group_slices;
    const long long last = (first + group_slices < n_slices) ? first + group_slices : n_slices;
    const int n_here = (int)(last > first ? last - first : 0);
    constexpr int slice_bytes = HALF ? kHalfSliceBytes : COMPACT ? kCompactSliceBytes : kWideSliceBytes;
    const char* const gbase = stream + (USE_LDS ? (size_t)(unsigned)__builtin_amdgcn_readfirstlane(g.z) * kSliceUnit : (size_t)first * kWideSliceBytes);
    const bool in_lds = USE_LDS && __builtin_amdgcn_readfirstlane(g.y) > 0;      // 0 fragments: the metas of this group are plain columns
    const bool strays = STRAYS && COMPACT && (__builtin_amdgcn_readfirstlane(g.w) & kGroupStrays) != 0;
    const int win_floats = lds_floats - (STRAYS ? n_waves * kStraySlots : 0);
    const int stray_at = win_floats + wave * kStraySlots;          // this wavefront's stray area inside every vector's window
    // the columns of every slice's strays live behind the headers, 64 per slice, 0xffffffff = none
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(hdr + n_slices), 0, strays ? (int)(n_slices * (kStraySlots * 4)) : 0, 0x00020000);

    // the forward kernel's walk (rotated start, a wavefront takes every n_waves-th slice); the first request leaves before the windows are staged.
    // GroupWalk and local_rows of hispmv_slice_walk.h hold this text for the other files; here it stays written out, because through
    // them hipcc gave three of these kernels more SGPR spills and the compact NV = 4 ones a VGPR more
    const int rot = n_here == 0 ? 0 : (int)((unsigned long long)group * 29ull % (unsigned)n_here);
    int k_slice = wave;
    int local = k_slice < n_here ? (k_slice + rot >= n_here ? k_slice + rot - n_here : k_slice + rot) : n_here;
    SliceMetas<COMPACT> w;
    int4 h = int4{0, 0, 0, 0};
    if (local < n_here) {
        h = load_int4(hdr + first + local);
        request_metas<COMPACT, HALF>(w, gbase + (size_t)local * slice_bytes, lane);
    }
    if (USE_LDS) {
        if (in_lds) {
            // the group's fragments {col_start, len, lds_off} of every vector's x into that vector's window: dword loads, 4 in flight per lane
            const int f0 = __builtin_amdgcn_readfirstlane(g.x), nf = __builtin_amdgcn_readfirstlane(g.y);
            for (int f = wave; f < nf; f += n_waves) {
                const int4 fr = load_int4(frags + f0 + f);
                const int col0 = __builtin_amdgcn_readfirstlane(fr.x), len = __builtin_amdgcn_readfirstlane(fr.y), off = __builtin_amdgcn_readfirstlane(fr.z);
#pragma unroll 1
                for (int vv = 0; vv < NV; ++vv) {
                    const __amdgpu_buffer_rsrc_t rxv = float_buffer(x + (size_t)vv * (size_t)cols, cols);
                    float* const win = xs + vv * lds_floats + off;
                    for (int i0 = 0; i0 < len; i0 += 256) {
                        float t[4];
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            const int i = i0 + 64 * u + lane;
                            t[u] = buffer_float(rxv, (i < len && col0 + i >= 0) ? (unsigned)(col0 + i) << 2 : kNoAccess);
                        }
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            const int i = i0 + 64 * u + lane;
                            if (i < len && off >= 0 && off + i < win_floats) win[i] = t[u];
                        }
                    }
                }
            }
        }
        __syncthreads();
    }

    while (local < n_here) {
        const int row_first = __builtin_amdgcn_readfirstlane(h.x);      // first row that ends in this slice
        const int n_rows = __builtin_amdgcn_readfirstlane(h.z);         // rows that end in it; its elements lie in rows row_first .. row_first + n_rows
        const int cur = local;
        unsigned c[kE];
        decode_metas<COMPACT>(w, c);
        unsigned sc = kNoAccess;
        if (strays) sc = __builtin_amdgcn_raw_buffer_load_b32(rs, (unsigned)((first + cur) * kStraySlots + lane) << 2, 0, 0);
        // local row of every element = row ends before it in the slice (the forward kernel's ballots, plus the lane's own ends)
        int lr[kE];
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
        // the next slice of this wavefront, into the registers the decode has left
        k_slice += n_waves;
        local = k_slice < n_here ? (k_slice + rot >= n_here ? k_slice + rot - n_here : k_slice + rot) : n_here;
        if (local < n_here) {
            h = load_int4(hdr + first + local);
            request_metas<COMPACT, HALF>(w, gbase + (size_t)local * slice_bytes, lane);
        }
        float acc[kE];
#pragma unroll
        for (int i = 0; i < kE; ++i) acc[i] = 0.0f;
#pragma unroll 1
        for (int vv = 0; vv < NV; ++vv) {
            const __amdgpu_buffer_rsrc_t rg = float_buffer(gy + (size_t)vv * (size_t)rows, rows);
            const __amdgpu_buffer_rsrc_t rxv = float_buffer(x + (size_t)vv * (size_t)cols, cols);
            float* const win = xs + vv * lds_floats;
            // gy of the slice's rows -> this wavefront's tile, coalesced; the open last row has no place in a full tile and is kept in a register
            for (int i = lane; i <= n_rows && i < ytile_floats; i += 64) tile[i] = buffer_float(rg, (unsigned)(row_first + i) << 2);
            const float g_open = buffer_float(rg, (unsigned)(row_first + n_rows) << 2);
            if (STRAYS && strays) win[stray_at + lane] = buffer_float(rxv, sc < (unsigned)cols ? sc << 2 : kNoAccess);
            __builtin_amdgcn_wave_barrier();      // (LDS operations of one wavefront execute in order: tile and stray area are complete for every lane)
            // the elements in two halves of 8: a wide group gathers x through L2 for plain columns (no window) and for the kGlobalColBit
            // elements of a staged group, 8 loads in flight per lane (16 at once cost the NV = 2 body two VGPRs of scratch)
#pragma unroll
            for (int i0 = 0; i0 < kE; i0 += kE / 2) {
                float xg[COMPACT ? 1 : kE / 2];
                (void)xg;
                if constexpr (!COMPACT) {
#pragma unroll
                    for (int i = 0; i < kE / 2; ++i) {
                        const unsigned ci = c[i0 + i] & ~kRowEndBit;
                        const bool global = !(USE_LDS && in_lds) || (ci & kGlobalColBit) != 0;
                        const unsigned col = ci & ~kGlobalColBit;
                        xg[i] = buffer_float(rxv, (global && col < (unsigned)cols) ? col << 2 : kNoAccess);
                    }
                }
#pragma unroll
                for (int i = i0; i < i0 + kE / 2; ++i) {
                    const int li = lr[i] < ytile_floats ? lr[i] : ytile_floats - 1;
                    const float gt = tile[li];
                    const float gr = lr[i] < ytile_floats ? gt : g_open;
                    float xv;
                    if constexpr (COMPACT) {
                        int idx = (int)(c[i] & 0x7fffu);
                        if (STRAYS && strays && idx >= win_floats) idx = stray_at + ((idx - win_floats) & (kStraySlots - 1));
                        xv = win[idx < lds_floats ? idx : 0];
                    } else {
                        const unsigned ci = c[i] & ~kRowEndBit;
                        if (USE_LDS && in_lds && !(ci & kGlobalColBit)) {
                            const float xl = win[ci < (unsigned)win_floats ? ci : 0u];
                            xv = ci < (unsigned)win_floats ? xl : 0.0f;
                        } else {
                            xv = xg[i - i0];
                        }
                    }
                    acc[i] = acc[i] + gr * xv;
                }
            }
            __builtin_amdgcn_wave_barrier();      // tile and stray area are read: the next vector (or slice) may fill them
        }
        // the map words of the slice, addressed as its values are: element k of lane L in step j is slot (j * 64 + L) * 4 + k
        const int4* const mp = (const int4*)(map + (size_t)(first + cur) * kValueChunk) + lane;
#pragma unroll
        for (int j = 0; j < kSliceSteps; ++j) {
            const int4 q = load_int4(mp + j * 64);
            store_grad(grad, n, q.x, acc[4 * j + 0], alpha, beta);
            store_grad(grad, n, q.y, acc[4 * j + 1], alpha, beta);
            store_grad(grad, n, q.z, acc[4 * j + 2], alpha, beta);
            store_grad(grad, n, q.w, acc[4 * j + 3], alpha, beta);
        }
    }
}

// HALF: the handle stores bf16 values and has half groups; the group word of every group decides which body decodes it.
template <int NV, bool USE_LDS, bool STRAYS, bool HALF>
__global__ __launch_bounds__(1024) void value_grad_slices_kernel(
    const char* __restrict__ words, const int4* __restrict__ hdr, const int4* __restrict__ groups, const int4* __restrict__ frags,
    const int32_t* __restrict__ map, const float* __restrict__ gy, const float* __restrict__ x, float* grad, long long n, float alpha, float beta,
    long long n_slices, int group_slices, int lds_floats, int ytile_floats, int cols, int rows) {
    const long long group = (long long)blockIdx.x;
    if constexpr (USE_LDS) {
        const int4 g = load_int4(groups + group);
        const int gw = __builtin_amdgcn_readfirstlane(g.w);
        if constexpr (HALF) {
            if (gw & kGroupHalf) {
                value_grad_group<NV, true, true, STRAYS, true>(words, hdr, frags, map, gy, x, grad, n, alpha, beta, n_slices, group_slices, lds_floats, ytile_floats, cols, rows, group, g);
                return;
            }
        }
        if (gw & kGroupCompact)
            value_grad_group<NV, true, true, STRAYS>(words, hdr, frags, map, gy, x, grad, n, alpha, beta, n_slices, group_slices, lds_floats, ytile_floats, cols, rows, group, g);
        else
            // (STRAYS goes to the wide body too: it uses no stray area, but its window ends where the wavefronts' stray areas begin)
            value_grad_group<NV, true, false, STRAYS>(words, hdr, frags, map, gy, x, grad, n, alpha, beta, n_slices, group_slices, lds_floats, ytile_floats, cols, rows, group, g);
    } else {
        value_grad_group<NV, false, false, false>(words, hdr, frags, map, gy, x, grad, n, alpha, beta, n_slices, group_slices, lds_floats, ytile_floats, cols, rows, group, int4{0, 0, 0, 0});
    }
}

// Dense: a thread owns 4 consecutive columns of kValueGradRows consecutive rows; gy[v, row] is wave-uniform, x[v, c0 .. c0 + 3] is read
// once per vector for the rows of the thread.  VEC: cols % 4 == 0 and x, grad 16-byte aligned; otherwise element accesses (odd cols put
// a row of grad at any 4-byte boundary).  Write-bound: rows * cols * 4 B.
template <bool VEC>
__global__ __launch_bounds__(256) void value_grad_dense_kernel(const float* __restrict__ gy, const float* __restrict__ x, float* grad, int rows, int cols,
                                                              int vecs, float alpha, float beta) {
    constexpr int R = kValueGradRows;
    const long long c0l = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (c0l >= cols) return;
    const int c0 = (int)c0l;
    for (long long rb = blockIdx.y; rb * R < rows; rb += gridDim.y) {
        const int r0 = (int)(rb * R);
        float4 a[R];
#pragma unroll
        for (int u = 0; u < R; ++u) a[u] = float4{0.0f, 0.0f, 0.0f, 0.0f};
        for (int v = 0; v < vecs; ++v) {
            const float* const xv = x + (size_t)v * (size_t)cols + (size_t)c0;
            float4 q = float4{0.0f, 0.0f, 0.0f, 0.0f};
            if constexpr (VEC) {
                q = *(const float4*)xv;
            } else {
                q.x = xv[0];
                if (c0 + 1 < cols) q.y = xv[1];
                if (c0 + 2 < cols) q.z = xv[2];
                if (c0 + 3 < cols) q.w = xv[3];
            }
#pragma unroll
            for (int u = 0; u < R; ++u) {
                const float gr = r0 + u < rows ? gy[(size_t)v * (size_t)rows + (size_t)(r0 + u)] : 0.0f;
                a[u].x = a[u].x + gr * q.x; a[u].y = a[u].y + gr * q.y; a[u].z = a[u].z + gr * q.z; a[u].w = a[u].w + gr * q.w;
            }
        }
#pragma unroll
        for (int u = 0; u < R; ++u) {
            if (r0 + u >= rows) continue;
            float* const p = grad + (size_t)(r0 + u) * (size_t)cols + (size_t)c0;
            float4 r = float4{alpha * a[u].x, alpha * a[u].y, alpha * a[u].z, alpha * a[u].w};
            if constexpr (VEC) {
                if (beta != 0.0f) { const float4 o = *(const float4*)p; r.x = r.x + beta * o.x; r.y = r.y + beta * o.y; r.z = r.z + beta * o.z; r.w = r.w + beta * o.w; }
                *(float4*)p = r;
            } else {
                p[0] = beta != 0.0f ? r.x + beta * p[0] : r.x;
                if (c0 + 1 < cols) p[1] = beta != 0.0f ? r.y + beta * p[1] : r.y;
                if (c0 + 2 < cols) p[2] = beta != 0.0f ? r.z + beta * p[2] : r.z;
                if (c0 + 3 < cols) p[3] = beta != 0.0f ? r.w + beta * p[3] : r.w;
            }
        }
    }
}

template <int NV>
hipError_t launch_value_grad_width(const SpmvDeviceMatrix& m, const int32_t* map, const float* gy, const float* x, float* grad, int64_t n, float alpha,
                                   float beta, hipStream_t stream) {
    return with_slice_flags(m, [&](auto USE_LDS, auto STRAYS, auto HALF) {
        constexpr auto kernel = value_grad_slices_kernel<NV, USE_LDS(), STRAYS(), HALF()>;
        const hipError_t e = raise_lds_limit<kernel>();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kernel, dim3((unsigned)m.n_groups), dim3((unsigned)m.block_threads), slice_lds_bytes(m, NV), stream, (const char*)m.words, m.hdr,
                           m.groups, m.frags, map, gy, x, grad, (long long)n, alpha, beta, (long long)m.n_slices, m.group_slices, m.lds_floats, m.ytile_floats,
                           m.cols, m.rows);
        return hipGetLastError();
    });
}

}  // namespace

hipError_t launch_value_grad(const SpmvDeviceMatrix& m, int nv, const int32_t* map, const float* gy, const float* x, float* grad, int64_t n, float alpha,
                             float beta, hipStream_t stream) {
    (void)hipGetLastError();
    if (nv != 1 && nv != 2 && nv != 4) return hipErrorInvalidValue;
    if (m.n_slices <= 0 || m.n_groups <= 0 || n <= 0) return hipSuccess;
    if (!map) return hipErrorInvalidValue;
    if (!slice_geometry_ok(m, slice_lds_bytes(m, nv))) return hipErrorInvalidValue;
    if ((int64_t)m.cols * nv >= (1 << 30) || (int64_t)m.rows * nv >= (1 << 30)) return hipErrorInvalidValue;
    switch (nv) {
        case 4: return launch_value_grad_width<4>(m, map, gy, x, grad, n, alpha, beta, stream);
        case 2: return launch_value_grad_width<2>(m, map, gy, x, grad, n, alpha, beta, stream);
        default: return launch_value_grad_width<1>(m, map, gy, x, grad, n, alpha, beta, stream);
    }
}

hipError_t launch_value_grad_dense(int32_t rows, int32_t cols, int64_t vecs, const float* gy, const float* x, float* grad, float alpha, float beta,
                                   hipStream_t stream) {
    (void)hipGetLastError();
    if (rows <= 0 || cols <= 0) return hipSuccess;
    if (vecs < 1 || (int64_t)rows * vecs >= (1 << 30) || (int64_t)cols * vecs >= (1 << 30)) return hipErrorInvalidValue;
    const int64_t row_blocks = ((int64_t)rows + kValueGradRows - 1) / kValueGradRows;
    const dim3 grid((unsigned)(((int64_t)cols + 1023) / 1024), (unsigned)(row_blocks < 65535 ? row_blocks : 65535));
    const bool vec = (cols & 3) == 0 && (((uintptr_t)x | (uintptr_t)grad) & 15) == 0;
    if (vec) hipLaunchKernelGGL(value_grad_dense_kernel<true>, grid, dim3(256), 0, stream, gy, x, grad, (int)rows, (int)cols, (int)vecs, alpha, beta);
    else hipLaunchKernelGGL(value_grad_dense_kernel<false>, grid, dim3(256), 0, stream, gy, x, grad, (int)rows, (int)cols, (int)vecs, alpha, beta);
    return hipGetLastError();
}

}  // namespace hispmv
