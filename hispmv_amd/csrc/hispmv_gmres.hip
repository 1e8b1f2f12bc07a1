// hispmv_gmres.hip -- the vector kernels of restarted GMRES(m) (hispmv_gmres.h; include/hispmv.h: hispmv_dot_basis_device,
// hispmv_gmres_device).  The grid, the chunk order and the dot product are hispmv_krylov.hip's: 256 threads, G = krylov_groups(n)
// workgroups, workgroup g takes chunks g, g + G, ...; vector arithmetic fp32 and unfused (-ffp-contract=off), scalars fp64, rounded
// once to fp32 before they meet a vector.  Everything between two products is a pass over the basis: one multi-dot kernel, the
// subtract-and-dot kernel twice (CGS2), and the rotate-and-normalise kernel.  Every workgroup finishes the sums it needs itself from
// the partials; only workgroup 0 writes the Givens data and the scalar block, and no kernel reads a word of these it writes.
#include <hip/hip_runtime.h>

#include "hispmv_block_jacobi_device.h"
#include "hispmv_gmres.h"
#include "hispmv_krylov_device.h"
#include "hispmv_krylov_scalar.h"

namespace hispmv {
namespace {

constexpr int T = kGmresDotTile;

// dot4 with the product fused into the sum: a product of two floats is exact in fp64, so these are the bits of multiply-then-add
__device__ __forceinline__ double dot4_fma(const float a[4], const float b[4], int m) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j < m) s = __builtin_fma((double)a[j], (double)b[j], s);
    return s;
}

// One wavefront finishes ONE sum over 256 values in block_sum's order, without a barrier: lane l stands for the threads l, l + 64,
// l + 128 and l + 192 of the tree.  v[t] += v[t + 128] gives (l, l + 128) and (l + 64, l + 192), v[t] += v[t + 64] adds the two, the
// shuffles are block_sum's.  Lane 0 returns the sum.
template <class F>
__device__ __forceinline__ double wave_tree(F&& value_of) {
    const int l = threadIdx.x & 63;
    const double a = value_of(l) + value_of(l + 128);
    const double b = value_of(l + 64) + value_of(l + 192);
    double w = a + b;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) w += __shfl_down(w, s, 64);
    return w;
}

// out[i] (LDS) = sum_partials(part + i * gp, groups) for i < k: wavefront v takes the sums v, v + 4, ...; one barrier in all.
__device__ __forceinline__ void finish_sums(const double* part, int64_t gp, int64_t groups, int k, double* out) {
    const int wave = threadIdx.x >> 6;
    for (int i = wave; i < k; i += kKrylovThreads / 64) {
        const double* p = part + (int64_t)i * gp;
        const double w = wave_tree([&](int t) {
            double s = 0.0;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (4 * t + j < groups) s += p[4 * t + j];
            return s;
        });
        if ((threadIdx.x & 63) == 0) out[i] = w;
    }
    __syncthreads();
}

// part[i * gp + workgroup] = this workgroup's partial of (V + i * ld, w) for i < k, kGmresDotTile sums per pass over the chunks: w's
// four floats are loaded once per chunk and pass.  sh: kGmresDotTile * 256 doubles.
__device__ __forceinline__ void multi_dot_pass(const float* V, int64_t ld, int k, const float* w, int64_t n, double* part, int64_t gp, double* sh) {
    const int t = threadIdx.x, wave = t >> 6;
    for (int i0 = 0; i0 < k; i0 += T) {
        double acc[T];
#pragma unroll
        for (int u = 0; u < T; ++u) acc[u] = 0.0;
        for_chunks(n, [&](int64_t i, int m) {
            float vw[4];
            ld4(w, i, m, vw);
#pragma unroll
            for (int u = 0; u < T; ++u)
                if (i0 + u < k) {
                    float vv[4];
                    ld4(V + (int64_t)(i0 + u) * ld, i, m, vv);
                    acc[u] += dot4_fma(vv, vw, m);
                }
        });
#pragma unroll
        for (int u = 0; u < T; ++u) sh[u * kKrylovThreads + t] = acc[u];
        __syncthreads();
        for (int u = wave; u < T && i0 + u < k; u += kKrylovThreads / 64) {
            const double* v = sh + u * kKrylovThreads;
            const double s = wave_tree([&](int tt) { return v[tt]; });
            if ((t & 63) == 0) part[(int64_t)(i0 + u) * gp + blockIdx.x] = s;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kKrylovThreads) void gmres_multi_dot_kernel(const float* V, int64_t ld, int k, const float* w, int64_t n, double* part,
                                                                         int64_t gp, const double* s_in) {
    __shared__ double sh[T * kKrylovThreads];
    if (s_in && frozen(s_in)) return;
    multi_dot_pass(V, ld, k, w, n, part, gp, sh);
}

__global__ __launch_bounds__(kKrylovThreads) void gmres_dot_finish_kernel(const double* part, int64_t gp, int64_t groups, int k, double* out) {
    __shared__ double sums[kGmresMaxBasis + 1];
    finish_sums(part, gp, groups, k, sums);
    if ((int)threadIdx.x < k) out[threadIdx.x] = sums[threadIdx.x];
}

// The start of a cycle, behind r = b - A x (in basis slot 0) and the partials of (r, r).  first: the block from nothing, as
// krylov_init_kernel builds it.  rr not finite: breakdown; rr <= rtol^2 bb: done; else v_0 = f32(1 / sqrt(rr)) r and g_res[0] = sqrt(rr).
// BS (here and in the rotate and close kernels): 0 = k.minv is an inverse diagonal, the text these kernels had before they took a block
// size; else the block size of a block-Jacobi buffer whose block area k.minv is (hispmv_block_jacobi_device.h).
template <int BS>
__global__ __launch_bounds__(kKrylovThreads) void gmres_open_kernel(GmresStep k) {
    __shared__ double sh[kKrylovThreads];
    double S[kKrylovState];
    const int64_t g = groups_of(k.n);
    bool zero_x = false;
    if (k.first) {
        const double b2 = sum_partials(k.part_b2, g, sh);
        krylov_rule_init(S, b2, b2, k.products, zero_x);
    } else {
        load_state(k.s_in, S);
    }
    bool act = false;
    float inv32 = 0.0f;
    if (!frozen(S)) {
        const double rr = sum_partials(k.part_rr, g, sh);
        S[kKsRr] = rr;
        if (!finite_d(rr)) S[kKsBreakdown] = 1.0;
        else if (rr <= k.tol2 * S[kKsBb]) S[kKsDone] = 1.0;
        else {
            const double beta = sqrt(rr);
            inv32 = (float)(1.0 / beta);
            act = true;
            S[kGsCols] = 0.0; S[kGsJ] = 0.0;
            if (blockIdx.x == 0 && threadIdx.x == 0) k.g_res[0] = beta;
        }
    }
    store_state(k.s_out, S);
    if (zero_x)
        for_chunks(k.n, [&](int64_t i, int m) {
            const float zero[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            st4(k.x, i, m, zero);
        });
    if (!act) return;
    for_chunks(k.n, [&](int64_t i, int m) {
        float r[4];
        ld4(k.V, i, m, r);
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = inv32 * r[e];
        st4(k.V, i, m, r);
        if (k.minv) {
            float d[4];
            if constexpr (BS == 0) {
                ld4(k.minv, i, m, d);
#pragma unroll
                for (int e = 0; e < 4; ++e) d[e] = d[e] * r[e];
            } else {
                block_jacobi_mul4<BS>(k.minv, i, m, r, d);
            }
            st4(k.z, i, m, d);
        }
    });
}

// One pass of classical Gram-Schmidt on w = basis vector j + 1: the sums h_i = (v_i, w), i <= j, from the partials the kernel before
// wrote; any not finite: breakdown, nothing written.  w = w - f32(h_i) v_i for i ascending.  Pass 1 then writes the partials of
// (v_i, w) for pass 2 over the elements it holds, and workgroup 0 stores h1; pass 2 writes the partials of (w, w) and h = h1 + h2.
__global__ __launch_bounds__(kKrylovThreads) void gmres_sub_kernel(GmresStep k) {
    __shared__ double sh[T * kKrylovThreads];
    __shared__ double hs[kGmresMaxBasis + 1];
    double S[kKrylovState];
    load_state(k.s_in, S);
    if (frozen(S)) {
        store_state(k.s_out, S);
        return;
    }
    const int cnt = k.j + 1, t = threadIdx.x;
    finish_sums(k.parts_in, k.gp, groups_of(k.n), cnt, hs);
    bool ok = true;
    for (int i = 0; i < cnt; ++i) ok = ok && finite_d(hs[i]);
    if (!ok) S[kKsBreakdown] = 1.0;
    store_state(k.s_out, S);
    if (!ok) return;
    if (blockIdx.x == 0 && t < cnt) {
        if (k.second) k.h[t] = k.h1[t] + hs[t];
        else k.h1[t] = hs[t];
    }
    float* w = k.V + (int64_t)cnt * k.stride;
    double acc_ww = 0.0;
    for_chunks(k.n, [&](int64_t i, int m) {
        float vw[4];
        ld4(w, i, m, vw);
#pragma unroll 4
        for (int b = 0; b < cnt; ++b) {
            float vv[4];
            ld4(k.V + (int64_t)b * k.stride, i, m, vv);
            const float h32 = (float)hs[b];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float hv = h32 * vv[e];
                vw[e] = vw[e] - hv;
            }
        }
        st4(w, i, m, vw);
        if (k.second) acc_ww += dot4_fma(vw, vw, m);
    });
    if (k.second) {
        const double ww = block_sum(acc_ww, sh);
        if (t == 0) k.part_ww[blockIdx.x] = ww;
    } else {
        // every thread reads back only the elements of w it stored itself
        multi_dot_pass(k.V, k.stride, cnt, w, k.n, k.parts_out, k.gp, sh);
    }
}

// The Givens step of column j, by every thread from the same words: the earlier rotations on h, the new one from h_j and
// hn = sqrt((w, w)), g_fin[j] and g_res[j + 1], the stopping rule on g_res[j + 1]^2; then v_{j+1} = f32(1 / hn) w in place and, with
// minv, z = minv v_{j+1}.
template <int BS>
__global__ __launch_bounds__(kKrylovThreads) void gmres_rotate_kernel(GmresStep k) {
    __shared__ double sh[kKrylovThreads];
    __shared__ double cs[kGmresMaxRestart], ss[kGmresMaxRestart], hh[kGmresMaxBasis + 1];
    double S[kKrylovState];
    load_state(k.s_in, S);
    if (frozen(S)) {
        store_state(k.s_out, S);
        return;
    }
    const int j = k.j, t = threadIdx.x;
    const bool writer = blockIdx.x == 0 && t == 0;
    if (t < j) { cs[t] = k.c[t]; ss[t] = k.s[t]; }
    if (t <= j) hh[t] = k.h[t];
    const double ww = sum_partials(k.part_ww, groups_of(k.n), sh);          // its barriers publish cs, ss, hh
    bool act = false;
    float inv32 = 0.0f;
    if (!finite_d(ww)) {
        S[kKsBreakdown] = 1.0;
    } else {
        const double hn = sqrt(ww);
        double hj = hh[0];
        for (int i = 0; i < j; ++i) {
            const double next = hh[i + 1];
            const double top = cs[i] * hj + ss[i] * next;
            const double low = cs[i] * next - ss[i] * hj;
            if (writer) k.R[i * kGmresMaxRestart + j] = top;
            hj = low;
        }
        const double d = sqrt(hj * hj + hn * hn);
        if (bad(d)) {
            S[kKsBreakdown] = 1.0;
        } else {
            const double c = hj / d, s = hn / d, g = k.g_res[j];
            const double fin = c * g, res = -(s * g);
            if (writer) {
                k.c[j] = c; k.s[j] = s; k.R[j * kGmresMaxRestart + j] = d; k.g_fin[j] = fin; k.g_res[j + 1] = res;
            }
            S[kGsJ] = (double)j; S[kGsCols] = (double)(j + 1); S[kKsIters] += 1.0;
            const double rr = res * res;
            S[kKsRr] = rr;
            if (rr <= k.tol2 * S[kKsBb]) S[kKsDone] = 1.0;
            else {
                act = true;
                inv32 = (float)(1.0 / hn);
            }
        }
    }
    store_state(k.s_out, S);
    if (!act) return;
    float* w = k.V + (int64_t)(j + 1) * k.stride;
    for_chunks(k.n, [&](int64_t i, int m) {
        float v[4];
        ld4(w, i, m, v);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = inv32 * v[e];
        st4(w, i, m, v);
        if (k.minv) {
            float d[4];
            if constexpr (BS == 0) {
                ld4(k.minv, i, m, d);
#pragma unroll
                for (int e = 0; e < 4; ++e) d[e] = d[e] * v[e];
            } else {
                block_jacobi_mul4<BS>(k.minv, i, m, v, d);
            }
            st4(k.z, i, m, d);
        }
    });
}

// The close of a cycle: acts once, and only on the cols completed columns -- also of a solve that froze inside the cycle.  Thread 0 of
// every workgroup solves R y = g_fin by back substitution from the same words; u = sum f32(y_i) v_i; x += minv u (or u).
template <int BS>
__global__ __launch_bounds__(kKrylovThreads) void gmres_close_kernel(GmresStep k) {
    __shared__ double Rs[kGmresMaxRestart * kGmresMaxRestart];
    __shared__ double gs[kGmresMaxRestart], y[kGmresMaxRestart];
    __shared__ float y32[kGmresMaxRestart];
    double S[kKrylovState];
    load_state(k.s_in, S);
    const int cols = (int)S[kGsCols], t = threadIdx.x;
    S[kGsCols] = 0.0;
    store_state(k.s_out, S);
    if (cols <= 0 || cols > kGmresMaxRestart) return;
    for (int e = t; e < cols * cols; e += kKrylovThreads) {
        const int i = e / cols, c = e % cols;
        if (c >= i) Rs[i * kGmresMaxRestart + c] = k.R[i * kGmresMaxRestart + c];
    }
    if (t < cols) gs[t] = k.g_fin[t];
    __syncthreads();
    if (t == 0)
        for (int i = cols - 1; i >= 0; --i) {
            double s = gs[i];
            for (int c = i + 1; c < cols; ++c) s = s - Rs[i * kGmresMaxRestart + c] * y[c];
            const double yi = s / Rs[i * kGmresMaxRestart + i];
            y[i] = yi;
            y32[i] = (float)yi;
        }
    __syncthreads();
    for_chunks(k.n, [&](int64_t i, int m) {
        float u[4], v[4], x[4];
        ld4(k.V, i, m, v);
        const float y0 = y32[0];
#pragma unroll
        for (int e = 0; e < 4; ++e) u[e] = y0 * v[e];
#pragma unroll 4
        for (int b = 1; b < cols; ++b) {
            ld4(k.V + (int64_t)b * k.stride, i, m, v);
            const float yb = y32[b];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float yv = yb * v[e];
                u[e] = u[e] + yv;
            }
        }
        if (k.minv) {
            float d[4];
            if constexpr (BS == 0) {
                ld4(k.minv, i, m, d);
#pragma unroll
                for (int e = 0; e < 4; ++e) u[e] = d[e] * u[e];
            } else {
                block_jacobi_mul4<BS>(k.minv, i, m, u, d);
#pragma unroll
                for (int e = 0; e < 4; ++e) u[e] = d[e];
            }
        }
        ld4(k.x, i, m, x);
#pragma unroll
        for (int e = 0; e < 4; ++e) x[e] = x[e] + u[e];
        st4(k.x, i, m, x);
    });
}

}  // namespace

hipError_t launch_gmres_multi_dot(const float* V, int64_t ld, int64_t k, const float* w, int64_t n, double* part, int64_t gp, const double* s_in,
                                  hipStream_t s) {
    if (n <= 0 || k <= 0) return hipSuccess;
    hipLaunchKernelGGL(gmres_multi_dot_kernel, dim3(grid_of(n)), dim3(kKrylovThreads), 0, s, V, ld, (int)k, w, n, part, gp, s_in);
    return hipGetLastError();
}
hipError_t launch_gmres_dot_finish(const double* part, int64_t gp, int64_t groups, int64_t k, double* out, hipStream_t s) {
    hipLaunchKernelGGL(gmres_dot_finish_kernel, dim3(1), dim3(kKrylovThreads), 0, s, part, gp, groups, (int)k, out);
    return hipGetLastError();
}

#define GMRES_LAUNCH(kernel)                                                                    \
    hipLaunchKernelGGL(kernel, dim3(grid_of(k.n)), dim3(kKrylovThreads), 0, s, k);                  \
    return hipGetLastError();

// the BS instantiation of one of the three kernels that precondition
#define GMRES_LAUNCH_BS(kernel)                                                                  \
    switch (bs) {                                                                                \
        case 0: { GMRES_LAUNCH(kernel<0>) }                                                      \
        case 4: { GMRES_LAUNCH(kernel<4>) }                                                      \
        case 8: { GMRES_LAUNCH(kernel<8>) }                                                      \
        case 16: { GMRES_LAUNCH(kernel<16>) }                                                    \
        case 32: { GMRES_LAUNCH(kernel<32>) }                                                    \
        default: return hipErrorInvalidValue;                                                    \
    }

hipError_t launch_gmres_open(const GmresStep& k, hipStream_t s, int bs) { GMRES_LAUNCH_BS(gmres_open_kernel) }
hipError_t launch_gmres_sub(const GmresStep& k, hipStream_t s) { GMRES_LAUNCH(gmres_sub_kernel) }
hipError_t launch_gmres_rotate(const GmresStep& k, hipStream_t s, int bs) { GMRES_LAUNCH_BS(gmres_rotate_kernel) }
hipError_t launch_gmres_close(const GmresStep& k, hipStream_t s, int bs) { GMRES_LAUNCH_BS(gmres_close_kernel) }

}  // namespace hispmv
