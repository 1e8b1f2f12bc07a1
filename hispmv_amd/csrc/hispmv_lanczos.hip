// hispmv_lanczos.hip -- the kernels the thick-restart solvers, Lanczos and Golub-Kahan, add to hispmv_gmres.hip's (hispmv_lanczos.h;
// include/hispmv.h: "Lanczos / eigsh", "Golub-Kahan / svds").  lanczos_open and basis_record run on the Krylov grid of their basis's
// length with its chunk order and its fixed-order fp64 sums: fp32 vectors, unfused (-ffp-contract=off), scalars fp64 and rounded once
// to fp32 before they meet a vector; every workgroup finishes the sums it needs itself, only workgroup 0 writes Hc, the alphas, the
// betas and the scalar block.  basis_rotate is the restart: a tall-skinny product V[:, :k] <- V[:, :m] Y that may run in place, lanes
// along the elements.
#include <hip/hip_runtime.h>

#include "hispmv_krylov_device.h"
#include "hispmv_krylov_scalar.h"
#include "hispmv_lanczos.h"

namespace hispmv {
namespace {

// The block from nothing behind the partials of (v0, v0): a sum that is zero or not finite is a breakdown, and slot 0 then holds the
// plain copy of v0; otherwise V_0 = f32(1 / sqrt((v0, v0))) * v0.
__global__ __launch_bounds__(kKrylovThreads) void lanczos_open_kernel(RecordStep k) {
    __shared__ double sh[kKrylovThreads];
    double S[kKrylovState];
#pragma unroll
    for (int i = 0; i < kKrylovState; ++i) S[i] = 0.0;
    const double vv = sum_partials(k.part, groups_of(k.n), sh);
    S[kKsRr] = vv;
    const bool act = !bad(vv);
    if (!act) S[kKsBreakdown] = 1.0;
    const float inv32 = act ? (float)(1.0 / sqrt(vv)) : 0.0f;
    store_state(k.s_out, S);
    for_chunks(k.n, [&](int64_t i, int m) {
        float v[4];
        ld4(k.v0, i, m, v);
        if (act) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = inv32 * v[e];
        }
        st4(k.V, i, m, v);
    });
}

// The end of one step's work on a basis, behind pass 2 of the subtract-and-dot kernel (Golub-Kahan's U side, j = 0: behind the dot
// kernel): ww = (w, w) from its partials, not finite: breakdown.  The rule ww <= tiny^2 * (ww + sum h_i^2) by every thread from the
// same words.  What RULE decides (hispmv_lanczos.h: RecordRule): where w lies and how many coefficients the step has -- U side: slot j
// and j of them, otherwise slot j + 1 and j + 1; what workgroup 0 records -- column j of Hc (not the V side), alpha_j = sqrt(ww) on the
// U side unless the rule holds, beta_j = sqrt(ww) otherwise; and the block's words -- U side: only where the rule holds, which there
// closes the space: steps = j, one more product, invariant and closed_u; otherwise steps = j + 1, one more product (the V side: two),
// and the rule is the invariant subspace rule.  Where the rule does not hold w = f32(1 / sqrt(ww)) * w in place.
template <RecordRule RULE>
__global__ __launch_bounds__(kKrylovThreads) void basis_record_kernel(RecordStep k) {
    constexpr bool U = RULE == kRecordGkU;
    __shared__ double sh[kKrylovThreads];
    __shared__ double hh[kLanczosMaxNcv + 1];
    double S[kKrylovState];
    load_state(k.s_in, S);
    if (frozen(S)) {
        store_state(k.s_out, S);
        return;
    }
    const int j = k.j, t = threadIdx.x, cnt = U ? j : j + 1;
    if (t < cnt) hh[t] = k.h[t];
    const double ww = sum_partials(k.part, groups_of(k.n), sh);          // its barriers publish hh
    if (!finite_d(ww)) {
        S[kKsBreakdown] = 1.0;
        store_state(k.s_out, S);
        return;
    }
    const double nrm = sqrt(ww);
    double hsq = 0.0;
    for (int i = 0; i < cnt; ++i) {
        const double sq = hh[i] * hh[i];
        hsq = hsq + sq;
    }
    const bool closed = ww <= kLanczosTiny2 * (ww + hsq);
    if (blockIdx.x == 0) {
        if (RULE != kRecordGkV && t < cnt) k.Hc[(int64_t)j * kLanczosHcLd + t] = hh[t];
        if (U) {
            if (t == 0 && !closed) k.alpha[j] = nrm;
        } else if (t == 0) {
            k.beta[j] = nrm;
        }
    }
    S[kKsRr] = ww;
    if (U) {
        if (closed) { S[kKsProducts] += 1.0; S[kLsSteps] = (double)j; S[kLsClosedU] = 1.0; }
    } else {
        S[kKsProducts] += RULE == kRecordGkV ? 2.0 : 1.0; S[kLsSteps] = (double)(j + 1);
    }
    if (closed) { S[kLsInvariant] = 1.0; S[kKsDone] = 1.0; }
    store_state(k.s_out, S);
    if (closed) return;
    const float inv32 = (float)(1.0 / nrm);
    float* w = k.V + (int64_t)(U ? j : j + 1) * k.stride;
    for_chunks(k.n, [&](int64_t i, int m) {
        float v[4];
        ld4(w, i, m, v);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = inv32 * v[e];
        st4(w, i, m, v);
    });
}

// out[c][e] = sum_{i < m} Yt[c][i] * V[i][e].  A wavefront serves 64 * kRotateElems elements: a lane owns kRotateElems of them, 64 apart,
// so every load and store of a wavefront is 64 consecutive floats whatever the alignment and ld; it holds all m inputs of its
// elements in registers before it stores the first output, which is what lets out be V.  W = 1: the four wavefronts of a workgroup
// serve four element groups, every column each.  W = 4 (a small n, where one wavefront's chain of k * m multiply-adds is the whole
// run time): the four wavefronts serve ONE element group and take the columns c = wave, wave + 4, ...; each loads all inputs, and a
// barrier stands between the last load and the first store of the workgroup.  Yt is read through uniform (scalar) loads: it aliases
// nothing the kernel writes.  MMAX: the register array's size, m <= MMAX -- a smaller basis takes fewer registers.
template <int MMAX, int W>
__global__ __launch_bounds__(kRotateThreads) void basis_rotate_kernel(const float* V, int64_t ld_v, int m, int k, const float* __restrict__ Yt,
                                                                       float* out, int64_t ld_out, int64_t n, const float* xsrc, float* xdst) {
    constexpr int E = kRotateElems, G = kRotateGroup, WAVES = kRotateThreads / 64;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));          // uniform, and known to be
    const int group = W == 1 ? wave : 0, first = W == 1 ? 0 : wave;
    const int64_t e0 = ((int64_t)blockIdx.x * (WAVES / W) + group) * (64 * E) + lane;
    const bool copies = xdst != nullptr && first == 0;
    float v[MMAX][E], x[E];
#pragma unroll
    for (int i = 0; i < MMAX; ++i)
#pragma unroll
        for (int u = 0; u < E; ++u) {
            const int64_t e = e0 + (int64_t)u * 64;
            v[i][u] = (i < m && e < n) ? V[(int64_t)i * ld_v + e] : 0.0f;
        }
    if (copies) {
#pragma unroll
        for (int u = 0; u < E; ++u) {
            const int64_t e = e0 + (int64_t)u * 64;
            x[u] = e < n ? xsrc[e] : 0.0f;
        }
    }
    if (W > 1) __syncthreads();          // every wavefront of the workgroup holds its inputs: the stores below may land on them
    for (int c = first; c < k; c += W) {
        const float* y = Yt + (int64_t)c * m;
        float acc[E];
#pragma unroll
        for (int u = 0; u < E; ++u) acc[u] = 0.0f;
        // the coefficients kRotateGroup at a time where a whole group lies below m: one wide uniform load and no branch between the
        // multiply-adds it feeds; the last, partial group one by one
#pragma unroll
        for (int i0 = 0; i0 < MMAX; i0 += G) {
            if (i0 + G <= m) {
                float yy[G];
#pragma unroll
                for (int g = 0; g < G; ++g) yy[g] = y[i0 + g];
#pragma unroll
                for (int g = 0; g < G; ++g)
                    if (i0 + g < MMAX) {
#pragma unroll
                        for (int u = 0; u < E; ++u) {
                            const float p = yy[g] * v[i0 + g][u];
                            acc[u] = acc[u] + p;
                        }
                    }
            } else {
#pragma unroll
                for (int g = 0; g < G; ++g)
                    if (i0 + g < MMAX && i0 + g < m) {
                        const float yi = y[i0 + g];
#pragma unroll
                        for (int u = 0; u < E; ++u) {
                            const float p = yi * v[i0 + g][u];
                            acc[u] = acc[u] + p;
                        }
                    }
            }
        }
#pragma unroll
        for (int u = 0; u < E; ++u) {
            const int64_t e = e0 + (int64_t)u * 64;
            if (e < n) out[(int64_t)c * ld_out + e] = acc[u];
        }
    }
    if (copies) {
#pragma unroll
        for (int u = 0; u < E; ++u) {
            const int64_t e = e0 + (int64_t)u * 64;
            if (e < n) xdst[e] = x[u];
        }
    }
}

}  // namespace

hipError_t launch_lanczos_open(const RecordStep& k, hipStream_t s) {
    hipLaunchKernelGGL(lanczos_open_kernel, dim3(grid_of(k.n)), dim3(kKrylovThreads), 0, s, k);
    return hipGetLastError();
}
hipError_t launch_basis_record(const RecordStep& k, RecordRule rule, hipStream_t s) {
    void (*const kernels[])(RecordStep) = {basis_record_kernel<kRecordLanczos>, basis_record_kernel<kRecordGkU>, basis_record_kernel<kRecordGkV>};
    hipLaunchKernelGGL(kernels[rule], dim3(grid_of(k.n)), dim3(kKrylovThreads), 0, s, k);
    return hipGetLastError();
}

#define ROTATE_LAUNCH(MMAX)                                                                                                                          \
    if (split) {                                                                                                                                      \
        hipLaunchKernelGGL((basis_rotate_kernel<MMAX, 4>), dim3(grid), dim3(kRotateThreads), 0, s, V, ld_v, m, k, Yt, out, ld_out, n, xsrc, xdst);          \
    } else {                                                                                                                                          \
        hipLaunchKernelGGL((basis_rotate_kernel<MMAX, 1>), dim3(grid), dim3(kRotateThreads), 0, s, V, ld_v, m, k, Yt, out, ld_out, n, xsrc, xdst);          \
    }                                                                                                                                                 \
    return hipGetLastError();

hipError_t launch_basis_rotate(const float* V, int64_t ld_v, int m, int k, const float* Yt, float* out, int64_t ld_out, int64_t n, const float* xsrc,
                               float* xdst, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (m < 1 || m > kRotateMaxIn || k < 1 || k > kRotateMaxOut) return hipErrorInvalidValue;
    // below kRotateSplitBelow elements the columns are split over the four wavefronts of a workgroup, which then serves a quarter of
    // the elements: the same bits, four times as many workgroups, a quarter of the chain
    const bool split = n < kRotateSplitBelow && k > 1;
    const int64_t per = (int64_t)64 * kRotateElems * (split ? 1 : kRotateThreads / 64);
    const unsigned grid = (unsigned)((n + per - 1) / per);
    if (m <= 16) { ROTATE_LAUNCH(16) }
    if (m <= 32) { ROTATE_LAUNCH(32) }
    if (m <= 48) { ROTATE_LAUNCH(48) }
    ROTATE_LAUNCH(kRotateMaxIn)
}

}  // namespace hispmv
