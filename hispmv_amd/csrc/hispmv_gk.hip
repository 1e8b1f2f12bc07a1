// hispmv_gk.hip -- the kernel thick-restart Golub-Kahan bidiagonalisation adds to hispmv_gmres.hip's and hispmv_lanczos.hip's
// (hispmv_gk.h; include/hispmv.h: "Golub-Kahan / svds").  gk_record runs on the Krylov grid of its side's length with its chunk order
// and its fixed-order fp64 sums: fp32 vectors, unfused (-ffp-contract=off), scalars fp64 and rounded once to fp32 before they meet a
// vector; every workgroup finishes the sums it needs itself, only workgroup 0 writes Gc, the alphas, the betas and the scalar block.
#include <hip/hip_runtime.h>

#include "hispmv_gk.h"
#include "hispmv_krylov_device.h"
#include "hispmv_krylov_scalar.h"

namespace hispmv {
namespace {

// The end of one side of step j, behind pass 2 of the subtract-and-dot kernel (U side, j = 0: behind the dot kernel): ww = (w, w) from
// its partials, not finite: breakdown.  The rule ww <= tiny^2 * (ww + sum g_i^2) by every thread from the same words.
// SIDE 0: w = U slot j, j coefficients; column j of Gc and alpha_j = sqrt(ww) by workgroup 0; the rule closes the space: steps = j, one
// more product, invariant and closed_u.  SIDE 1: w = V slot j + 1, j + 1 coefficients; beta_j = sqrt(ww), steps = j + 1, two more
// products; the rule is Lanczos's invariant rule.  Otherwise w = f32(1 / sqrt(ww)) * w in place.
template <int SIDE>
__global__ __launch_bounds__(kKrylovThreads) void gk_record_kernel(GkStep k) {
    __shared__ double sh[kKrylovThreads];
    __shared__ double gg[kGkMaxNcv + 1];
    double S[kKrylovState];
    load_state(k.s_in, S);
    if (frozen(S)) {
        store_state(k.s_out, S);
        return;
    }
    const int j = k.j, t = threadIdx.x, cnt = SIDE == 0 ? j : j + 1;
    if (t < cnt) gg[t] = k.g[t];
    const double ww = sum_partials(k.part, groups_of(k.n), sh);          // its barriers publish gg
    if (!finite_d(ww)) {
        S[kKsBreakdown] = 1.0;
        store_state(k.s_out, S);
        return;
    }
    const double nrm = sqrt(ww);
    double gsq = 0.0;
    for (int i = 0; i < cnt; ++i) {
        const double sq = gg[i] * gg[i];
        gsq = gsq + sq;
    }
    const bool closed = ww <= kLanczosTiny2 * (ww + gsq);
    if (blockIdx.x == 0) {
        if (SIDE == 0) {
            if (t < cnt) k.Gc[(int64_t)j * kGkGcLd + t] = gg[t];
            if (t == 0 && !closed) k.alpha[j] = nrm;
        } else if (t == 0) {
            k.beta[j] = nrm;
        }
    }
    S[kKsRr] = ww;
    if (SIDE == 0) {
        if (closed) { S[kKsProducts] += 1.0; S[kGkSteps] = (double)j; S[kGkClosedU] = 1.0; }
    } else {
        S[kKsProducts] += 2.0; S[kGkSteps] = (double)(j + 1);
    }
    if (closed) { S[kGkInvariant] = 1.0; S[kKsDone] = 1.0; }
    store_state(k.s_out, S);
    if (closed) return;
    const float inv32 = (float)(1.0 / nrm);
    float* w = k.W + (int64_t)(SIDE == 0 ? j : j + 1) * k.stride;
    for_chunks(k.n, [&](int64_t i, int m) {
        float v[4];
        ld4(w, i, m, v);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = inv32 * v[e];
        st4(w, i, m, v);
    });
}

}  // namespace

hipError_t launch_gk_record(const GkStep& k, int side, hipStream_t s) {
    if (side == 0) hipLaunchKernelGGL(gk_record_kernel<0>, dim3(grid_of(k.n)), dim3(kKrylovThreads), 0, s, k);
    else hipLaunchKernelGGL(gk_record_kernel<1>, dim3(grid_of(k.n)), dim3(kKrylovThreads), 0, s, k);
    return hipGetLastError();
}

}  // namespace hispmv
