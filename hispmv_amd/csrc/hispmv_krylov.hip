// hispmv_krylov.hip -- the vector kernels of the Krylov layer (hispmv_krylov.h; include/hispmv.h: hispmv_dot_device, hispmv_cg_device,
// hispmv_bicgstab_device, hispmv_cgls_device).  Pure streams: a workgroup of 256 threads takes chunks of 1024 elements, chunk g, g + G,
// ... ascending for workgroup g of G = krylov_groups(n); a thread owns 4 consecutive floats of a chunk (one 16-byte access where that
// vector is 16-byte aligned and the chunk is whole, 4-byte accesses otherwise).  Vector arithmetic is fp32 and unfused
// (-ffp-contract=off); every scalar is fp64, computed by every workgroup itself from the same partials, hence with the same bits, and
// rounded once to fp32 before it meets a vector.  No atomics, no tickets: a dot product's partials are summed by the NEXT kernel,
// which hands the sums to the scalar rule of hispmv_krylov_scalar.h: the arithmetic of every scalar is written there.
#include <hip/hip_runtime.h>

#include "hispmv_block_jacobi_device.h"
#include "hispmv_krylov.h"
#include "hispmv_krylov_device.h"
#include "hispmv_krylov_scalar.h"

namespace hispmv {
namespace {

__device__ __forceinline__ const double* slot_of(const KrylovStep& k, int slot) { return k.parts + (int64_t)slot * kKrylovMaxGroups; }
__device__ __forceinline__ double* slot_out(const KrylovStep& k, int slot) { return k.parts + (int64_t)slot * kKrylovMaxGroups; }

__global__ __launch_bounds__(kKrylovThreads) void krylov_dot_kernel(const float* a, const float* b, int64_t n, double* part) {
    __shared__ double sh[kKrylovThreads];
    double acc = 0.0;
    for_chunks(n, [&](int64_t i, int m) {
        float va[4], vb[4];
        ld4(a, i, m, va);
        ld4(b, i, m, vb);
        acc += dot4(va, vb, m);
    });
    const double s = block_sum(acc, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(kKrylovThreads) void krylov_dot_finish_kernel(const double* part, int64_t groups, double* out) {
    __shared__ double sh[kKrylovThreads];
    const double s = sum_partials(part, groups, sh);
    if (threadIdx.x == 0) out[0] = s;
}

// The first kernel of a solve, behind the products that give src (the residual; CGLS: A^T of it): the scalar block from nothing.
// BS (here and in the CG update and the direction kernel): 0 = k.minv is the inverse diagonal, the text these kernels had before they
// took a block size; else the block size of a block-Jacobi buffer whose block area k.minv is (hispmv_block_jacobi_device.h).
template <int BS>
__global__ __launch_bounds__(kKrylovThreads) void krylov_init_kernel(KrylovStep k) {
    __shared__ double sh[kKrylovThreads];
    double S[kKrylovState];
    const double b2 = sum_partials(slot_of(k, kSlotB2), groups_of(k.n2), sh);
    const double bb = k.slot_bb == kSlotB2 ? b2 : sum_partials(slot_of(k, k.slot_bb), groups_of(k.n), sh);
    bool zero_x = false;
    krylov_rule_init(S, b2, bb, k.products, zero_x);
    store_state(k.s_out, S);
    double acc_rr = 0.0, acc_rz = 0.0;
    for_chunks(k.n, [&](int64_t i, int m) {
        float r[4], z[4];
        ld4(k.r, i, m, r);
        if (k.minv) {
            if constexpr (BS == 0) {
                float d[4];
                ld4(k.minv, i, m, d);
#pragma unroll
                for (int j = 0; j < 4; ++j) z[j] = d[j] * r[j];
            } else {
                block_jacobi_mul4<BS>(k.minv, i, m, r, z);
            }
            acc_rz += dot4(r, z, m);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) z[j] = r[j];
        }
        acc_rr += dot4(r, r, m);
        st4(k.p, i, m, z);
        if (k.rhat) st4(k.rhat, i, m, r);
        if (zero_x) {
            const float zero[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            st4(k.x, i, m, zero);
        }
    });
    const double rr = block_sum(acc_rr, sh);
    if (threadIdx.x == 0) slot_out(k, kSlotRr)[blockIdx.x] = rr;
    if (k.minv) {
        const double rz = block_sum(acc_rz, sh);
        if (threadIdx.x == 0) slot_out(k, kSlotRho)[blockIdx.x] = rz;
    }
}

// The dot pass behind a product.  first: rr and rho of the initial residual still lie in their partials (over n2 elements); they are
// summed here and the stopping rule sees the initial residual.
__global__ __launch_bounds__(kKrylovThreads) void krylov_step_dot_kernel(KrylovStep k) {
    __shared__ double sh[kKrylovThreads];
    double S[kKrylovState];
    load_state(k.s_in, S);
    if (k.first && !frozen(S)) {
        const double rr = sum_partials(slot_of(k, kSlotRr), groups_of(k.n2), sh);
        const double rho = k.slot_rho == kSlotRr ? rr : sum_partials(slot_of(k, k.slot_rho), groups_of(k.n2), sh);
        krylov_rule_first(S, rr, rho, k.tol2);
    }
    store_state(k.s_out, S);
    double acc1 = 0.0, acc2 = 0.0;
    for_chunks(k.n, [&](int64_t i, int m) {
        float a[4], b[4];
        ld4(k.a1, i, m, a);
        ld4(k.b1, i, m, b);
        acc1 += dot4(a, b, m);
        if (k.a2) {
            ld4(k.a2, i, m, a);
            ld4(k.b2, i, m, b);
            acc2 += dot4(a, b, m);
        }
    });
    const double s1 = block_sum(acc1, sh);
    if (threadIdx.x == 0) slot_out(k, k.slot1)[blockIdx.x] = s1;
    if (k.a2) {
        const double s2 = block_sum(acc2, sh);
        if (threadIdx.x == 0) slot_out(k, k.slot2)[blockIdx.x] = s2;
    }
}

// CG: alpha = rho / (p, q); x += alpha p; r -= alpha q; the partials of (r, r) and, with minv, of (r, minv r)
template <int BS>
__global__ __launch_bounds__(kKrylovThreads) void krylov_cg_update_kernel(KrylovStep k) {
    __shared__ double sh[kKrylovThreads];
    double S[kKrylovState];
    load_state(k.s_in, S);
    bool act = false;
    float a32 = 0.0f;
    if (!frozen(S)) {
        const double den = sum_partials(slot_of(k, kSlotDen), groups_of(k.n), sh);
        act = krylov_rule_alpha<false>(S, den, a32);
    }
    store_state(k.s_out, S);
    if (!act) return;
    double acc_rr = 0.0, acc_rz = 0.0;
    for_chunks(k.n, [&](int64_t i, int m) {
        float x[4], p[4], r[4], q[4];
        ld4(k.x, i, m, x);
        ld4(k.p, i, m, p);
        ld4(k.r, i, m, r);
        ld4(k.q, i, m, q);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float ap = a32 * p[j];
            x[j] = x[j] + ap;
            const float aq = a32 * q[j];
            r[j] = r[j] - aq;
        }
        st4(k.x, i, m, x);
        st4(k.r, i, m, r);
        acc_rr += dot4(r, r, m);
        if (k.minv) {
            if constexpr (BS == 0) {
                float d[4], z[4];
                ld4(k.minv, i, m, d);
#pragma unroll
                for (int j = 0; j < 4; ++j) z[j] = d[j] * r[j];
                acc_rz += dot4(r, z, m);
            } else {
                float z[4];
                block_jacobi_mul4<BS>(k.minv, i, m, r, z);
                acc_rz += dot4(r, z, m);
            }
        }
    });
    const double rr = block_sum(acc_rr, sh);
    if (threadIdx.x == 0) slot_out(k, kSlotRr)[blockIdx.x] = rr;
    if (k.minv) {
        const double rz = block_sum(acc_rz, sh);
        if (threadIdx.x == 0) slot_out(k, kSlotRho)[blockIdx.x] = rz;
    }
}

// CG and CGLS: the stopping rule on the new rr, then beta = rho' / rho; p = z + beta p with z = minv r (or r; CGLS: s)
template <int BS>
__global__ __launch_bounds__(kKrylovThreads) void krylov_direction_kernel(KrylovStep k) {
    __shared__ double sh[kKrylovThreads];
    double S[kKrylovState];
    load_state(k.s_in, S);
    bool act = false;
    float b32 = 0.0f;
    if (!frozen(S)) {
        const double rr = sum_partials(slot_of(k, kSlotRr), groups_of(k.n), sh);
        const double rho = k.slot_rho == kSlotRr ? rr : sum_partials(slot_of(k, k.slot_rho), groups_of(k.n), sh);
        act = krylov_rule_direction(S, rr, rho, k.tol2, b32);
    }
    store_state(k.s_out, S);
    if (!act) return;
    for_chunks(k.n, [&](int64_t i, int m) {
        float r[4], p[4];
        ld4(k.r, i, m, r);
        ld4(k.p, i, m, p);
        if (k.minv) {
            if constexpr (BS == 0) {
                float d[4];
                ld4(k.minv, i, m, d);
#pragma unroll
                for (int j = 0; j < 4; ++j) r[j] = d[j] * r[j];
            } else {
                float z[4];
                block_jacobi_mul4<BS>(k.minv, i, m, r, z);
#pragma unroll
                for (int j = 0; j < 4; ++j) r[j] = z[j];
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float bp = b32 * p[j];
            p[j] = r[j] + bp;
        }
        st4(k.p, i, m, p);
    });
}

// CGLS: alpha = rho / (q, q); x += alpha p over n elements; r -= alpha q over n2
__global__ __launch_bounds__(kKrylovThreads) void krylov_cgls_update_kernel(KrylovStep k) {
    __shared__ double sh[kKrylovThreads];
    double S[kKrylovState];
    load_state(k.s_in, S);
    bool act = false;
    float a32 = 0.0f;
    if (!frozen(S)) {
        const double den = sum_partials(slot_of(k, kSlotDen), groups_of(k.n2), sh);
        act = krylov_rule_alpha<false>(S, den, a32);
    }
    store_state(k.s_out, S);
    if (!act) return;
    const int64_t nmax = k.n > k.n2 ? k.n : k.n2;
    for_chunks(nmax, [&](int64_t i, int) {
        const int mx = k.n - i >= 4 ? 4 : k.n - i > 0 ? (int)(k.n - i) : 0;
        const int mr = k.n2 - i >= 4 ? 4 : k.n2 - i > 0 ? (int)(k.n2 - i) : 0;
        if (mx > 0) {
            float x[4], p[4];
            ld4(k.x, i, mx, x);
            ld4(k.p, i, mx, p);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float ap = a32 * p[j];
                x[j] = x[j] + ap;
            }
            st4(k.x, i, mx, x);
        }
        if (mr > 0) {
            float r[4], q[4];
            ld4(k.r, i, mr, r);
            ld4(k.q, i, mr, q);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float aq = a32 * q[j];
                r[j] = r[j] - aq;
            }
            st4(k.r, i, mr, r);
        }
    });
}

// BiCGSTAB: alpha = rho / (rhat, v); s = r - alpha v, stored over r; the partials of (s, s)
__global__ __launch_bounds__(kKrylovThreads) void krylov_bicg_s_kernel(KrylovStep k) {
    __shared__ double sh[kKrylovThreads];
    double S[kKrylovState];
    load_state(k.s_in, S);
    bool act = false;
    float a32 = 0.0f;
    if (!frozen(S)) {
        const double den = sum_partials(slot_of(k, kSlotDen), groups_of(k.n), sh);
        act = krylov_rule_alpha<true>(S, den, a32);
    }
    store_state(k.s_out, S);
    if (!act) return;
    double acc = 0.0;
    for_chunks(k.n, [&](int64_t i, int m) {
        float r[4], v[4];
        ld4(k.r, i, m, r);
        ld4(k.q, i, m, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float av = a32 * v[j];
            r[j] = r[j] - av;
        }
        st4(k.r, i, m, r);
        acc += dot4(r, r, m);
    });
    const double ss = block_sum(acc, sh);
    if (threadIdx.x == 0) slot_out(k, kSlotSs)[blockIdx.x] = ss;
}

// BiCGSTAB: (s, s) within the tolerance: x += alpha p and done.  Otherwise omega = (t, s) / (t, t); x += alpha p; x += omega s;
// r = s - omega t; the partials of (r, r) and (rhat, r)
__global__ __launch_bounds__(kKrylovThreads) void krylov_bicg_x_kernel(KrylovStep k) {
    __shared__ double sh[kKrylovThreads];
    double S[kKrylovState];
    load_state(k.s_in, S);
    int act = 0;          // 1 the half step, 2 the whole
    const float a32 = (float)S[kKsAlpha];
    float w32 = 0.0f;
    if (!frozen(S)) {
        const int64_t g = groups_of(k.n);
        const double ss = sum_partials(slot_of(k, kSlotSs), g, sh);
        const double ts = sum_partials(slot_of(k, kSlotTs), g, sh);
        const double tt = sum_partials(slot_of(k, kSlotTt), g, sh);
        act = krylov_rule_bicg_omega(S, ss, ts, tt, k.tol2, w32);
    }
    store_state(k.s_out, S);
    if (!act) return;
    double acc_rr = 0.0, acc_rho = 0.0;
    for_chunks(k.n, [&](int64_t i, int m) {
        float x[4], p[4];
        ld4(k.x, i, m, x);
        ld4(k.p, i, m, p);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float ap = a32 * p[j];
            x[j] = x[j] + ap;
        }
        if (act == 2) {
            float s[4], t[4], h[4];
            ld4(k.r, i, m, s);
            ld4(k.t, i, m, t);
            ld4(k.rhat, i, m, h);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float ws = w32 * s[j];
                x[j] = x[j] + ws;
                const float wt = w32 * t[j];
                s[j] = s[j] - wt;
            }
            st4(k.r, i, m, s);
            acc_rr += dot4(s, s, m);
            acc_rho += dot4(h, s, m);
        }
        st4(k.x, i, m, x);
    });
    if (act != 2) return;
    const double rr = block_sum(acc_rr, sh);
    if (threadIdx.x == 0) slot_out(k, kSlotRr)[blockIdx.x] = rr;
    const double rho = block_sum(acc_rho, sh);
    if (threadIdx.x == 0) slot_out(k, kSlotRho)[blockIdx.x] = rho;
}

// BiCGSTAB: the stopping rule on the new rr, then beta = (rho' / rho) (alpha / omega); p = r + beta (p - omega v)
__global__ __launch_bounds__(kKrylovThreads) void krylov_bicg_p_kernel(KrylovStep k) {
    __shared__ double sh[kKrylovThreads];
    double S[kKrylovState];
    load_state(k.s_in, S);
    bool act = false;
    float b32 = 0.0f;
    const float w32 = (float)S[kKsOmega];
    if (!frozen(S)) {
        const int64_t g = groups_of(k.n);
        const double rr = sum_partials(slot_of(k, kSlotRr), g, sh);
        const double rho = sum_partials(slot_of(k, kSlotRho), g, sh);
        act = krylov_rule_bicg_beta(S, rr, rho, k.tol2, b32);
    }
    store_state(k.s_out, S);
    if (!act) return;
    for_chunks(k.n, [&](int64_t i, int m) {
        float r[4], p[4], v[4];
        ld4(k.r, i, m, r);
        ld4(k.p, i, m, p);
        ld4(k.q, i, m, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float wv = w32 * v[j];
            const float d = p[j] - wv;
            const float bd = b32 * d;
            p[j] = r[j] + bd;
        }
        st4(k.p, i, m, p);
    });
}

}  // namespace

hipError_t launch_krylov_dot(const float* a, const float* b, int64_t n, double* part, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(krylov_dot_kernel, dim3(grid_of(n)), dim3(kKrylovThreads), 0, s, a, b, n, part);
    return hipGetLastError();
}
hipError_t launch_krylov_dot_finish(const double* part, int64_t groups, double* out, hipStream_t s) {
    hipLaunchKernelGGL(krylov_dot_finish_kernel, dim3(1), dim3(kKrylovThreads), 0, s, part, groups, out);
    return hipGetLastError();
}

#define KRYLOV_LAUNCH(kernel, n_)                                                              \
    hipLaunchKernelGGL(kernel, dim3(grid_of(n_)), dim3(kKrylovThreads), 0, s, k);                  \
    return hipGetLastError();

// the BS instantiation of one of the three kernels that precondition
#define KRYLOV_LAUNCH_BS(kernel, n_)                                                                \
    switch (bs) {                                                                                   \
        case 0: { KRYLOV_LAUNCH(kernel<0>, n_) }                                                    \
        case 4: { KRYLOV_LAUNCH(kernel<4>, n_) }                                                    \
        case 8: { KRYLOV_LAUNCH(kernel<8>, n_) }                                                    \
        case 16: { KRYLOV_LAUNCH(kernel<16>, n_) }                                                  \
        case 32: { KRYLOV_LAUNCH(kernel<32>, n_) }                                                  \
        default: return hipErrorInvalidValue;                                                       \
    }

hipError_t launch_krylov_init(const KrylovStep& k, hipStream_t s, int bs) { KRYLOV_LAUNCH_BS(krylov_init_kernel, k.n) }
hipError_t launch_krylov_step_dot(const KrylovStep& k, hipStream_t s) { KRYLOV_LAUNCH(krylov_step_dot_kernel, k.n) }
hipError_t launch_krylov_cg_update(const KrylovStep& k, hipStream_t s, int bs) { KRYLOV_LAUNCH_BS(krylov_cg_update_kernel, k.n) }
hipError_t launch_krylov_direction(const KrylovStep& k, hipStream_t s, int bs) { KRYLOV_LAUNCH_BS(krylov_direction_kernel, k.n) }
hipError_t launch_krylov_cgls_update(const KrylovStep& k, hipStream_t s) { KRYLOV_LAUNCH(krylov_cgls_update_kernel, (k.n > k.n2 ? k.n : k.n2)) }
hipError_t launch_krylov_bicg_s(const KrylovStep& k, hipStream_t s) { KRYLOV_LAUNCH(krylov_bicg_s_kernel, k.n) }
hipError_t launch_krylov_bicg_x(const KrylovStep& k, hipStream_t s) { KRYLOV_LAUNCH(krylov_bicg_x_kernel, k.n) }
hipError_t launch_krylov_bicg_p(const KrylovStep& k, hipStream_t s) { KRYLOV_LAUNCH(krylov_bicg_p_kernel, k.n) }

}  // namespace hispmv
