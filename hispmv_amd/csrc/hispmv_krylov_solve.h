// hispmv_krylov_solve.h -- what the single-vector and the multi-right-hand-side Krylov entries share on the host
// (hispmv_krylov_abi.cpp, hispmv_krylov_multi_abi.cpp; hispmv_gmres_abi.cpp takes the checks, KrylovBlocks and KrylovSolve and has a
// loop of its own): the solver tables, the bookkeeping of the two scalar
// blocks, the argument checks with their texts, the owner of the pinned buffer, and krylov_run, THE order of launches of a solve.  A
// backend (the Solve struct of either file) derives from KrylovSolve and supplies its vectors, its products, its launchers and how it
// looks at the device and writes results; the workspace layouts stay beside their backend.
#pragma once
#include <cmath>
#include <utility>

#include "hispmv_ctx.h"
#include "hispmv_krylov.h"

namespace hispmv {

// per solver HISPMV_KRYLOV_CG, _BICGSTAB, _CGLS (the multi entries take the first two)
constexpr int kKrylovVectors[3] = {3, 5, 4};          // CG: r p q; BiCGSTAB: r rhat p v t; CGLS: r q s p
constexpr int kKrylovLaunches[3] = {3, 5, 4};         // vector kernels of an iteration
constexpr int kKrylovProducts[3] = {1, 2, 1};
constexpr int kKrylovProductsT[3] = {0, 0, 1};

// The two scalar blocks: every kernel of a solve reads the block the kernel before it wrote and writes the other.  Kernel j of
// `kernels` writes block (kernels - 1 - j) % 2, so the last one writes block 0, which the status entries read.
struct KrylovBlocks {
    int64_t kernels = 0, launched = 0;
    int64_t current() const { return (kernels - launched) % 2; }          // the block the last launched kernel wrote
    int64_t take() { return (kernels - launched++) % 2; }                 // the block the next kernel reads; it writes 1 - that
};

// What a backend is built on.  Owns the pinned buffer of the host's looks (check_every > 0), whichever way the solve ends.
struct KrylovSolve {
    hispmv_ctx* c = nullptr;
    int idx = 0, solver = 0;
    int64_t max_iters = 0, check_every = 0, products = 0;
    char* work = nullptr;
    void* stream_arg = nullptr;
    hipStream_t s = nullptr;
    const float *d_b = nullptr, *d_minv = nullptr;
    float* d_x = nullptr;
    double* pinned = nullptr;
    KrylovBlocks blocks;
    int64_t current() const { return blocks.current(); }
    KrylovSolve() = default;
    KrylovSolve(const KrylovSolve&) = delete;
    ~KrylovSolve() { host_free(pinned); }
};
// a backend's launcher of one vector kernel, reported under the launcher's own name
#define KRYLOV_LAUNCHER(name, launcher)          \
    int name(const decltype(base)& k) {          \
        LAUNCH_TRY(c, launcher, k, s);           \
        return HISPMV_OK;                        \
    }

inline void fill_result(const double* S, bool all_enqueued, int64_t products, hispmv_krylov_result* out) {
    out->status = S[kKsBreakdown] != 0.0 ? HISPMV_KRYLOV_BREAKDOWN : S[kKsDone] != 0.0 ? HISPMV_KRYLOV_CONVERGED : HISPMV_KRYLOV_MAX_ITERS;
    out->iterations = (int32_t)S[kKsIters];
    out->relres = S[kKsBb] > 0.0 ? std::sqrt(S[kKsRr] / S[kKsBb]) : 0.0;
    out->products = all_enqueued ? (int64_t)S[kKsProducts] : products;
}

// The checks of the entries, under the context's lock; w = the entry's name as its messages give it.
inline int krylov_check_scalars(hispmv_ctx* c, const std::string& w, double rtol, int64_t max_iters, int64_t check_every) {
    if (!(rtol >= 0.0)) return fail(c, HISPMV_EINVAL, w + ": rtol must not be negative");
    if (max_iters < 1 || max_iters > (1LL << 30)) return fail(c, HISPMV_EINVAL, w + ": max_iters must be at least 1 (and at most 2^30)");
    if (check_every < 0) return fail(c, HISPMV_EINVAL, w + ": check_every must not be negative");
    return HISPMV_OK;
}
inline int krylov_check_square(hispmv_ctx* c, const std::string& w, const Matrix& m) {
    if (m.rows == m.cols) return HISPMV_OK;
    return fail(c, HISPMV_EINVAL, w + ": the handle is " + std::to_string(m.rows) + " x " + std::to_string(m.cols) + ", the solver needs a square matrix (hispmv_cgls_device takes any)");
}
// missing: a vector the call needs is NULL; a, b, opt: its fp32 vectors (opt may be NULL)
inline int krylov_check_operands(hispmv_ctx* c, const std::string& w, bool missing, const void* a, const void* b, const void* opt = nullptr) {
    if (missing) return fail(c, HISPMV_EINVAL, "NULL device vector");
    if (((uintptr_t)a | (uintptr_t)b | (uintptr_t)opt) & 3) return fail(c, HISPMV_EINVAL, w + ": device pointers must be 4-byte aligned");
    return HISPMV_OK;
}
// the block-Jacobi buffer of hispmv_cg_bj_device and hispmv_gmres_bj_device in the place of d_minv
inline int krylov_check_blocks(hispmv_ctx* c, const std::string& w, const void* d_pre, int64_t bs) {
    if (bs != 4 && bs != 8 && bs != 16 && bs != 32) return fail(c, HISPMV_EINVAL, w + ": block_size must be 4, 8, 16 or 32");
    if (!d_pre || ((uintptr_t)d_pre & 15)) return fail(c, HISPMV_EINVAL, w + ": the block-Jacobi buffer must be the 16-byte aligned one of hispmv_block_jacobi_setup_device");
    return HISPMV_OK;
}
// asks = who wants `need` bytes: "hispmv_krylov_info asks for", "the 2 partials take"
inline int krylov_check_work(hispmv_ctx* c, const std::string& w, const void* d_work, int64_t work_bytes, int64_t need, const std::string& asks) {
    if (work_bytes < need || (need > 0 && !d_work))
        return fail(c, HISPMV_EINVAL, w + ": the workspace holds " + std::to_string(d_work ? work_bytes : 0) + " bytes, " + asks + " " + std::to_string(need));
    if ((uintptr_t)d_work & 15) return fail(c, HISPMV_EINVAL, w + ": the workspace must be 16-byte aligned");
    return HISPMV_OK;
}
// the checks of hispmv_dot_device and hispmv_dot_multi_device behind those of their sizes
inline int krylov_check_dot(hispmv_ctx* c, const std::string& w, int64_t n, const float* d_a, const float* d_b, const double* d_out) {
    if (const int rc = krylov_check_operands(c, w, !d_out || (n > 0 && (!d_a || !d_b)), d_a, d_b)) return rc;
    if ((uintptr_t)d_out & 7) return fail(c, HISPMV_EINVAL, w + ": d_out must be 8-byte aligned");
    return HISPMV_OK;
}

// the operands of the backend's next kernel: it reads the block the kernel before it wrote
template <class B>
auto krylov_step(B& v) {
    auto k = v.base;
    const int64_t in = v.blocks.take();
    k.s_in = v.state(in);
    k.s_out = v.state(1 - in);
    return k;
}

// The launches of a solve, in order.  Returns behind the last one (check_every == 0) or behind the look that ends it.  The backend's
// base step carries what every kernel of it shares (lengths, x, the partials, tol2); B::kCgls: the backend has product_t and the two
// CGLS kernels, and its base step the lengths n (of x) and n2 (of b).
template <class B>
int krylov_run(B& v) {
    const bool bicg = v.solver == HISPMV_KRYLOV_BICGSTAB;
    bool cgls = false;
    if constexpr (B::kCgls) cgls = v.solver == HISPMV_KRYLOV_CGLS;
    // (b, b); a caller that looks at all learns here that b is zero: x = 0, converged, no product
    if (const int rc = v.dot_bb()) return rc;
    if (v.check_every > 0) {
        bool zero = false;
        if (const int rc = v.zero_rhs(&zero)) return rc;
        if (zero) {
            v.report(hispmv_krylov_result{HISPMV_KRYLOV_CONVERGED, 0, 0.0, 0});
            return HISPMV_OK;
        }
    }
    float *r = v.vec(0), *p = v.vec(cgls ? 3 : bicg ? 2 : 1), *q = v.vec(cgls ? 1 : bicg ? 3 : 2);          // BiCGSTAB: q is v
    float *rhat = bicg ? v.vec(1) : nullptr, *t = bicg ? v.vec(4) : nullptr, *sv = cgls ? v.vec(2) : nullptr;
    v.base.minv = v.d_minv; v.base.r = r; v.base.p = p;
    // where rho's partials lie: with minv (CG only) (r, minv r) has an array of its own, otherwise rho is rr -- also BiCGSTAB's first,
    // (rhat, r) = (r, r); its later ones the kernels keep in kSlotRho themselves
    v.base.slot_rho = v.d_minv ? kSlotRho : kSlotRr;
    if constexpr (B::kCgls)
        if (cgls)          // the reference of the stopping rule: (A^T b, A^T b)
            if (const int rc = v.reference(sv)) return rc;
    if (const int rc = v.residual(r)) return rc;          // r = b - A x
    if constexpr (B::kCgls)
        if (cgls)
            if (const int rc = v.product_t(r, sv)) return rc;
    {
        auto k = krylov_step(v);
        k.rhat = rhat;
        if (cgls) k.r = sv;
        if (const int rc = v.init(k)) return rc;
    }
    bool stop = false, looked = false;
    for (int64_t it = 0; it < v.max_iters && !stop; ++it) {
        looked = false;
        if (const int rc = v.product(p, q)) return rc;          // q = A p (BiCGSTAB: v)
        auto k = krylov_step(v);
        k.first = it == 0; k.slot1 = kSlotDen; k.a1 = cgls ? q : bicg ? rhat : p; k.b1 = q;
        if constexpr (B::kCgls)
            if (cgls) std::swap(k.n, k.n2);          // (q, q) streams the length of b; first: rr and rho lie over that of x
        if (const int rc = v.step_dot(k)) return rc;
        if (bicg) {
            k = krylov_step(v);
            k.q = q;
            if (const int rc = v.bicg_s(k)) return rc;
            if (const int rc = v.product(r, t)) return rc;          // t = A s
            k = krylov_step(v);
            k.a1 = t; k.b1 = r; k.slot1 = kSlotTs; k.a2 = t; k.b2 = t; k.slot2 = kSlotTt;
            if (const int rc = v.step_dot(k)) return rc;
            k = krylov_step(v);
            k.t = t; k.rhat = rhat;
            if (const int rc = v.bicg_x(k)) return rc;
            k = krylov_step(v);
            k.q = q;
            if (const int rc = v.bicg_p(k)) return rc;
        } else if (!cgls) {
            k = krylov_step(v);
            k.q = q;
            if (const int rc = v.cg_update(k)) return rc;
            k = krylov_step(v);
            if (const int rc = v.direction(k)) return rc;
        } else if constexpr (B::kCgls) {
            k = krylov_step(v);
            k.q = q;
            if (const int rc = v.cgls_update(k)) return rc;
            if (const int rc = v.product_t(r, sv)) return rc;          // s = A^T r
            k = krylov_step(v);
            k.a1 = sv; k.b1 = sv; k.slot1 = kSlotRr;
            if (const int rc = v.step_dot(k)) return rc;
            k = krylov_step(v);
            k.r = sv;
            if (const int rc = v.direction(k)) return rc;
        }
        if (v.check_every > 0 && (it + 1) % v.check_every == 0) {
            if (const int rc = v.check(&stop)) return rc;
            looked = true;
        }
    }
    if (v.check_every == 0) {
        v.report(hispmv_krylov_result{HISPMV_KRYLOV_IN_FLIGHT, 0, 0.0, v.products});
        return HISPMV_OK;
    }
    if (!looked)
        if (const int rc = v.check(&stop)) return rc;
    v.report_looked();
    return HISPMV_OK;
}

}  // namespace hispmv
