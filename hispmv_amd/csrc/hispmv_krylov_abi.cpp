// hispmv_krylov_abi.cpp -- the Krylov entries of the C ABI (include/hispmv.h: hispmv_prep_krylov_groups, hispmv_krylov_info,
// hispmv_dot_device, hispmv_cg_device, hispmv_bicgstab_device, hispmv_cgls_device, hispmv_krylov_status) over the launchers of
// hispmv_krylov.h.  A translation unit of its own: the solver loops issue their products through hispmv_spmv_device and
// hispmv_spmv_device_t like any caller (so the context's lock is held for the argument checks only), run everything between two
// products in the vector kernels, and keep their whole state in the caller's workspace.
#include <cmath>

#include "hispmv_ctx.h"
#include "hispmv_krylov.h"

using namespace hispmv;

namespace {

// The workspace: two scalar blocks (a kernel reads one and writes the other), one double for hispmv_dot_device-style results, the
// partial arrays, then the solver's vectors, each of `stride` floats (a multiple of 4: every one 16-byte aligned).
constexpr int64_t kStateBytes = kKrylovState * 8;
constexpr int64_t kScratchOff = 2 * kStateBytes;
constexpr int64_t kPartsOff = 512;
constexpr int64_t kVecsOff = kPartsOff + (int64_t)kKrylovSlots * kKrylovMaxGroups * 8;
const int kVectors[3] = {3, 5, 4};          // CG: r p q; BiCGSTAB: r rhat p v t; CGLS: r q s p
const int kLaunches[3] = {3, 5, 4};
const int kProducts[3] = {1, 2, 1};
const int kProductsT[3] = {0, 0, 1};
const char* const kNames[3] = {"cg_device", "bicgstab_device", "cgls_device"};

int64_t stride_of(const Matrix& m) { return ((int64_t)std::max(m.rows, m.cols) + 3) / 4 * 4; }
int64_t work_bytes_of(const Matrix& m, int solver) { return kVecsOff + kVectors[solver] * stride_of(m) * 4; }
bool accepts(const Matrix& m, int solver) {
    if (!m.loaded) return false;
    return solver == HISPMV_KRYLOV_CGLS ? (m.companion || transposable_handle(m)) : m.rows == m.cols;
}

struct Solve {
    hispmv_ctx* c = nullptr;
    int idx = 0, solver = 0;
    int64_t rows = 0, cols = 0, stride = 0;
    int64_t max_iters = 0, check_every = 0;
    char* work = nullptr;
    void* stream_arg = nullptr;
    hipStream_t s = nullptr;
    double* pinned = nullptr;
    int64_t products = 0, state_kernels = 0, launched = 0;
    KrylovStep base;

    float* vec(int i) const { return (float*)(work + kVecsOff) + i * stride; }
    double* state(int64_t which) const { return (double*)(work + which * kStateBytes); }
    double* parts() const { return (double*)(work + kPartsOff); }
    double* slot(int k) const { return parts() + (int64_t)k * kKrylovMaxGroups; }
    // the block the last launched kernel wrote: kernel j of state_kernels writes block (state_kernels - 1 - j) % 2, the last one block 0
    int64_t current() const { return (state_kernels - launched) % 2; }
    // the next kernel's operands: it reads the block the one before it wrote
    KrylovStep step() {
        KrylovStep k = base;
        k.s_out = state((state_kernels - 1 - launched) % 2);
        k.s_in = state((state_kernels - launched) % 2);
        ++launched;
        return k;
    }
    int product(const float* x, const float* bias, float* y, float alpha, float beta) {
        ++products;
        return hispmv_spmv_device(c, idx, x, bias, y, alpha, beta, stream_arg);
    }
    int product_t(const float* x, float* y) {
        ++products;
        return hispmv_spmv_device_t(c, idx, x, nullptr, y, 1.0f, 0.0f, stream_arg);
    }
};

void fill_result(const double* S, bool all_enqueued, int64_t products, hispmv_krylov_result* out) {
    out->status = S[kKsBreakdown] != 0.0 ? HISPMV_KRYLOV_BREAKDOWN : S[kKsDone] != 0.0 ? HISPMV_KRYLOV_CONVERGED : HISPMV_KRYLOV_MAX_ITERS;
    out->iterations = (int32_t)S[kKsIters];
    out->relres = S[kKsBb] > 0.0 ? std::sqrt(S[kKsRr] / S[kKsBb]) : 0.0;
    out->products = all_enqueued ? (int64_t)S[kKsProducts] : products;
}

// One host look at the scalar block: copy, wait, read.  *stop = the solve has ended on the device.
int check(Solve& v, bool* stop) {
    HIP_TRY(v.c, hipMemcpyAsync(v.pinned, v.state(v.current()), kStateBytes, hipMemcpyDeviceToHost, v.s));
    HIP_TRY(v.c, hipStreamSynchronize(v.s));
    *stop = v.pinned[kKsDone] != 0.0 || v.pinned[kKsBreakdown] != 0.0;
    return HISPMV_OK;
}

// The launches of a solve, in order.  Returns behind the last one (check_every == 0) or behind the check that ends it.
int run(Solve& v, const float* d_b, float* d_x, const float* d_minv, hispmv_krylov_result* result) {
    hipStream_t s = v.s;
    const int64_t n = v.cols, nr = v.rows;          // elements of x; of b
    const bool cgls = v.solver == HISPMV_KRYLOV_CGLS, bicg = v.solver == HISPMV_KRYLOV_BICGSTAB;
    // (b, b); a caller that looks at all learns here that b is zero: x = 0, converged, no product
    LAUNCH_TRY(v.c, launch_krylov_dot, d_b, d_b, nr, v.slot(kSlotB2), s);
    if (v.check_every > 0) {
        double* d_scratch = (double*)(v.work + kScratchOff);
        LAUNCH_TRY(v.c, launch_krylov_dot_finish, v.slot(kSlotB2), krylov_groups(nr), d_scratch, s);
        HIP_TRY(v.c, hipMemcpyAsync(v.pinned, d_scratch, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(v.c, hipStreamSynchronize(s));
        if (v.pinned[0] == 0.0) {
            HIP_TRY(v.c, hipMemsetAsync(d_x, 0, (size_t)n * 4, s));
            result->status = HISPMV_KRYLOV_CONVERGED; result->iterations = 0; result->relres = 0.0; result->products = 0;
            return HISPMV_OK;
        }
    }
    float *r = v.vec(0), *p = nullptr, *q = nullptr, *rhat = nullptr, *t = nullptr, *sv = nullptr;
    if (cgls) { q = v.vec(1); sv = v.vec(2); p = v.vec(3); }
    else if (bicg) { rhat = v.vec(1); p = v.vec(2); q = v.vec(3); t = v.vec(4); }
    else { p = v.vec(1); q = v.vec(2); }
    v.base.x = d_x; v.base.minv = d_minv; v.base.p = p;
    // where rho's partials lie: with minv (CG only) (r, minv r) has an array of its own, otherwise rho is rr -- also BiCGSTAB's first,
    // (rhat, r) = (r, r); its later ones the kernels keep in kSlotRho themselves
    v.base.slot_rho = d_minv ? kSlotRho : kSlotRr;
    if (cgls) {          // the reference of the stopping rule: (A^T b, A^T b)
        if (const int rc = v.product_t(d_b, sv)) return rc;
        LAUNCH_TRY(v.c, launch_krylov_dot, sv, sv, n, v.slot(kSlotBb), s);
    }
    if (const int rc = v.product(d_x, d_b, r, -1.0f, 1.0f)) return rc;          // r = b - A x
    if (cgls) {
        if (const int rc = v.product_t(r, sv)) return rc;
    }
    {
        KrylovStep k = v.step();
        k.n = n; k.n2 = nr; k.r = cgls ? sv : r; k.rhat = rhat; k.slot_bb = cgls ? kSlotBb : kSlotB2;
        LAUNCH_TRY(v.c, launch_krylov_init, k, s);
    }
    bool stop = false, looked = false;
    for (int64_t it = 0; it < v.max_iters && !stop; ++it) {
        looked = false;
        if (const int rc = v.product(p, nullptr, q, 1.0f, 0.0f)) return rc;          // q = A p (BiCGSTAB: v)
        {
            KrylovStep k = v.step();
            k.first = it == 0; k.slot1 = kSlotDen;
            if (cgls) { k.n = nr; k.n2 = n; k.a1 = q; k.b1 = q; }
            else { k.n = n; k.n2 = n; k.a1 = bicg ? rhat : p; k.b1 = q; }
            LAUNCH_TRY(v.c, launch_krylov_step_dot, k, s);
        }
        if (cgls) {
            KrylovStep k = v.step();
            k.n = n; k.n2 = nr; k.r = r; k.q = q;
            LAUNCH_TRY(v.c, launch_krylov_cgls_update, k, s);
            if (const int rc = v.product_t(r, sv)) return rc;
            k = v.step();
            k.n = n; k.a1 = sv; k.b1 = sv; k.slot1 = kSlotRr;
            LAUNCH_TRY(v.c, launch_krylov_step_dot, k, s);
            k = v.step();
            k.n = n; k.r = sv; k.minv = nullptr;
            LAUNCH_TRY(v.c, launch_krylov_direction, k, s);
        } else if (bicg) {
            KrylovStep k = v.step();
            k.n = n; k.r = r; k.q = q;
            LAUNCH_TRY(v.c, launch_krylov_bicg_s, k, s);
            if (const int rc = v.product(r, nullptr, t, 1.0f, 0.0f)) return rc;          // t = A s
            k = v.step();
            k.n = n; k.a1 = t; k.b1 = r; k.slot1 = kSlotTs; k.a2 = t; k.b2 = t; k.slot2 = kSlotTt;
            LAUNCH_TRY(v.c, launch_krylov_step_dot, k, s);
            k = v.step();
            k.n = n; k.r = r; k.t = t; k.rhat = rhat;
            LAUNCH_TRY(v.c, launch_krylov_bicg_x, k, s);
            k = v.step();
            k.n = n; k.r = r; k.q = q;
            LAUNCH_TRY(v.c, launch_krylov_bicg_p, k, s);
        } else {
            KrylovStep k = v.step();
            k.n = n; k.r = r; k.q = q;
            LAUNCH_TRY(v.c, launch_krylov_cg_update, k, s);
            k = v.step();
            k.n = n; k.r = r;
            LAUNCH_TRY(v.c, launch_krylov_direction, k, s);
        }
        if (v.check_every > 0 && (it + 1) % v.check_every == 0) {
            if (const int rc = check(v, &stop)) return rc;
            looked = true;
        }
    }
    if (v.check_every == 0) {
        result->status = HISPMV_KRYLOV_IN_FLIGHT; result->iterations = 0; result->relres = 0.0; result->products = v.products;
        return HISPMV_OK;
    }
    if (!looked)
        if (const int rc = check(v, &stop)) return rc;
    fill_result(v.pinned, false, v.products, result);
    return HISPMV_OK;
}

int solve(hispmv_ctx* c, int idx, int solver, const float* d_b, float* d_x, const float* d_minv, double rtol, int64_t max_iters, int64_t check_every,
          void* d_work, int64_t work_bytes, void* stream, hispmv_krylov_result* result) {
    if (!c || !result) return HISPMV_EINVAL;
    Solve v;
    const std::string w(kNames[solver]);
    {
        std::lock_guard<std::mutex> g(c->mu);
        if (!(rtol >= 0.0)) return fail(c, HISPMV_EINVAL, w + ": rtol must not be negative");
        if (max_iters < 1 || max_iters > (1LL << 30)) return fail(c, HISPMV_EINVAL, w + ": max_iters must be at least 1 (and at most 2^30)");
        if (check_every < 0) return fail(c, HISPMV_EINVAL, w + ": check_every must not be negative");
        Matrix* mp = nullptr;
        if (const int rc = find_handle(c, idx, kNames[solver], &mp)) return rc;
        const Matrix& m = *mp;
        if (solver != HISPMV_KRYLOV_CGLS && m.rows != m.cols)
            return fail(c, HISPMV_EINVAL, w + ": the handle is " + std::to_string(m.rows) + " x " + std::to_string(m.cols) + ", the solver needs a square matrix (hispmv_cgls_device takes any)");
        if (solver == HISPMV_KRYLOV_CGLS && !m.companion && !transposable_handle(m)) return refuse_tile_stream(c, m, kNames[solver], "transposed product");
        if (!d_b || !d_x) return fail(c, HISPMV_EINVAL, "NULL device vector");
        if (((uintptr_t)d_b | (uintptr_t)d_x | (uintptr_t)d_minv) & 3) return fail(c, HISPMV_EINVAL, w + ": device pointers must be 4-byte aligned");
        const int64_t need = work_bytes_of(m, solver);
        if (!d_work || work_bytes < need) return fail(c, HISPMV_EINVAL, w + ": the workspace holds " + std::to_string(d_work ? work_bytes : 0) + " bytes, hispmv_krylov_info asks for " + std::to_string(need));
        if ((uintptr_t)d_work & 15) return fail(c, HISPMV_EINVAL, w + ": the workspace must be 16-byte aligned");
        if (const int rc = adopt_stream(c, stream, &v.s)) return rc;
        v.rows = m.rows; v.cols = m.cols; v.stride = stride_of(m);
    }
    v.c = c; v.idx = idx; v.solver = solver; v.max_iters = max_iters; v.check_every = check_every; v.work = (char*)d_work; v.stream_arg = stream;
    v.state_kernels = 1 + max_iters * kLaunches[solver];
    v.base.parts = v.parts(); v.base.tol2 = rtol * rtol;
    v.base.products = (double)((solver == HISPMV_KRYLOV_CGLS ? 3 : 1) + max_iters * (kProducts[solver] + kProductsT[solver]));
    if (check_every > 0) HIP_TRY(c, hipHostMalloc((void**)&v.pinned, kStateBytes, hipHostMallocDefault));
    const int rc = run(v, d_b, d_x, d_minv, result);
    host_free(v.pinned);
    return rc;
}

}  // namespace

HISPMV_API int hispmv_prep_krylov_groups(int64_t n, int64_t* groups) {
    if (!groups || n < 0) return HISPMV_EINVAL;
    *groups = krylov_groups(n);
    return HISPMV_OK;
}

HISPMV_API int hispmv_krylov_info(const hispmv_ctx* c, int idx, int solver, int64_t out[8]) {
    if (!c || !out || idx < 0 || idx >= (int)c->mats.size() || solver < 0 || solver > 2) return HISPMV_EINVAL;
    for (int i = 0; i < 8; ++i) out[i] = 0;
    const Matrix& m = *c->mats[(size_t)idx];
    if (!accepts(m, solver)) return HISPMV_OK;
    out[0] = 1; out[1] = work_bytes_of(m, solver); out[2] = kLaunches[solver]; out[3] = kProducts[solver]; out[4] = kProductsT[solver];
    out[5] = kVecsOff; out[6] = m.cols; out[7] = m.rows;
    return HISPMV_OK;
}

HISPMV_API int hispmv_dot_device(hispmv_ctx* c, int64_t n, const float* d_a, const float* d_b, double* d_out, void* d_work, int64_t work_bytes, void* stream) {
    if (!c) return HISPMV_EINVAL;
    hipStream_t s;
    {
        std::lock_guard<std::mutex> g(c->mu);
        if (n < 0) return fail(c, HISPMV_EINVAL, "dot_device: n must not be negative");
        if (!d_out || (n > 0 && (!d_a || !d_b))) return fail(c, HISPMV_EINVAL, "NULL device vector");
        if (((uintptr_t)d_a | (uintptr_t)d_b) & 3) return fail(c, HISPMV_EINVAL, "dot_device: device pointers must be 4-byte aligned");
        if ((uintptr_t)d_out & 7) return fail(c, HISPMV_EINVAL, "dot_device: d_out must be 8-byte aligned");
        const int64_t need = krylov_groups(n) * 8;
        if (work_bytes < need || (need > 0 && !d_work))
            return fail(c, HISPMV_EINVAL, "dot_device: the workspace holds " + std::to_string(d_work ? work_bytes : 0) + " bytes, the " + std::to_string(krylov_groups(n)) + " partials take " + std::to_string(need));
        if ((uintptr_t)d_work & 15) return fail(c, HISPMV_EINVAL, "dot_device: the workspace must be 16-byte aligned");
        if (const int rc = adopt_stream(c, stream, &s)) return rc;
    }
    LAUNCH_TRY(c, launch_krylov_dot, d_a, d_b, n, (double*)d_work, s);
    LAUNCH_TRY(c, launch_krylov_dot_finish, (const double*)d_work, krylov_groups(n), d_out, s);
    return HISPMV_OK;
}

HISPMV_API int hispmv_cg_device(hispmv_ctx* c, int idx, const float* d_b, float* d_x, const float* d_minv, double rtol, int64_t max_iters, int64_t check_every,
                                void* d_work, int64_t work_bytes, void* stream, hispmv_krylov_result* result) {
    return solve(c, idx, HISPMV_KRYLOV_CG, d_b, d_x, d_minv, rtol, max_iters, check_every, d_work, work_bytes, stream, result);
}

HISPMV_API int hispmv_bicgstab_device(hispmv_ctx* c, int idx, const float* d_b, float* d_x, double rtol, int64_t max_iters, int64_t check_every,
                                      void* d_work, int64_t work_bytes, void* stream, hispmv_krylov_result* result) {
    return solve(c, idx, HISPMV_KRYLOV_BICGSTAB, d_b, d_x, nullptr, rtol, max_iters, check_every, d_work, work_bytes, stream, result);
}

HISPMV_API int hispmv_cgls_device(hispmv_ctx* c, int idx, const float* d_b, float* d_x, double rtol, int64_t max_iters, int64_t check_every,
                                  void* d_work, int64_t work_bytes, void* stream, hispmv_krylov_result* result) {
    return solve(c, idx, HISPMV_KRYLOV_CGLS, d_b, d_x, nullptr, rtol, max_iters, check_every, d_work, work_bytes, stream, result);
}

HISPMV_API int hispmv_krylov_status(hispmv_ctx* c, const void* d_work, void* stream, hispmv_krylov_result* result) {
    if (!c || !result) return HISPMV_EINVAL;
    hipStream_t s;
    {
        std::lock_guard<std::mutex> g(c->mu);
        if (!d_work || ((uintptr_t)d_work & 15)) return fail(c, HISPMV_EINVAL, "krylov_status: the workspace must be the 16-byte aligned one of the solve");
        if (const int rc = adopt_stream(c, stream, &s)) return rc;
    }
    double S[kKrylovState];
    HIP_TRY(c, hipStreamSynchronize(s));
    HIP_TRY(c, hipMemcpy(S, d_work, kStateBytes, hipMemcpyDeviceToHost));          // block 0: what the last kernel of the solve wrote
    fill_result(S, true, 0, result);
    return HISPMV_OK;
}
