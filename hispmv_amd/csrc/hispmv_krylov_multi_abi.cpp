// hispmv_krylov_multi_abi.cpp -- the multi-right-hand-side Krylov entries of the C ABI (include/hispmv.h: hispmv_prep_krylov_multi,
// hispmv_krylov_multi_info, hispmv_dot_multi_device, hispmv_cg_multi_device, hispmv_bicgstab_multi_device, hispmv_krylov_multi_status)
// over the launchers of hispmv_krylov_multi.h.  The loops are those of hispmv_krylov_abi.cpp with one launch for all columns: they
// issue their products through hispmv_spmm_device like any caller (so the context's lock is held for the argument checks only) and
// keep their whole state, the product's workspace included, in the caller's workspace.
#include <cmath>
#include <vector>

#include "hispmv_ctx.h"
#include "hispmv_krylov_multi.h"

using namespace hispmv;

namespace {

constexpr int64_t kBlockBytes = kKrylovState * 8;          // one column's scalar block
const int kVectors[2] = {3, 5};                            // CG: r p q; BiCGSTAB: r rhat p v t
const int kLaunches[2] = {3, 5};
const int kProducts[2] = {1, 2};
const char* const kNames[2] = {"cg_multi_device", "bicgstab_multi_device"};

int64_t round16(int64_t b) { return (b + 15) / 16 * 16; }

// the workspace of `solver` for num_vecs columns on a handle of n rows whose products take spmm_bytes
struct Work {
    KrylovMultiLayout l;
    int64_t n = 0, vec_bytes = 0, vecs_off = 0, spmm_off = 0, spmm_bytes = 0, total = 0;
};
Work work_of(int64_t n, int64_t num_vecs, int solver, int64_t spmm_bytes) {
    Work w;
    w.l = krylov_multi_layout(n, num_vecs);
    w.n = n;
    w.vec_bytes = n * w.l.ldw * 4;
    w.vecs_off = w.l.state_bytes + w.l.part_bytes;
    w.spmm_off = w.vecs_off + kVectors[solver] * w.vec_bytes;
    w.spmm_bytes = round16(spmm_bytes);
    w.total = w.spmm_off + w.spmm_bytes;
    return w;
}

struct Solve {
    hispmv_ctx* c = nullptr;
    int idx = 0, solver = 0;
    int64_t m = 0, ld_b = 0, ld_x = 0;
    int64_t max_iters = 0, check_every = 0;
    Work w;
    char* work = nullptr;
    void* stream_arg = nullptr;
    hipStream_t s = nullptr;
    double* pinned = nullptr;          // m scalar blocks
    int64_t products = 0, state_kernels = 0, launched = 0;
    KrylovMultiStep base;

    float* vec(int i) const { return (float*)(work + w.vecs_off + i * w.vec_bytes); }
    double* state(int64_t which) const { return (double*)(work + which * w.l.ldw * kBlockBytes); }
    double* scratch() const { return (double*)(work + 2 * w.l.ldw * kBlockBytes); }
    double* parts() const { return (double*)(work + w.l.state_bytes); }
    double* slot(int k) const { return parts() + (int64_t)k * w.l.groups * w.l.ldw; }
    // kernel j of state_kernels writes block (state_kernels - 1 - j) % 2, the last one block 0 (what hispmv_krylov_multi_status reads)
    int64_t current() const { return (state_kernels - launched) % 2; }
    KrylovMultiStep step() {
        KrylovMultiStep k = base;
        k.s_out = state((state_kernels - 1 - launched) % 2);
        k.s_in = state((state_kernels - launched) % 2);
        ++launched;
        return k;
    }
    // yt = alpha * A xt + beta * bias over all columns; yt and a bias are vectors of the workspace
    int product(const float* xt, int64_t ld_xt, const float* bias, float* yt, float alpha, float beta) {
        ++products;
        return hispmv_spmm_device(c, idx, xt, m, ld_xt, bias, bias ? w.l.ldw : 0, yt, w.l.ldw, alpha, beta, work + w.spmm_off, w.spmm_bytes, stream_arg);
    }
};

void fill_result(const double* S, bool all_enqueued, int64_t products, hispmv_krylov_result* out) {
    out->status = S[kKsBreakdown] != 0.0 ? HISPMV_KRYLOV_BREAKDOWN : S[kKsDone] != 0.0 ? HISPMV_KRYLOV_CONVERGED : HISPMV_KRYLOV_MAX_ITERS;
    out->iterations = (int32_t)S[kKsIters];
    out->relres = S[kKsBb] > 0.0 ? std::sqrt(S[kKsRr] / S[kKsBb]) : 0.0;
    out->products = all_enqueued ? (int64_t)S[kKsProducts] : products;
}

// One host look at the columns' scalar blocks: one copy, one wait.  *stop = every column has ended on the device.
int check(Solve& v, bool* stop) {
    HIP_TRY(v.c, hipMemcpyAsync(v.pinned, v.state(v.current()), (size_t)(v.m * kBlockBytes), hipMemcpyDeviceToHost, v.s));
    HIP_TRY(v.c, hipStreamSynchronize(v.s));
    *stop = true;
    for (int64_t col = 0; col < v.m; ++col) {
        const double* S = v.pinned + col * kKrylovState;
        if (S[kKsDone] == 0.0 && S[kKsBreakdown] == 0.0) *stop = false;
    }
    return HISPMV_OK;
}

int run(Solve& v, const float* d_b, float* d_x, const float* d_minv, hispmv_krylov_result* results) {
    hipStream_t s = v.s;
    const int64_t n = v.w.n, ldw = v.w.l.ldw, groups = v.w.l.groups;
    const int m = (int)v.m;
    const bool bicg = v.solver == HISPMV_KRYLOV_BICGSTAB;
    LAUNCH_TRY(v.c, launch_krylov_multi_dot, d_b, v.ld_b, d_b, v.ld_b, n, m, ldw, v.slot(kSlotB2), s);
    if (v.check_every > 0) {          // one look at the (b_v, b_v): all zero -> X = 0, converged, no product
        LAUNCH_TRY(v.c, launch_krylov_multi_dot_finish, v.slot(kSlotB2), groups, m, ldw, v.scratch(), s);
        HIP_TRY(v.c, hipMemcpyAsync(v.pinned, v.scratch(), (size_t)m * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(v.c, hipStreamSynchronize(s));
        bool all_zero = true;
        for (int col = 0; col < m; ++col) all_zero = all_zero && v.pinned[col] == 0.0;
        if (all_zero) {
            HIP_TRY(v.c, hipMemset2DAsync(d_x, (size_t)v.ld_x * 4, 0, (size_t)m * 4, (size_t)n, s));
            for (int col = 0; col < m; ++col) results[col] = hispmv_krylov_result{HISPMV_KRYLOV_CONVERGED, 0, 0.0, 0};
            return HISPMV_OK;
        }
    }
    float *r = v.vec(0), *p = nullptr, *q = nullptr, *rhat = nullptr, *t = nullptr;
    if (bicg) { rhat = v.vec(1); p = v.vec(2); q = v.vec(3); t = v.vec(4); }
    else { p = v.vec(1); q = v.vec(2); }
    v.base.x = d_x; v.base.ld_x = v.ld_x; v.base.minv = d_minv; v.base.p = p; v.base.r = r;
    v.base.slot_rho = d_minv ? kSlotRho : kSlotRr;
    // R = B, then R = R - A X in place
    HIP_TRY(v.c, hipMemcpy2DAsync(r, (size_t)ldw * 4, d_b, (size_t)v.ld_b * 4, (size_t)m * 4, (size_t)n, hipMemcpyDeviceToDevice, s));
    if (const int rc = v.product(d_x, v.ld_x, r, r, -1.0f, 1.0f)) return rc;
    {
        KrylovMultiStep k = v.step();
        k.rhat = rhat;
        LAUNCH_TRY(v.c, launch_krylov_multi_init, k, s);
    }
    bool stop = false, looked = false;
    for (int64_t it = 0; it < v.max_iters && !stop; ++it) {
        looked = false;
        if (const int rc = v.product(p, ldw, nullptr, q, 1.0f, 0.0f)) return rc;          // q = A p (BiCGSTAB: v)
        {
            KrylovMultiStep k = v.step();
            k.first = it == 0; k.slot1 = kSlotDen; k.a1 = bicg ? rhat : p; k.b1 = q;
            LAUNCH_TRY(v.c, launch_krylov_multi_step_dot, k, s);
        }
        if (bicg) {
            KrylovMultiStep k = v.step();
            k.q = q;
            LAUNCH_TRY(v.c, launch_krylov_multi_bicg_s, k, s);
            if (const int rc = v.product(r, ldw, nullptr, t, 1.0f, 0.0f)) return rc;      // t = A s
            k = v.step();
            k.a1 = t; k.b1 = r; k.slot1 = kSlotTs; k.a2 = t; k.b2 = t; k.slot2 = kSlotTt;
            LAUNCH_TRY(v.c, launch_krylov_multi_step_dot, k, s);
            k = v.step();
            k.t = t; k.rhat = rhat;
            LAUNCH_TRY(v.c, launch_krylov_multi_bicg_x, k, s);
            k = v.step();
            k.q = q;
            LAUNCH_TRY(v.c, launch_krylov_multi_bicg_p, k, s);
        } else {
            KrylovMultiStep k = v.step();
            k.q = q;
            LAUNCH_TRY(v.c, launch_krylov_multi_cg_update, k, s);
            k = v.step();
            LAUNCH_TRY(v.c, launch_krylov_multi_direction, k, s);
        }
        if (v.check_every > 0 && (it + 1) % v.check_every == 0) {
            if (const int rc = check(v, &stop)) return rc;
            looked = true;
        }
    }
    if (v.check_every == 0) {
        for (int col = 0; col < m; ++col) results[col] = hispmv_krylov_result{HISPMV_KRYLOV_IN_FLIGHT, 0, 0.0, v.products};
        return HISPMV_OK;
    }
    if (!looked)
        if (const int rc = check(v, &stop)) return rc;
    for (int col = 0; col < m; ++col) fill_result(v.pinned + (int64_t)col * kKrylovState, false, v.products, results + col);
    return HISPMV_OK;
}

// What hispmv_spmm_device makes of handle idx, asked through its own doors.  *bytes = its workspace for (num_vecs, ldw), -1 for a
// handle it refuses.
int spmm_bytes_of(const hispmv_ctx* c, int idx, int64_t num_vecs, int64_t ldw, int64_t* bytes) {
    int64_t out[8];
    if (hispmv_spmm_info(c, idx, num_vecs, ldw, out) != HISPMV_OK) return HISPMV_EINVAL;
    *bytes = out[0] ? out[5] : -1;
    return HISPMV_OK;
}

int check_dims(hispmv_ctx* c, const std::string& w, int64_t n, int64_t num_vecs) {
    if (num_vecs < 1) return fail(c, HISPMV_EINVAL, w + ": num_vecs must be at least 1");
    if (num_vecs > kKrylovMultiMaxVecs) return fail(c, HISPMV_EINVAL, w + ": num_vecs must not exceed 2^20");
    if (n > kKrylovMultiMaxN)
        return fail(c, HISPMV_EINVAL, w + ": n = " + std::to_string(n) + ", the multi-right-hand-side entries take n <= 1024 * 1024 (one chunk of 1024 rows per workgroup)");
    return HISPMV_OK;
}

int solve(hispmv_ctx* c, int idx, int solver, const float* d_b, int64_t ld_b, float* d_x, int64_t ld_x, int64_t num_vecs, const float* d_minv, double rtol,
          int64_t max_iters, int64_t check_every, void* d_work, int64_t work_bytes, void* stream, hispmv_krylov_result* results) {
    if (!c || !results) return HISPMV_EINVAL;
    Solve v;
    const std::string w(kNames[solver]);
    bool refused = false;
    {
        std::lock_guard<std::mutex> g(c->mu);
        if (!(rtol >= 0.0)) return fail(c, HISPMV_EINVAL, w + ": rtol must not be negative");
        if (max_iters < 1 || max_iters > (1LL << 30)) return fail(c, HISPMV_EINVAL, w + ": max_iters must be at least 1 (and at most 2^30)");
        if (check_every < 0) return fail(c, HISPMV_EINVAL, w + ": check_every must not be negative");
        Matrix* mp = nullptr;
        if (const int rc = find_handle(c, idx, kNames[solver], &mp)) return rc;
        const Matrix& m = *mp;
        if (const int rc = check_dims(c, w, std::max(m.rows, m.cols), num_vecs)) return rc;
        if (ld_b < num_vecs || ld_x < num_vecs) return fail(c, HISPMV_EINVAL, w + ": ld_b and ld_x must be at least num_vecs");
        int64_t spmm_bytes = 0;
        if (const int rc = spmm_bytes_of(c, idx, num_vecs, krylov_multi_layout(m.rows, num_vecs).ldw, &spmm_bytes)) return fail(c, rc, w + ": hispmv_spmm_info failed");
        refused = spmm_bytes < 0;
        if (!refused) {
            if (m.rows != m.cols)
                return fail(c, HISPMV_EINVAL, w + ": the handle is " + std::to_string(m.rows) + " x " + std::to_string(m.cols) + ", the solver needs a square matrix (hispmv_cgls_device takes any)");
            if (!d_b || !d_x) return fail(c, HISPMV_EINVAL, "NULL device vector");
            if (((uintptr_t)d_b | (uintptr_t)d_x | (uintptr_t)d_minv) & 3) return fail(c, HISPMV_EINVAL, w + ": device pointers must be 4-byte aligned");
            v.w = work_of(m.rows, num_vecs, solver, spmm_bytes);
            if (!d_work || work_bytes < v.w.total)
                return fail(c, HISPMV_EINVAL, w + ": the workspace holds " + std::to_string(d_work ? work_bytes : 0) + " bytes, hispmv_krylov_multi_info asks for " + std::to_string(v.w.total));
            if ((uintptr_t)d_work & 15) return fail(c, HISPMV_EINVAL, w + ": the workspace must be 16-byte aligned");
            if (const int rc = adopt_stream(c, stream, &v.s)) return rc;
        }
    }
    // a tile-stream or dense handle: hispmv_spmm_device's own refusal, which comes before any of its argument checks and any launch
    if (refused) return hispmv_spmm_device(c, idx, nullptr, 1, 1, nullptr, 0, nullptr, 1, 0.0f, 0.0f, nullptr, 0, stream);
    v.c = c; v.idx = idx; v.solver = solver; v.m = num_vecs; v.ld_b = ld_b; v.ld_x = ld_x;
    v.max_iters = max_iters; v.check_every = check_every; v.work = (char*)d_work; v.stream_arg = stream;
    v.state_kernels = 1 + max_iters * kLaunches[solver];
    v.base.n = v.w.n; v.base.m = (int)num_vecs; v.base.ldw = v.w.l.ldw; v.base.groups = v.w.l.groups;
    v.base.parts = v.parts(); v.base.tol2 = rtol * rtol;
    v.base.products = (double)(1 + max_iters * kProducts[solver]);
    if (check_every > 0) HIP_TRY(c, hipHostMalloc((void**)&v.pinned, (size_t)(num_vecs * kBlockBytes), hipHostMallocDefault));
    const int rc = run(v, d_b, d_x, d_minv, results);
    host_free(v.pinned);
    return rc;
}

}  // namespace

HISPMV_API int hispmv_prep_krylov_multi(int64_t n, int64_t num_vecs, int64_t out[4]) {
    if (!out || n < 0 || n > kKrylovMultiMaxN || num_vecs < 1 || num_vecs > kKrylovMultiMaxVecs) return HISPMV_EINVAL;
    const KrylovMultiLayout l = krylov_multi_layout(n, num_vecs);
    out[0] = l.groups; out[1] = l.ldw; out[2] = l.state_bytes; out[3] = l.part_bytes;
    return HISPMV_OK;
}

HISPMV_API int hispmv_krylov_multi_info(const hispmv_ctx* c, int idx, int solver, int64_t num_vecs, int64_t out[8]) {
    if (!c || !out || idx < 0 || idx >= (int)c->mats.size() || solver < 0 || solver > 1 || num_vecs < 1 || num_vecs > kKrylovMultiMaxVecs) return HISPMV_EINVAL;
    for (int i = 0; i < 8; ++i) out[i] = 0;
    const Matrix& m = *c->mats[(size_t)idx];
    if (!m.loaded || m.rows != m.cols || m.rows > kKrylovMultiMaxN) return HISPMV_OK;
    int64_t spmm_bytes = 0;
    if (spmm_bytes_of(c, idx, num_vecs, krylov_multi_layout(m.rows, num_vecs).ldw, &spmm_bytes) != HISPMV_OK || spmm_bytes < 0) return HISPMV_OK;
    const Work w = work_of(m.rows, num_vecs, solver, spmm_bytes);
    out[0] = 1; out[1] = w.total; out[2] = kLaunches[solver]; out[3] = kProducts[solver]; out[4] = w.l.ldw; out[5] = w.vecs_off; out[6] = m.rows; out[7] = w.l.groups;
    return HISPMV_OK;
}

HISPMV_API int hispmv_dot_multi_device(hispmv_ctx* c, int64_t n, int64_t num_vecs, const float* d_a, int64_t ld_a, const float* d_b, int64_t ld_b, double* d_out,
                                       void* d_work, int64_t work_bytes, void* stream) {
    if (!c) return HISPMV_EINVAL;
    hipStream_t s;
    const std::string w("dot_multi_device");
    KrylovMultiLayout l;
    {
        std::lock_guard<std::mutex> g(c->mu);
        if (n < 0) return fail(c, HISPMV_EINVAL, w + ": n must not be negative");
        if (const int rc = check_dims(c, w, n, num_vecs)) return rc;
        if (ld_a < num_vecs || ld_b < num_vecs) return fail(c, HISPMV_EINVAL, w + ": ld_a and ld_b must be at least num_vecs");
        if (!d_out || (n > 0 && (!d_a || !d_b))) return fail(c, HISPMV_EINVAL, "NULL device vector");
        if (((uintptr_t)d_a | (uintptr_t)d_b) & 3) return fail(c, HISPMV_EINVAL, w + ": device pointers must be 4-byte aligned");
        if ((uintptr_t)d_out & 7) return fail(c, HISPMV_EINVAL, w + ": d_out must be 8-byte aligned");
        l = krylov_multi_layout(n, num_vecs);
        const int64_t need = l.groups * l.ldw * 8;
        if (work_bytes < need || (need > 0 && !d_work))
            return fail(c, HISPMV_EINVAL, w + ": the workspace holds " + std::to_string(d_work ? work_bytes : 0) + " bytes, the " + std::to_string(l.groups) + " x " + std::to_string(l.ldw) + " partials take " + std::to_string(need));
        if ((uintptr_t)d_work & 15) return fail(c, HISPMV_EINVAL, w + ": the workspace must be 16-byte aligned");
        if (const int rc = adopt_stream(c, stream, &s)) return rc;
    }
    LAUNCH_TRY(c, launch_krylov_multi_dot, d_a, ld_a, d_b, ld_b, n, (int)num_vecs, l.ldw, (double*)d_work, s);
    LAUNCH_TRY(c, launch_krylov_multi_dot_finish, (const double*)d_work, l.groups, (int)num_vecs, l.ldw, d_out, s);
    return HISPMV_OK;
}

HISPMV_API int hispmv_cg_multi_device(hispmv_ctx* c, int idx, const float* d_b, int64_t ld_b, float* d_x, int64_t ld_x, int64_t num_vecs, const float* d_minv,
                                      double rtol, int64_t max_iters, int64_t check_every, void* d_work, int64_t work_bytes, void* stream,
                                      hispmv_krylov_result* results) {
    return solve(c, idx, HISPMV_KRYLOV_CG, d_b, ld_b, d_x, ld_x, num_vecs, d_minv, rtol, max_iters, check_every, d_work, work_bytes, stream, results);
}

HISPMV_API int hispmv_bicgstab_multi_device(hispmv_ctx* c, int idx, const float* d_b, int64_t ld_b, float* d_x, int64_t ld_x, int64_t num_vecs, double rtol,
                                            int64_t max_iters, int64_t check_every, void* d_work, int64_t work_bytes, void* stream, hispmv_krylov_result* results) {
    return solve(c, idx, HISPMV_KRYLOV_BICGSTAB, d_b, ld_b, d_x, ld_x, num_vecs, nullptr, rtol, max_iters, check_every, d_work, work_bytes, stream, results);
}

HISPMV_API int hispmv_krylov_multi_status(hispmv_ctx* c, const void* d_work, int64_t num_vecs, void* stream, hispmv_krylov_result* results) {
    if (!c || !results) return HISPMV_EINVAL;
    hipStream_t s;
    {
        std::lock_guard<std::mutex> g(c->mu);
        if (num_vecs < 1 || num_vecs > kKrylovMultiMaxVecs) return fail(c, HISPMV_EINVAL, "krylov_multi_status: num_vecs must be that of the solve");
        if (!d_work || ((uintptr_t)d_work & 15)) return fail(c, HISPMV_EINVAL, "krylov_multi_status: the workspace must be the 16-byte aligned one of the solve");
        if (const int rc = adopt_stream(c, stream, &s)) return rc;
    }
    std::vector<double> S((size_t)num_vecs * kKrylovState);
    HIP_TRY(c, hipStreamSynchronize(s));
    HIP_TRY(c, hipMemcpy(S.data(), d_work, S.size() * 8, hipMemcpyDeviceToHost));          // block 0: what the last kernel of the solve wrote
    for (int64_t col = 0; col < num_vecs; ++col) fill_result(S.data() + col * kKrylovState, true, 0, results + col);
    return HISPMV_OK;
}
