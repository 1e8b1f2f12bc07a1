// hispmv_krylov_multi_abi.cpp -- the multi-right-hand-side Krylov entries of the C ABI (include/hispmv.h: hispmv_prep_krylov_multi,
// hispmv_krylov_multi_info, hispmv_dot_multi_device, hispmv_cg_multi_device, hispmv_bicgstab_multi_device, hispmv_krylov_multi_status)
// over the launchers of hispmv_krylov_multi.h.  The loop is krylov_run (hispmv_krylov_solve.h), the one of hispmv_krylov_abi.cpp, with
// one launch for all columns: it issues its products through hispmv_spmm_device like any caller (so the context's lock is held for the
// argument checks only) and keeps its whole state, the product's workspace included, in the caller's workspace.
#include <vector>

#include "hispmv_krylov_multi.h"
#include "hispmv_krylov_solve.h"

using namespace hispmv;

namespace {

constexpr int64_t kBlockBytes = kKrylovState * 8;          // one column's scalar block
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
    w.spmm_off = w.vecs_off + kKrylovVectors[solver] * w.vec_bytes;
    w.spmm_bytes = round16(spmm_bytes);
    w.total = w.spmm_off + w.spmm_bytes;
    return w;
}

// The multi-right-hand-side backend of krylov_run: products through hispmv_spmm_device, a scalar block and a result per column.
struct Solve : KrylovSolve {
    static constexpr bool kCgls = false;
    int64_t m = 0, ld_b = 0, ld_x = 0;
    Work w;
    hispmv_krylov_result* results = nullptr;
    KrylovMultiStep base;

    float* vec(int i) const { return (float*)(work + w.vecs_off + i * w.vec_bytes); }
    double* state(int64_t which) const { return (double*)(work + which * w.l.ldw * kBlockBytes); }
    double* scratch() const { return (double*)(work + 2 * w.l.ldw * kBlockBytes); }
    double* parts() const { return (double*)(work + w.l.state_bytes); }
    double* slot(int k) const { return parts() + (int64_t)k * w.l.groups * w.l.ldw; }
    // yt = alpha * A xt + beta * bias over all columns; yt and a bias are vectors of the workspace
    int product(const float* xt, int64_t ld_xt, const float* bias, float* yt, float alpha, float beta) {
        ++products;
        return hispmv_spmm_device(c, idx, xt, m, ld_xt, bias, bias ? w.l.ldw : 0, yt, w.l.ldw, alpha, beta, work + w.spmm_off, w.spmm_bytes, stream_arg);
    }
    int product(const float* xt, float* yt) { return product(xt, w.l.ldw, nullptr, yt, 1.0f, 0.0f); }
    // R = B, then R = R - A X in place
    int residual(float* r) {
        HIP_TRY(c, hipMemcpy2DAsync(r, (size_t)w.l.ldw * 4, d_b, (size_t)ld_b * 4, (size_t)m * 4, (size_t)w.n, hipMemcpyDeviceToDevice, s));
        return product(d_x, ld_x, r, r, -1.0f, 1.0f);
    }
    int dot_bb() { LAUNCH_TRY(c, launch_krylov_multi_dot, d_b, ld_b, d_b, ld_b, w.n, (int)m, w.l.ldw, slot(kSlotB2), s); return HISPMV_OK; }
    // one look at the (b_v, b_v); all zero: X = 0
    int zero_rhs(bool* zero) {
        LAUNCH_TRY(c, launch_krylov_multi_dot_finish, slot(kSlotB2), w.l.groups, (int)m, w.l.ldw, scratch(), s);
        HIP_TRY(c, hipMemcpyAsync(pinned, scratch(), (size_t)m * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        *zero = true;
        for (int64_t col = 0; col < m; ++col) *zero = *zero && pinned[col] == 0.0;
        if (*zero) HIP_TRY(c, hipMemset2DAsync(d_x, (size_t)ld_x * 4, 0, (size_t)m * 4, (size_t)w.n, s));
        return HISPMV_OK;
    }
    KRYLOV_LAUNCHER(init, launch_krylov_multi_init)
    KRYLOV_LAUNCHER(step_dot, launch_krylov_multi_step_dot)
    KRYLOV_LAUNCHER(cg_update, launch_krylov_multi_cg_update)
    KRYLOV_LAUNCHER(direction, launch_krylov_multi_direction)
    KRYLOV_LAUNCHER(bicg_s, launch_krylov_multi_bicg_s)
    KRYLOV_LAUNCHER(bicg_x, launch_krylov_multi_bicg_x)
    KRYLOV_LAUNCHER(bicg_p, launch_krylov_multi_bicg_p)
    // One host look at the columns' scalar blocks: one copy, one wait.  *stop = every column has ended on the device.
    int check(bool* stop) {
        HIP_TRY(c, hipMemcpyAsync(pinned, state(current()), (size_t)(m * kBlockBytes), hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        *stop = true;
        for (int64_t col = 0; col < m; ++col) {
            const double* S = pinned + col * kKrylovState;
            if (S[kKsDone] == 0.0 && S[kKsBreakdown] == 0.0) *stop = false;
        }
        return HISPMV_OK;
    }
    void report(const hispmv_krylov_result& r) {
        for (int64_t col = 0; col < m; ++col) results[col] = r;
    }
    void report_looked() {
        for (int64_t col = 0; col < m; ++col) fill_result(pinned + col * kKrylovState, false, products, results + col);
    }
};

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
        if (const int rc = krylov_check_scalars(c, w, rtol, max_iters, check_every)) return rc;
        Matrix* mp = nullptr;
        if (const int rc = find_handle(c, idx, kNames[solver], &mp)) return rc;
        const Matrix& m = *mp;
        if (const int rc = check_dims(c, w, std::max(m.rows, m.cols), num_vecs)) return rc;
        if (ld_b < num_vecs || ld_x < num_vecs) return fail(c, HISPMV_EINVAL, w + ": ld_b and ld_x must be at least num_vecs");
        int64_t spmm_bytes = 0;
        if (const int rc = spmm_bytes_of(c, idx, num_vecs, krylov_multi_layout(m.rows, num_vecs).ldw, &spmm_bytes)) return fail(c, rc, w + ": hispmv_spmm_info failed");
        refused = spmm_bytes < 0;
        if (!refused) {
            if (const int rc = krylov_check_square(c, w, m)) return rc;
            if (const int rc = krylov_check_operands(c, w, !d_b || !d_x, d_b, d_x, d_minv)) return rc;
            v.w = work_of(m.rows, num_vecs, solver, spmm_bytes);
            if (const int rc = krylov_check_work(c, w, d_work, work_bytes, v.w.total, "hispmv_krylov_multi_info asks for")) return rc;
            if (const int rc = adopt_stream(c, stream, &v.s)) return rc;
        }
    }
    // a tile-stream or dense handle: hispmv_spmm_device's own refusal, which comes before any of its argument checks and any launch
    if (refused) return hispmv_spmm_device(c, idx, nullptr, 1, 1, nullptr, 0, nullptr, 1, 0.0f, 0.0f, nullptr, 0, stream);
    v.c = c; v.idx = idx; v.solver = solver; v.m = num_vecs; v.ld_b = ld_b; v.ld_x = ld_x;
    v.max_iters = max_iters; v.check_every = check_every; v.work = (char*)d_work; v.stream_arg = stream;
    v.d_b = d_b; v.d_x = d_x; v.d_minv = d_minv; v.results = results;
    v.blocks.kernels = 1 + max_iters * kKrylovLaunches[solver];
    v.base.n = v.w.n; v.base.m = (int)num_vecs; v.base.ldw = v.w.l.ldw; v.base.groups = v.w.l.groups;
    v.base.x = d_x; v.base.ld_x = ld_x; v.base.parts = v.parts(); v.base.tol2 = rtol * rtol;
    v.base.products = (double)(1 + max_iters * kKrylovProducts[solver]);
    if (check_every > 0) HIP_TRY(c, hipHostMalloc((void**)&v.pinned, (size_t)(num_vecs * kBlockBytes), hipHostMallocDefault));
    return krylov_run(v);
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
    out[0] = 1; out[1] = w.total; out[2] = kKrylovLaunches[solver]; out[3] = kKrylovProducts[solver]; out[4] = w.l.ldw; out[5] = w.vecs_off; out[6] = m.rows; out[7] = w.l.groups;
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
        if (const int rc = krylov_check_dot(c, w, n, d_a, d_b, d_out)) return rc;
        l = krylov_multi_layout(n, num_vecs);
        if (const int rc = krylov_check_work(c, w, d_work, work_bytes, l.groups * l.ldw * 8, "the " + std::to_string(l.groups) + " x " + std::to_string(l.ldw) + " partials take")) return rc;
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
