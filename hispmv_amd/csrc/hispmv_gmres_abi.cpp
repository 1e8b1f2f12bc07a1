// hispmv_gmres_abi.cpp -- the restarted GMRES(m) entries of the C ABI (include/hispmv.h: hispmv_gmres_info, hispmv_dot_basis_device,
// hispmv_gmres_device; the host-only hispmv_prep_gmres lies in hispmv_prep_abi.cpp) over the launchers of hispmv_gmres.h.  A
// translation unit of its own like the two Krylov entry files: the products go through hispmv_spmv_device like any caller's, the
// checks and the two-block bookkeeping are hispmv_krylov_solve.h's, and the whole state of a solve lies in the caller's workspace in
// the layout of gmres_layout, whose first 256 bytes hispmv_krylov_status reads unchanged.
#include "hispmv_gmres.h"
#include "hispmv_krylov_solve.h"

using namespace hispmv;

namespace {

// The order of launches of a GMRES solve.  Cycles of m = min(restart, iterations left) inner steps: r = b - A x into basis slot 0, the
// partials of (r, r), the open kernel; per step the product into slot j + 1 and the four vector kernels; the close.  The close is
// enqueued behind every cycle the loop leaves, also behind the look that found the solve ended inside it.
struct Gmres : KrylovSolve {
    int64_t n = 0, restart = 0;
    int bs = 0;                       // 0: d_minv is NULL or an inverse diagonal; else the block size of the block-Jacobi buffer it is
    GmresLayout l;
    hispmv_krylov_result* result = nullptr;
    GmresStep base;

    template <class P> P* at(int64_t off) const { return (P*)(work + off); }
    double* state(int64_t which) const { return at<double>(which * kGmresStateBytes); }
    float* vec(int64_t i) const { return at<float>(l.off_v) + i * l.stride; }
    GmresStep step() {
        GmresStep k = base;
        const int64_t in = blocks.take();
        k.s_in = state(in);
        k.s_out = state(1 - in);
        return k;
    }
    int look(bool* stop) {
        HIP_TRY(c, hipMemcpyAsync(pinned, state(current()), kGmresStateBytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        *stop = pinned[kKsDone] != 0.0 || pinned[kKsBreakdown] != 0.0;
        return HISPMV_OK;
    }
    int run() {
        LAUNCH_TRY(c, launch_krylov_dot, d_b, d_b, n, at<double>(l.off_b2), s);
        if (check_every > 0) {          // a caller that looks at all learns here that b is zero: x = 0, converged, no product
            double* d_scratch = at<double>(kGmresScratchOff);
            LAUNCH_TRY(c, launch_krylov_dot_finish, at<double>(l.off_b2), l.groups, d_scratch, s);
            HIP_TRY(c, hipMemcpyAsync(pinned, d_scratch, 8, hipMemcpyDeviceToHost, s));
            HIP_TRY(c, hipStreamSynchronize(s));
            if (pinned[0] == 0.0) {
                HIP_TRY(c, hipMemsetAsync(d_x, 0, (size_t)n * 4, s));
                *result = hispmv_krylov_result{HISPMV_KRYLOV_CONVERGED, 0, 0.0, 0};
                return HISPMV_OK;
            }
        }
        bool stop = false;
        for (int64_t it = 0; it < max_iters && !stop;) {
            const int64_t m = std::min(restart, max_iters - it);
            ++products;
            if (const int rc = hispmv_spmv_device(c, idx, d_x, d_b, vec(0), -1.0f, 1.0f, stream_arg)) return rc;
            LAUNCH_TRY(c, launch_krylov_dot, vec(0), vec(0), n, at<double>(l.off_rr), s);
            GmresStep k = step();
            k.first = it == 0;
            LAUNCH_TRY(c, launch_gmres_open, k, s, bs);
            for (int64_t j = 0; j < m && !stop; ++j) {
                ++products;
                if (const int rc = hispmv_spmv_device(c, idx, d_minv ? base.z : vec(j), nullptr, vec(j + 1), 1.0f, 0.0f, stream_arg)) return rc;
                LAUNCH_TRY(c, launch_gmres_multi_dot, vec(0), l.stride, j + 1, vec(j + 1), n, at<double>(l.off_pa), l.gp, state(current()), s);
                k = step();
                k.j = (int)j; k.parts_in = at<double>(l.off_pa); k.parts_out = at<double>(l.off_pb);
                LAUNCH_TRY(c, launch_gmres_sub, k, s);
                k = step();
                k.j = (int)j; k.second = 1; k.parts_in = at<double>(l.off_pb);
                LAUNCH_TRY(c, launch_gmres_sub, k, s);
                k = step();
                k.j = (int)j;
                LAUNCH_TRY(c, launch_gmres_rotate, k, s, bs);
                ++it;
                if (check_every > 0 && it % check_every == 0)
                    if (const int rc = look(&stop)) return rc;
            }
            k = step();
            LAUNCH_TRY(c, launch_gmres_close, k, s, bs);
        }
        if (check_every == 0) {
            *result = hispmv_krylov_result{HISPMV_KRYLOV_IN_FLIGHT, 0, 0.0, products};
            return HISPMV_OK;
        }
        if (const int rc = look(&stop)) return rc;          // the final look, behind the last close: x is complete
        fill_result(pinned, false, products, result);
        return HISPMV_OK;
    }
};

}  // namespace

HISPMV_API int hispmv_gmres_info(const hispmv_ctx* c, int idx, int64_t restart, int with_minv, int64_t out[8]) {
    if (!c || !out || idx < 0 || idx >= (int)c->mats.size() || restart < 1 || restart > kGmresMaxRestart) return HISPMV_EINVAL;
    for (int i = 0; i < 8; ++i) out[i] = 0;
    const Matrix& m = *c->mats[(size_t)idx];
    if (!m.loaded || m.rows != m.cols) return HISPMV_OK;
    const GmresLayout l = gmres_layout(m.rows, restart, with_minv != 0);
    out[0] = 1; out[1] = l.work_bytes; out[2] = kGmresLaunchesInner; out[3] = kGmresLaunchesCycle; out[4] = 1;
    out[5] = l.off_v; out[6] = l.stride; out[7] = m.rows;
    return HISPMV_OK;
}

HISPMV_API int hispmv_dot_basis_device(hispmv_ctx* c, int64_t n, int64_t k, const float* d_V, int64_t ld_v, const float* d_w, double* d_out, void* d_work,
                                       int64_t work_bytes, void* stream) {
    if (!c) return HISPMV_EINVAL;
    hipStream_t s;
    const std::string w("dot_basis_device");
    const int64_t groups = krylov_groups(n);
    {
        std::lock_guard<std::mutex> g(c->mu);
        if (n < 0) return fail(c, HISPMV_EINVAL, w + ": n must not be negative");
        if (k < 1 || k > kGmresMaxBasis) return fail(c, HISPMV_EINVAL, w + ": k must be 1 .. " + std::to_string(kGmresMaxBasis));
        if (k > 1 && ld_v < n) return fail(c, HISPMV_EINVAL, w + ": ld_v must be at least n");
        if (const int rc = krylov_check_dot(c, w, n, d_V, d_w, d_out)) return rc;
        if (const int rc = krylov_check_work(c, w, d_work, work_bytes, 8 * k * groups, "the " + std::to_string(k * groups) + " partials take")) return rc;
        if (const int rc = adopt_stream(c, stream, &s)) return rc;
    }
    LAUNCH_TRY(c, launch_gmres_multi_dot, d_V, ld_v, k, d_w, n, (double*)d_work, groups, nullptr, s);
    LAUNCH_TRY(c, launch_gmres_dot_finish, (const double*)d_work, groups, groups, k, d_out, s);
    return HISPMV_OK;
}

namespace {
// bs > 0 (hispmv_gmres_bj_device): d_minv is the block-Jacobi buffer of that block size, 16-byte aligned, and may not be NULL
int gmres_solve(hispmv_ctx* c, int idx, const float* d_b, float* d_x, const float* d_minv, int64_t bs, int64_t restart, double rtol, int64_t max_iters,
                int64_t check_every, void* d_work, int64_t work_bytes, void* stream, hispmv_krylov_result* result) {
    if (!c || !result) return HISPMV_EINVAL;
    Gmres v;
    const char* const name = bs != 0 ? "gmres_bj_device" : "gmres_device";
    const std::string w(name);
    {
        std::lock_guard<std::mutex> g(c->mu);
        if (const int rc = krylov_check_scalars(c, w, rtol, max_iters, check_every)) return rc;
        if (restart < 1 || restart > kGmresMaxRestart) return fail(c, HISPMV_EINVAL, w + ": restart must be 1 .. " + std::to_string(kGmresMaxRestart));
        Matrix* mp = nullptr;
        if (const int rc = find_handle(c, idx, name, &mp)) return rc;
        const Matrix& m = *mp;
        if (const int rc = krylov_check_square(c, w, m)) return rc;
        if (bs != 0)
            if (const int rc = krylov_check_blocks(c, w, d_minv, bs)) return rc;
        if (const int rc = krylov_check_operands(c, w, !d_b || !d_x, d_b, d_x, d_minv)) return rc;
        v.n = m.rows;
        v.l = gmres_layout(v.n, restart, d_minv != nullptr);
        if (const int rc = krylov_check_work(c, w, d_work, work_bytes, v.l.work_bytes, "hispmv_gmres_info asks for")) return rc;
        if (const int rc = adopt_stream(c, stream, &v.s)) return rc;
    }
    v.c = c; v.idx = idx; v.max_iters = max_iters; v.check_every = check_every; v.work = (char*)d_work; v.stream_arg = stream;
    v.d_b = d_b; v.d_x = d_x; v.d_minv = d_minv; v.result = result; v.restart = restart; v.bs = (int)bs;
    const int64_t cycles = (max_iters + restart - 1) / restart;
    v.blocks.kernels = 2 * cycles + 3 * max_iters;          // open and close per cycle; subtract twice and rotate per step
    GmresStep& b = v.base;
    const GmresLayout& l = v.l;
    b.n = v.n; b.tol2 = rtol * rtol; b.products = (double)(cycles + max_iters); b.gp = l.gp; b.V = v.vec(0); b.stride = l.stride;
    b.x = d_x; b.minv = d_minv; b.z = d_minv ? v.at<float>(l.off_z) : nullptr;
    b.part_b2 = v.at<double>(l.off_b2); b.part_rr = v.at<double>(l.off_rr); b.part_ww = v.at<double>(l.off_ww);
    b.c = v.at<double>(l.off_c); b.s = v.at<double>(l.off_s); b.g_fin = v.at<double>(l.off_gfin); b.g_res = v.at<double>(l.off_gres);
    b.h1 = v.at<double>(l.off_h1); b.h = v.at<double>(l.off_h); b.R = v.at<double>(l.off_r);
    if (check_every > 0) HIP_TRY(c, hipHostMalloc((void**)&v.pinned, kGmresStateBytes, hipHostMallocDefault));
    return v.run();
}
}  // namespace

HISPMV_API int hispmv_gmres_device(hispmv_ctx* c, int idx, const float* d_b, float* d_x, const float* d_minv, int64_t restart, double rtol, int64_t max_iters,
                                   int64_t check_every, void* d_work, int64_t work_bytes, void* stream, hispmv_krylov_result* result) {
    return gmres_solve(c, idx, d_b, d_x, d_minv, 0, restart, rtol, max_iters, check_every, d_work, work_bytes, stream, result);
}

HISPMV_API int hispmv_gmres_bj_device(hispmv_ctx* c, int idx, const float* d_b, float* d_x, const void* d_pre, int64_t block_size, int64_t restart, double rtol,
                                      int64_t max_iters, int64_t check_every, void* d_work, int64_t work_bytes, void* stream, hispmv_krylov_result* result) {
    if (block_size == 0) return c ? fail(c, HISPMV_EINVAL, "gmres_bj_device: block_size must be 4, 8, 16 or 32") : HISPMV_EINVAL;
    return gmres_solve(c, idx, d_b, d_x, (const float*)d_pre, block_size, restart, rtol, max_iters, check_every, d_work, work_bytes, stream, result);
}
