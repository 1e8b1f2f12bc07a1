// hispmv_lanczos_abi.cpp -- the thick-restart Lanczos entries of the C ABI (include/hispmv.h: hispmv_prep_lanczos, hispmv_prep_ritz,
// hispmv_lanczos_info, hispmv_basis_rotate_device, hispmv_lanczos_steps_device, hispmv_lanczos_status, hispmv_eigsh_device) over the
// launchers of hispmv_lanczos.h and the two GMRES launchers a step shares.  The products go through hispmv_spmv_device like any
// caller's, the checks are hispmv_krylov_solve.h's, and the whole state of a run lies in the caller's workspace in the layout of
// lanczos_layout.  The host half -- the Ritz values of the projected matrix, their order, the stopping rule -- is hispmv_prep_ritz,
// which needs no device.
#include <algorithm>
#include <numeric>
#include <vector>

#include "hispmv_krylov_solve.h"
#include "hispmv_lanczos.h"

using namespace hispmv;

namespace {

constexpr int kM = kLanczosMaxNcv;
constexpr int64_t kStateBytes = kKrylovState * 8;

// Cyclic Jacobi in Rutishauser's form on the symmetric a (m x m, row-major, destroyed): d = the eigenvalues, column c of v (row-major)
// the eigenvector of d[c].  Returns the sweeps it took.
int jacobi(double* a, int m, double* d, double* v) {
    double b[kM], z[kM];
    for (int i = 0; i < m; ++i) {
        for (int c = 0; c < m; ++c) v[i * m + c] = i == c ? 1.0 : 0.0;
        b[i] = d[i] = a[i * m + i];
        z[i] = 0.0;
    }
    auto rot = [&](double* x, int i1, int i2, double s, double tau) {
        const double g = x[i1], h = x[i2];
        x[i1] = g - s * (h + g * tau);
        x[i2] = h + s * (g - h * tau);
    };
    for (int sweep = 1; sweep <= 64; ++sweep) {
        double sm = 0.0;
        for (int p = 0; p < m - 1; ++p)
            for (int q = p + 1; q < m; ++q) sm += std::fabs(a[p * m + q]);
        if (sm == 0.0) return sweep - 1;
        const double tresh = sweep < 4 ? 0.2 * sm / ((double)m * m) : 0.0;
        for (int p = 0; p < m - 1; ++p)
            for (int q = p + 1; q < m; ++q) {
                const double apq = a[p * m + q], g = 100.0 * std::fabs(apq);
                if (sweep > 4 && std::fabs(d[p]) + g == std::fabs(d[p]) && std::fabs(d[q]) + g == std::fabs(d[q])) {
                    a[p * m + q] = 0.0;
                } else if (std::fabs(apq) > tresh) {
                    double h = d[q] - d[p], t;
                    if (std::fabs(h) + g == std::fabs(h)) {
                        t = apq / h;
                    } else {
                        const double theta = 0.5 * h / apq;
                        t = 1.0 / (std::fabs(theta) + std::sqrt(1.0 + theta * theta));
                        if (theta < 0.0) t = -t;
                    }
                    const double c = 1.0 / std::sqrt(1.0 + t * t), s = t * c, tau = s / (1.0 + c);
                    h = t * apq;
                    z[p] -= h; z[q] += h; d[p] -= h; d[q] += h;
                    a[p * m + q] = 0.0;
                    for (int j = 0; j < p; ++j) rot(a, j * m + p, j * m + q, s, tau);
                    for (int j = p + 1; j < q; ++j) rot(a, p * m + j, j * m + q, s, tau);
                    for (int j = q + 1; j < m; ++j) rot(a, p * m + j, q * m + j, s, tau);
                    for (int j = 0; j < m; ++j) rot(v, j * m + p, j * m + q, s, tau);
                }
            }
        for (int i = 0; i < m; ++i) {
            b[i] += z[i];
            d[i] = b[i];
            z[i] = 0.0;
        }
    }
    return 64;
}

// The Ritz step: theta, Yt (row c = the eigenvector of theta[c], m x m) and res in the order of `which`; counts = {converged among
// the first min(k, m), sweeps}.  Returns the scale max |theta|.
double ritz(const double* H, int64_t ld, int m, int k, int which, double beta, double tol, double* theta, double* Yt, double* res, int64_t counts[2]) {
    double a[kM * kM], v[kM * kM], d[kM];
    for (int i = 0; i < m; ++i)
        for (int c = 0; c < m; ++c) a[i * m + c] = c >= i ? H[i * ld + c] : H[c * ld + i];
    counts[1] = jacobi(a, m, d, v);
    int order[kM];
    std::iota(order, order + m, 0);
    std::stable_sort(order, order + m, [&](int x, int y) {
        if (which == HISPMV_EIGSH_SA) return d[x] < d[y];
        if (which == HISPMV_EIGSH_LM) return std::fabs(d[x]) > std::fabs(d[y]);
        return d[x] > d[y];
    });
    double scale = 0.0;
    for (int i = 0; i < m; ++i) scale = std::max(scale, std::fabs(d[i]));
    counts[0] = 0;
    for (int c = 0; c < m; ++c) {
        theta[c] = d[order[c]];
        for (int i = 0; i < m; ++i) Yt[c * m + i] = v[i * m + order[c]];
        res[c] = beta * std::fabs(Yt[c * m + m - 1]);
        if (c < std::min(k, m) && res[c] <= tol * scale) ++counts[0];
    }
    return scale;
}

// The order of launches of a run.  A step: the product into slot j + 1, the multi-dot pass over slots 0 .. j, the subtract-and-dot
// kernel twice, the normalise-and-record kernel.  The three kernels of a step that write the scalar block pass it round three blocks,
// 0 -> 1 -> 2 -> 0: every kernel reads one block and writes another, and every step -- so every call -- leaves the state in block 0,
// which the open kernel writes, the multi-dot kernel and the next step read, and hispmv_lanczos_status reports.
struct Lanczos : KrylovSolve {
    int64_t n = 0;
    LanczosLayout l;
    int cur = 0;

    template <class P> P* at(int64_t off) const { return (P*)(work + off); }
    double* state(int64_t which) const { return at<double>(which * kStateBytes); }
    float* vec(int64_t i) const { return at<float>(l.off_v) + i * l.stride; }
    template <class K> void turn(K& k) {
        k.s_in = state(cur);
        cur = (cur + 1) % 3;
        k.s_out = state(cur);
    }
    LanczosStep lstep() {
        LanczosStep k;
        k.n = n; k.V = vec(0); k.stride = l.stride; k.Hc = at<double>(l.off_hc); k.beta = at<double>(l.off_beta); k.h = at<double>(l.off_h);
        turn(k);
        return k;
    }
    GmresStep gstep(int64_t j, bool second) {
        GmresStep k;
        k.n = n; k.j = (int)j; k.second = second; k.gp = l.gp; k.V = vec(0); k.stride = l.stride;
        k.parts_in = at<double>(second ? l.off_pb : l.off_pa); k.parts_out = at<double>(l.off_pb); k.part_ww = at<double>(l.off_ww);
        k.h1 = at<double>(l.off_h1); k.h = at<double>(l.off_h);
        turn(k);
        return k;
    }
    int open(const float* d_v0) {
        LAUNCH_TRY(c, launch_krylov_dot, d_v0, d_v0, n, at<double>(l.off_vv), s);
        LanczosStep k = lstep();
        k.s_out = state(cur = 0);          // from nothing, into block 0
        k.v0 = d_v0; k.part = at<double>(l.off_vv);
        LAUNCH_TRY(c, launch_lanczos_open, k, s);
        return HISPMV_OK;
    }
    int steps(int64_t j0, int64_t j1) {
        for (int64_t j = j0; j < j1; ++j) {
            if (const int rc = hispmv_spmv_device(c, idx, vec(j), nullptr, vec(j + 1), 1.0f, 0.0f, stream_arg)) return rc;
            LAUNCH_TRY(c, launch_gmres_multi_dot, vec(0), l.stride, j + 1, vec(j + 1), n, at<double>(l.off_pa), l.gp, state(cur), s);
            LAUNCH_TRY(c, launch_gmres_sub, gstep(j, false), s);
            LAUNCH_TRY(c, launch_gmres_sub, gstep(j, true), s);
            LanczosStep k = lstep();
            k.j = (int)j; k.part = at<double>(l.off_ww);
            LAUNCH_TRY(c, launch_lanczos_norm, k, s);
        }
        return HISPMV_OK;
    }
};

// what the three entries that take a handle and a workspace check alike; fills v
int lanczos_enter(hispmv_ctx* c, const char* name, int idx, int64_t basis_ncv, const void* d_work, int64_t work_bytes, void* stream, Lanczos& v) {
    const std::string w(name);
    Matrix* mp = nullptr;
    if (const int rc = find_handle(c, idx, name, &mp)) return rc;
    if (const int rc = krylov_check_square(c, w, *mp)) return rc;
    v.n = mp->rows;
    v.l = lanczos_layout(v.n, basis_ncv);
    if (const int rc = krylov_check_work(c, w, d_work, work_bytes, v.l.work_bytes, "hispmv_lanczos_info asks for")) return rc;
    if (const int rc = adopt_stream(c, stream, &v.s)) return rc;
    v.c = c; v.idx = idx; v.work = (char*)d_work; v.stream_arg = stream;
    return HISPMV_OK;
}

}  // namespace

HISPMV_API int hispmv_prep_lanczos(int64_t n, int64_t ncv, int64_t out[8]) {
    if (!out || n < 0 || ncv < 2 || ncv > kLanczosMaxNcv) return HISPMV_EINVAL;
    const LanczosLayout l = lanczos_layout(n, ncv);
    out[0] = l.work_bytes; out[1] = l.off_v; out[2] = l.stride; out[3] = l.groups; out[4] = l.off_hc; out[5] = l.off_yt;
    out[6] = kLanczosLaunchesStep; out[7] = ncv + 1;
    return HISPMV_OK;
}

HISPMV_API int hispmv_prep_ritz(const double* H, int64_t ld, int64_t m, int64_t k, int which, double beta, double tol, double* theta_out, double* Yt_out,
                                double* res_out, int64_t counts_out[2]) {
    if (!H || !theta_out || !Yt_out || !res_out || !counts_out || m < 1 || m > kM || ld < m || k < 1 || !(tol >= 0.0)) return HISPMV_EINVAL;
    if (which != HISPMV_EIGSH_LA && which != HISPMV_EIGSH_SA && which != HISPMV_EIGSH_LM) return HISPMV_EINVAL;
    ritz(H, ld, (int)m, (int)std::min<int64_t>(k, kM), which, beta, tol, theta_out, Yt_out, res_out, counts_out);
    return HISPMV_OK;
}

HISPMV_API int hispmv_lanczos_info(const hispmv_ctx* c, int idx, int64_t ncv, int64_t out[8]) {
    if (!c || !out || idx < 0 || idx >= (int)c->mats.size() || ncv < 2 || ncv > kLanczosMaxNcv) return HISPMV_EINVAL;
    for (int i = 0; i < 8; ++i) out[i] = 0;
    const Matrix& m = *c->mats[(size_t)idx];
    if (!m.loaded || m.rows != m.cols) return HISPMV_OK;
    const LanczosLayout l = lanczos_layout(m.rows, ncv);
    out[0] = 1; out[1] = l.work_bytes; out[2] = l.off_v; out[3] = l.stride; out[4] = l.off_hc; out[5] = l.off_yt; out[6] = kLanczosLaunchesStep;
    out[7] = m.rows;
    return HISPMV_OK;
}

HISPMV_API int hispmv_basis_rotate_device(hispmv_ctx* c, int64_t n, int64_t m, int64_t k, const float* d_V, int64_t ld_v, const float* d_Yt, float* d_out,
                                          int64_t ld_out, void* stream) {
    if (!c) return HISPMV_EINVAL;
    hipStream_t s;
    const std::string w("basis_rotate_device");
    {
        std::lock_guard<std::mutex> g(c->mu);
        if (n < 0) return fail(c, HISPMV_EINVAL, w + ": n must not be negative");
        if (m < 1 || m > kRotateMaxIn) return fail(c, HISPMV_EINVAL, w + ": m must be 1 .. " + std::to_string(kRotateMaxIn));
        if (k < 1 || k > kRotateMaxOut) return fail(c, HISPMV_EINVAL, w + ": k must be 1 .. " + std::to_string(kRotateMaxOut));
        if ((m > 1 && ld_v < n) || (k > 1 && ld_out < n)) return fail(c, HISPMV_EINVAL, w + ": ld_v and ld_out must be at least n");
        if (const int rc = krylov_check_operands(c, w, !d_Yt || (n > 0 && (!d_V || !d_out)), d_V, d_out, d_Yt)) return rc;
        if (d_out == d_V && ld_out != ld_v) return fail(c, HISPMV_EINVAL, w + ": in place (d_out == d_V) ld_out must be ld_v");
        if (const int rc = adopt_stream(c, stream, &s)) return rc;
    }
    LAUNCH_TRY(c, launch_basis_rotate, d_V, ld_v, (int)m, (int)k, d_Yt, d_out, ld_out, n, nullptr, nullptr, s);
    return HISPMV_OK;
}

HISPMV_API int hispmv_lanczos_steps_device(hispmv_ctx* c, int idx, int64_t j0, int64_t j1, int first, const float* d_v0, void* d_work, int64_t work_bytes,
                                           void* stream) {
    if (!c) return HISPMV_EINVAL;
    Lanczos v;
    const std::string w("lanczos_steps_device");
    {
        std::lock_guard<std::mutex> g(c->mu);
        if (j0 < 0 || j1 <= j0 || j1 > kLanczosMaxNcv) return fail(c, HISPMV_EINVAL, w + ": steps j0 .. j1 - 1 need 0 <= j0 < j1 <= " + std::to_string(kLanczosMaxNcv));
        if (first && j0 != 0) return fail(c, HISPMV_EINVAL, w + ": a first call starts at step 0");
        if (const int rc = krylov_check_operands(c, w, first && !d_v0, d_v0, nullptr)) return rc;
        if (const int rc = lanczos_enter(c, "lanczos_steps_device", idx, std::max<int64_t>(j1, 2), d_work, work_bytes, stream, v)) return rc;
    }
    if (first)
        if (const int rc = v.open(d_v0)) return rc;
    return v.steps(j0, j1);
}

HISPMV_API int hispmv_lanczos_status(hispmv_ctx* c, const void* d_work, void* stream, int64_t out[4]) {
    if (!c || !out) return HISPMV_EINVAL;
    hipStream_t s;
    {
        std::lock_guard<std::mutex> g(c->mu);
        if (!d_work || ((uintptr_t)d_work & 15)) return fail(c, HISPMV_EINVAL, "lanczos_status: the workspace must be the 16-byte aligned one of the run");
        if (const int rc = adopt_stream(c, stream, &s)) return rc;
    }
    double S[kKrylovState];
    HIP_TRY(c, hipStreamSynchronize(s));
    HIP_TRY(c, hipMemcpy(S, d_work, kStateBytes, hipMemcpyDeviceToHost));          // block 0: where every call leaves the state
    out[0] = (int64_t)S[kLsSteps]; out[1] = S[kLsInvariant] != 0.0; out[2] = S[kKsBreakdown] != 0.0; out[3] = (int64_t)S[kKsProducts];
    return HISPMV_OK;
}

HISPMV_API int hispmv_eigsh_device(hispmv_ctx* c, int idx, int64_t k, int64_t ncv, int which, double tol, int64_t max_products, const float* d_v0,
                                   float* d_vecs, int64_t ld_vecs, double* vals_out, double* res_out, void* d_work, int64_t work_bytes, void* stream,
                                   hispmv_eigsh_result* result) {
    if (!c || !result) return HISPMV_EINVAL;
    Lanczos v;
    const std::string w("eigsh_device");
    {
        std::lock_guard<std::mutex> g(c->mu);
        if (k < 1) return fail(c, HISPMV_EINVAL, w + ": k must be at least 1");
        if (ncv < k + 1 || ncv > kLanczosMaxNcv) return fail(c, HISPMV_EINVAL, w + ": ncv must be k + 1 .. " + std::to_string(kLanczosMaxNcv));
        if (which != HISPMV_EIGSH_LA && which != HISPMV_EIGSH_SA && which != HISPMV_EIGSH_LM)
            return fail(c, HISPMV_EINVAL, w + ": which must be HISPMV_EIGSH_LA, _SA or _LM");
        if (!(tol >= 0.0)) return fail(c, HISPMV_EINVAL, w + ": tol must not be negative");
        if (max_products < 1 || max_products > (1LL << 30)) return fail(c, HISPMV_EINVAL, w + ": max_products must be at least 1 (and at most 2^30)");
        if (!vals_out || !res_out) return fail(c, HISPMV_EINVAL, w + ": vals_out and res_out must not be NULL");
        if (const int rc = krylov_check_operands(c, w, !d_v0 || !d_vecs, d_v0, d_vecs)) return rc;
        if (const int rc = lanczos_enter(c, "eigsh_device", idx, ncv, d_work, work_bytes, stream, v)) return rc;
        if (k > 1 && ld_vecs < v.n) return fail(c, HISPMV_EINVAL, w + ": ld_vecs must be at least n");
    }
    // pinned: the scalar block, Hc and the betas as the workspace holds them, then the fp32 coefficients of a rotation
    const int64_t hc_doubles = (int64_t)(kM + 1) * kLanczosHcLd;
    HIP_TRY(c, hipHostMalloc((void**)&v.pinned, (size_t)((kKrylovState + hc_doubles) * 8 + kRotateMaxOut * kRotateMaxIn * 4), hipHostMallocDefault));
    const double* S = v.pinned;
    const double *Hc = v.pinned + kKrylovState, *betas = Hc + (int64_t)kM * kLanczosHcLd;
    float* y32 = (float*)(v.pinned + kKrylovState + hc_doubles);
    std::vector<double> H((size_t)kM * kM, 0.0), Yt((size_t)kM * kM), theta(kM), res(kM);
    const int n_cv = (int)ncv, kk = (int)k;
    int64_t cycles = 0, counts[2] = {0, 0};
    *result = hispmv_eigsh_result{HISPMV_KRYLOV_BREAKDOWN, 0, 0, 0, 0.0};
    if (const int rc = v.open(d_v0)) return rc;
    // the coefficients of `cols` Ritz vectors over m basis vectors into the workspace, then the rotation into out
    auto rotate = [&](int m, int cols, float* out, int64_t ld_out, const float* xsrc, float* xdst) -> int {
        for (int col = 0; col < cols; ++col)
            for (int i = 0; i < m; ++i) y32[col * m + i] = (float)Yt[(size_t)col * m + i];
        HIP_TRY(c, hipMemcpyAsync(v.at<float>(v.l.off_yt), y32, (size_t)cols * m * 4, hipMemcpyHostToDevice, v.s));
        LAUNCH_TRY(c, launch_basis_rotate, v.vec(0), v.l.stride, m, cols, v.at<float>(v.l.off_yt), out, ld_out, v.n, xsrc, xdst, v.s);
        return HISPMV_OK;
    };
    for (int j0 = 0;;) {
        if (const int rc = v.steps(j0, n_cv)) return rc;
        ++cycles;
        HIP_TRY(c, hipMemcpyAsync(v.pinned, v.state(0), kStateBytes, hipMemcpyDeviceToHost, v.s));
        HIP_TRY(c, hipMemcpyAsync(v.pinned + kKrylovState, v.at<double>(v.l.off_hc), (size_t)hc_doubles * 8, hipMemcpyDeviceToHost, v.s));
        HIP_TRY(c, hipStreamSynchronize(v.s));
        result->products = (int64_t)S[kKsProducts];
        result->cycles = cycles;
        const int m = (int)S[kLsSteps];
        if (S[kKsBreakdown] != 0.0 || m < 1 || m > n_cv) return HISPMV_OK;          // BREAKDOWN: d_vecs untouched
        for (int j = j0; j < m; ++j)
            for (int i = 0; i <= j; ++i) H[(size_t)i * kM + j] = H[(size_t)j * kM + i] = Hc[(int64_t)j * kLanczosHcLd + i];
        result->scale = ritz(H.data(), kM, m, kk, which, betas[m - 1], tol, theta.data(), Yt.data(), res.data(), counts);
        const int found = std::min(kk, m);
        const bool invariant = S[kLsInvariant] != 0.0;
        int status = -1;
        if (counts[0] == found && m >= kk) status = HISPMV_KRYLOV_CONVERGED;
        else if (invariant) status = HISPMV_KRYLOV_INVARIANT;
        else if (result->products >= max_products) status = HISPMV_KRYLOV_MAX_ITERS;
        if (status >= 0) {
            for (int i = 0; i < found; ++i) { vals_out[i] = theta[i]; res_out[i] = res[i]; }
            if (const int rc = rotate(m, found, d_vecs, ld_vecs, nullptr, nullptr)) return rc;
            HIP_TRY(c, hipStreamSynchronize(v.s));
            result->status = status; result->found = found;
            return HISPMV_OK;
        }
        const int keep = std::min(kk + (n_cv - kk) / 2, n_cv - 1);
        if (const int rc = rotate(m, keep, v.vec(0), v.l.stride, v.vec(m), v.vec(keep))) return rc;
        std::fill(H.begin(), H.end(), 0.0);
        for (int i = 0; i < keep; ++i) H[(size_t)i * kM + i] = theta[i];
        j0 = keep;
    }
}
