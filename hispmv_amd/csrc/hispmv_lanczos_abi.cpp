// hispmv_lanczos_abi.cpp -- the thick-restart Lanczos entries of the C ABI (include/hispmv.h: hispmv_prep_lanczos, hispmv_prep_ritz,
// hispmv_lanczos_info, hispmv_basis_rotate_device, hispmv_lanczos_steps_device, hispmv_lanczos_status, hispmv_eigsh_device) as a
// backend of hispmv_thick_restart.h: a step's launches on one basis, the checks and the driver loop are its, shared with Golub-Kahan.
// The products go through hispmv_spmv_device like any caller's, and the whole state of a run lies in the caller's workspace in the
// layout of lanczos_layout.  The host half -- the Ritz values of the projected matrix, their order, the stopping rule -- is hispmv_prep_ritz,
// which needs no device.
#include <algorithm>
#include <numeric>
#include <vector>

#include "hispmv_thick_restart.h"

using namespace hispmv;

namespace {

constexpr int kM = kLanczosMaxNcv;

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

// The order of launches of a run.  A step: the product into slot j + 1, the orthogonalisation against slots 0 .. j (the multi-dot pass,
// the subtract-and-dot kernel twice), the record kernel.  The backend of thick_restart_run: the projected matrix is H, the look Hc
// with the betas behind it.
struct Lanczos : ThickRestart {
    static constexpr int64_t kLookDoubles = (int64_t)(kM + 1) * kLanczosHcLd;
    static constexpr int kRotations = 1, kLd = kM;
    int64_t n = 0;
    int which = 0;
    float* d_vecs = nullptr;
    int64_t ld_vecs = 0;
    std::vector<double> P, Yt, vals, res;          // of the driver only: H (kM x kM), the Ritz step's results

    float* vec(int64_t i) const { return at<float>(l.off_v) + i * l.stride; }
    int open(const float* d_v0) { return ThickRestart::open(d_v0, n, vec(0), l.stride); }
    int steps(int64_t j0, int64_t j1) {
        for (int64_t j = j0; j < j1; ++j) {
            if (const int rc = hispmv_spmv_device(c, idx, vec(j), nullptr, vec(j + 1), 1.0f, 0.0f, stream_arg)) return rc;
            if (const int rc = orthogonalise(n, vec(0), l.stride, j)) return rc;
            if (const int rc = record(n, vec(0), l.stride, j, kRecordLanczos, nullptr, true)) return rc;
        }
        return HISPMV_OK;
    }
    bool verdict(const double* S, int n_cv, int* m, bool* invariant, hispmv_eigsh_result*) const {
        *m = (int)S[kLsSteps];
        *invariant = S[kLsInvariant] != 0.0;
        return S[kKsBreakdown] == 0.0 && *m >= 1 && *m <= n_cv;
    }
    void project(const double* Hc, int j0, int m) {
        for (int j = j0; j < m; ++j)
            for (int i = 0; i <= j; ++i) P[(size_t)i * kM + j] = P[(size_t)j * kM + i] = Hc[(int64_t)j * kLanczosHcLd + i];
    }
    double decompose(const double* Hc, int m, int k, double tol, int64_t counts[2]) {
        const double* betas = Hc + (int64_t)kM * kLanczosHcLd;
        return ritz(P.data(), kM, m, k, which, betas[m - 1], tol, vals.data(), Yt.data(), res.data(), counts);
    }
    int finish(float* y32, int m, int found) { return rotate(y32, Yt.data(), n, vec(0), l.stride, m, found, d_vecs, ld_vecs, nullptr, nullptr); }
    int restart(float* y32, int m, int keep) { return rotate(y32, Yt.data(), n, vec(0), l.stride, m, keep, vec(0), l.stride, vec(m), vec(keep)); }
};

// the checks of the two entries that take a handle and a workspace; fills v
int lanczos_enter(hispmv_ctx* c, const char* name, int idx, int64_t basis_ncv, const void* d_work, int64_t work_bytes, void* stream, Lanczos& v) {
    return thick_restart_enter(c, name, idx, d_work, work_bytes, "hispmv_lanczos_info asks for", stream, v, [&](const Matrix& m) {
        if (const int rc = krylov_check_square(c, name, m)) return rc;
        v.n = m.rows;
        v.l = lanczos_layout(v.n, basis_ncv);
        return HISPMV_OK;
    });
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
    double S[kKrylovState];
    if (const int rc = thick_restart_status(c, "lanczos_status", d_work, stream, S)) return rc;
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
    v.which = which; v.d_vecs = d_vecs; v.ld_vecs = ld_vecs;
    v.P.assign((size_t)kM * kM, 0.0); v.Yt.resize((size_t)kM * kM); v.vals.resize(kM); v.res.resize(kM);
    return thick_restart_run(v, k, ncv, tol, max_products, d_v0, vals_out, res_out, result);
}
