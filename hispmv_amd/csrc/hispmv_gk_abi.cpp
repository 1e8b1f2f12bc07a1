// hispmv_gk_abi.cpp -- the thick-restart Golub-Kahan entries of the C ABI (include/hispmv.h: hispmv_prep_gk, hispmv_prep_bsvd,
// hispmv_gk_info, hispmv_gk_steps_device, hispmv_gk_status, hispmv_svds_device) as a backend of hispmv_thick_restart.h: a step's
// launches on one basis, the checks and the driver loop are its, shared with Lanczos.  The products go through hispmv_spmv_device and
// hispmv_spmv_device_t like any caller's, and the whole state of a run lies in the caller's workspace in the layout of gk_layout.  The host half -- the SVD of the projected matrix, its order, the stopping rule -- is hispmv_prep_bsvd, which needs no
// device.
#include <algorithm>
#include <numeric>
#include <vector>

#include "hispmv_thick_restart.h"

using namespace hispmv;

namespace {

constexpr int kM = kLanczosMaxNcv;
constexpr int kC = kM + 1;          // columns of the widest projected matrix

// One-sided (Hestenes) Jacobi on G = B^T (cb x rb, rb <= cb): plane rotations from the right make the columns of G orthogonal,
// G J = Q diag(s), so B = J diag(s) Q^T.  Pairs (p, q) in row-cyclic order; a pair rotates when |g_p . g_q| > 8 eps |g_p| |g_q|; at
// most 64 sweeps.  A column whose norm is zero has no direction: its place in Q is filled by the first unit vector e_0, e_1, ... that
// two Gram-Schmidt passes against the columns Q already holds leave longer than 1/2.  The order: descending, ties in Jacobi's order
// (a stable sort).  s[c], row c of Pt (rb long) and row c of Qt (cb long) belong together.  Returns the sweeps it took.
int hestenes(const double* B, int64_t ld, int rb, int cb, double* s, double* Pt, double* Qt) {
    std::vector<double> G((size_t)cb * rb), J((size_t)rb * rb, 0.0), nrm((size_t)rb), Q((size_t)cb * rb);
    for (int i = 0; i < rb; ++i) {
        J[(size_t)i * rb + i] = 1.0;
        for (int c = 0; c < cb; ++c) G[(size_t)c * rb + i] = B[i * ld + c];
    }
    constexpr double kEps8 = 8.0 * 2.220446049250313e-16;
    int sweeps = 0;
    for (int sweep = 1; sweep <= 64; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < rb - 1; ++p)
            for (int q = p + 1; q < rb; ++q) {
                double a = 0.0, b = 0.0, g = 0.0;
                for (int r = 0; r < cb; ++r) {
                    const double x = G[(size_t)r * rb + p], y = G[(size_t)r * rb + q];
                    a += x * x; b += y * y; g += x * y;
                }
                if (!(std::fabs(g) > kEps8 * std::sqrt(a * b))) continue;
                rotated = true;
                const double zeta = (b - a) / (2.0 * g);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
                const double cs = 1.0 / std::sqrt(1.0 + t * t), sn = cs * t;
                for (int r = 0; r < cb; ++r) {
                    const double x = G[(size_t)r * rb + p], y = G[(size_t)r * rb + q];
                    G[(size_t)r * rb + p] = cs * x - sn * y;
                    G[(size_t)r * rb + q] = sn * x + cs * y;
                }
                for (int r = 0; r < rb; ++r) {
                    const double x = J[(size_t)r * rb + p], y = J[(size_t)r * rb + q];
                    J[(size_t)r * rb + p] = cs * x - sn * y;
                    J[(size_t)r * rb + q] = sn * x + cs * y;
                }
            }
        if (!rotated) break;
        sweeps = sweep;
    }
    for (int i = 0; i < rb; ++i) {
        double a = 0.0;
        for (int r = 0; r < cb; ++r) a += G[(size_t)r * rb + i] * G[(size_t)r * rb + i];
        nrm[(size_t)i] = std::sqrt(a);
    }
    std::vector<int> order((size_t)rb);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return nrm[(size_t)x] > nrm[(size_t)y]; });
    int e_next = 0;
    for (int c = 0; c < rb; ++c) {
        const int i = order[(size_t)c];
        s[c] = nrm[(size_t)i];
        for (int r = 0; r < rb; ++r) Pt[(size_t)c * rb + r] = J[(size_t)r * rb + i];
        double* q = Qt + (size_t)c * cb;
        if (s[c] > 1e-290) {
            for (int r = 0; r < cb; ++r) q[r] = G[(size_t)r * rb + i] / s[c];
            continue;
        }
        s[c] = 0.0;
        for (; e_next < cb; ++e_next) {
            for (int r = 0; r < cb; ++r) q[r] = r == e_next ? 1.0 : 0.0;
            for (int pass = 0; pass < 2; ++pass)
                for (int d = 0; d < c; ++d) {
                    const double* o = Qt + (size_t)d * cb;
                    double dot = 0.0;
                    for (int r = 0; r < cb; ++r) dot += o[r] * q[r];
                    for (int r = 0; r < cb; ++r) q[r] -= dot * o[r];
                }
            double a = 0.0;
            for (int r = 0; r < cb; ++r) a += q[r] * q[r];
            if (a > 0.25) {
                a = std::sqrt(a);
                for (int r = 0; r < cb; ++r) q[r] /= a;
                ++e_next;
                break;
            }
        }
    }
    return sweeps;
}

// The look's small SVD with its residual estimates: res[c] = beta * |Pt[c][rb - 1]|; counts = {converged among the first min(k, rb),
// sweeps}.  Returns the scale s[0].
double bsvd(const double* B, int64_t ld, int rb, int cb, int k, double beta, double tol, double* s, double* Pt, double* Qt, double* res, int64_t counts[2]) {
    counts[1] = hestenes(B, ld, rb, cb, s, Pt, Qt);
    counts[0] = 0;
    for (int c = 0; c < rb; ++c) {
        res[c] = beta * std::fabs(Pt[(size_t)c * rb + rb - 1]);
        if (c < std::min(k, rb) && res[c] <= tol * s[0]) ++counts[0];
    }
    return s[0];
}

// The order of launches of a run.  A step: the forward product into U slot j, the orthogonalisation against U slots 0 .. j - 1, the U
// side's record kernel (j = 0: the dot kernel and the record kernel); the transposed product into V slot j + 1, the orthogonalisation
// against V slots 0 .. j, the V side's record kernel, the step's last.  The backend of thick_restart_run: the projected matrix is B,
// the look Gc with the alphas and the betas behind it.
struct Gk : ThickRestart {
    static constexpr int64_t kLookDoubles = (int64_t)(kM + 2) * kLanczosHcLd;
    static constexpr int kRotations = 2, kLd = kC;
    int64_t rows = 0, cols = 0;
    int vectors = 0;
    float *d_u = nullptr, *d_v = nullptr;
    int64_t ld_u = 0, ld_v = 0;
    bool closed = false;                                   // of the last look: the U side closed the space, B has m + 1 columns
    std::vector<double> P, Pt, Qt, vals, res;          // of the driver only: B (kM x kC), the small SVD's results

    float* vvec(int64_t i) const { return at<float>(l.off_v) + i * l.stride; }
    float* uvec(int64_t i) const { return at<float>(l.off_u) + i * l.stride_u; }
    int open(const float* d_v0) { return ThickRestart::open(d_v0, cols, vvec(0), l.stride); }
    int steps(int64_t j0, int64_t j1) {
        for (int64_t j = j0; j < j1; ++j) {
            if (const int rc = hispmv_spmv_device(c, idx, vvec(j), nullptr, uvec(j), 1.0f, 0.0f, stream_arg)) return rc;
            if (j == 0) {
                LAUNCH_TRY(c, launch_krylov_dot, uvec(0), uvec(0), rows, at<double>(l.off_ww), s);
            } else if (const int rc = orthogonalise(rows, uvec(0), l.stride_u, j - 1)) {
                return rc;
            }
            if (const int rc = record(rows, uvec(0), l.stride_u, j, kRecordGkU, at<double>(l.off_alpha), false)) return rc;
            if (const int rc = hispmv_spmv_device_t(c, idx, uvec(j), nullptr, vvec(j + 1), 1.0f, 0.0f, stream_arg)) return rc;
            if (const int rc = orthogonalise(cols, vvec(0), l.stride, j)) return rc;
            if (const int rc = record(cols, vvec(0), l.stride, j, kRecordGkV, nullptr, true)) return rc;
        }
        return HISPMV_OK;
    }
    bool verdict(const double* S, int n_cv, int* m, bool* invariant, hispmv_eigsh_result* result) {
        *m = (int)S[kLsSteps];
        *invariant = S[kLsInvariant] != 0.0;
        closed = S[kLsClosedU] != 0.0;
        if (S[kKsBreakdown] != 0.0 || *m < 0 || *m > n_cv || (*m == 0 && !closed)) return false;
        if (*m == 0) result->status = HISPMV_KRYLOV_INVARIANT;          // A v0 = 0: nothing found, and no breakdown
        return *m > 0;
    }
    void project(const double* Gc, int j0, int m) {
        const double* alphas = Gc + (int64_t)kM * kLanczosHcLd;
        for (int j = j0; j < (closed ? m + 1 : m); ++j) {
            for (int i = 0; i < j && i < m; ++i) P[(size_t)i * kC + j] = Gc[(int64_t)j * kLanczosHcLd + i];
            if (j < m) P[(size_t)j * kC + j] = alphas[j];
        }
    }
    double decompose(const double* Gc, int m, int k, double tol, int64_t counts[2]) {
        const double* betas = Gc + (int64_t)(kM + 1) * kLanczosHcLd;
        return bsvd(P.data(), kC, m, closed ? m + 1 : m, k, closed ? 0.0 : betas[m - 1], tol, vals.data(), Pt.data(), Qt.data(), res.data(), counts);
    }
    int finish(float* y32, int m, int found) {
        if (!vectors) return HISPMV_OK;
        if (const int rc = rotate(y32, Pt.data(), rows, uvec(0), l.stride_u, m, found, d_u, ld_u, nullptr, nullptr)) return rc;
        return rotate(y32 + kThickYtFloats, Qt.data(), cols, vvec(0), l.stride, closed ? m + 1 : m, found, d_v, ld_v, nullptr, nullptr);
    }
    int restart(float* y32, int m, int keep) {
        if (const int rc = rotate(y32, Pt.data(), rows, uvec(0), l.stride_u, m, keep, uvec(0), l.stride_u, nullptr, nullptr)) return rc;
        return rotate(y32 + kThickYtFloats, Qt.data(), cols, vvec(0), l.stride, m, keep, vvec(0), l.stride, vvec(m), vvec(keep));
    }
};

// the checks of the two entries that take a handle and a workspace; fills v
int gk_enter(hispmv_ctx* c, const char* name, int idx, int64_t k, int64_t basis_ncv, const void* d_work, int64_t work_bytes, void* stream, Gk& v) {
    return thick_restart_enter(c, name, idx, d_work, work_bytes, "hispmv_gk_info asks for", stream, v, [&](const Matrix& m) {
        if (!m.companion && !transposable_handle(m)) return refuse_tile_stream(c, m, "spmv_device_t", "transposed product");
        if (k > std::min(m.rows, m.cols))
            return fail(c, HISPMV_EINVAL, std::string(name) + ": the handle is " + std::to_string(m.rows) + " x " + std::to_string(m.cols) +
                                              ", k must be at most the smaller of the two");
        v.rows = m.rows; v.cols = m.cols;
        v.l = gk_layout(v.rows, v.cols, basis_ncv);
        return HISPMV_OK;
    });
}

}  // namespace

HISPMV_API int hispmv_prep_gk(int64_t rows, int64_t cols, int64_t ncv, int64_t out[8]) {
    if (!out || rows < 0 || cols < 0 || ncv < 2 || ncv > kM) return HISPMV_EINVAL;
    const LanczosLayout l = gk_layout(rows, cols, ncv);
    out[0] = l.work_bytes; out[1] = l.off_v; out[2] = l.stride; out[3] = l.off_u; out[4] = l.stride_u; out[5] = l.off_hc; out[6] = l.off_yt;
    out[7] = l.off_vv;
    return HISPMV_OK;
}

HISPMV_API int hispmv_prep_bsvd(const double* B, int64_t ld, int64_t rows_b, int64_t cols_b, int64_t k, double beta, double tol, double* s_out,
                                double* Pt_out, double* Qt_out, double* res_out, int64_t counts_out[2]) {
    if (!B || !s_out || !Pt_out || !Qt_out || !res_out || !counts_out) return HISPMV_EINVAL;
    if (rows_b < 1 || rows_b > kM || cols_b < rows_b || cols_b > rows_b + 1 || ld < cols_b || k < 1 || !(tol >= 0.0) || !(beta >= 0.0)) return HISPMV_EINVAL;
    bsvd(B, ld, (int)rows_b, (int)cols_b, (int)std::min<int64_t>(k, kM), beta, tol, s_out, Pt_out, Qt_out, res_out, counts_out);
    return HISPMV_OK;
}

HISPMV_API int hispmv_gk_info(const hispmv_ctx* c, int idx, int64_t ncv, int64_t out[8]) {
    if (!c || !out || idx < 0 || idx >= (int)c->mats.size() || ncv < 2 || ncv > kM) return HISPMV_EINVAL;
    for (int i = 0; i < 8; ++i) out[i] = 0;
    const Matrix& m = *c->mats[(size_t)idx];
    if (!m.loaded || (!m.companion && !transposable_handle(m))) return HISPMV_OK;
    const LanczosLayout l = gk_layout(m.rows, m.cols, ncv);
    out[0] = 1; out[1] = l.work_bytes; out[2] = l.off_v; out[3] = l.stride; out[4] = l.off_u; out[5] = l.stride_u; out[6] = l.off_hc; out[7] = l.off_yt;
    return HISPMV_OK;
}

HISPMV_API int hispmv_gk_steps_device(hispmv_ctx* c, int idx, int64_t ncv, int64_t j0, int64_t j1, int first, const float* d_v0, void* d_work,
                                      int64_t work_bytes, void* stream) {
    if (!c) return HISPMV_EINVAL;
    Gk v;
    const std::string w("gk_steps_device");
    {
        std::lock_guard<std::mutex> g(c->mu);
        if (ncv < 2 || ncv > kM) return fail(c, HISPMV_EINVAL, w + ": ncv must be 2 .. " + std::to_string(kM));
        if (j0 < 0 || j1 <= j0 || j1 > ncv) return fail(c, HISPMV_EINVAL, w + ": steps j0 .. j1 - 1 need 0 <= j0 < j1 <= ncv");
        if (first && j0 != 0) return fail(c, HISPMV_EINVAL, w + ": a first call starts at step 0");
        if (const int rc = krylov_check_operands(c, w, first && !d_v0, d_v0, nullptr)) return rc;
        if (const int rc = gk_enter(c, "gk_steps_device", idx, 0, ncv, d_work, work_bytes, stream, v)) return rc;
    }
    if (first)
        if (const int rc = v.open(d_v0)) return rc;
    return v.steps(j0, j1);
}

HISPMV_API int hispmv_gk_status(hispmv_ctx* c, const void* d_work, void* stream, int64_t out[5]) {
    if (!c || !out) return HISPMV_EINVAL;
    double S[kKrylovState];
    if (const int rc = thick_restart_status(c, "gk_status", d_work, stream, S)) return rc;
    out[0] = (int64_t)S[kLsSteps]; out[1] = S[kLsInvariant] != 0.0; out[2] = S[kLsClosedU] != 0.0; out[3] = S[kKsBreakdown] != 0.0;
    out[4] = (int64_t)S[kKsProducts];
    return HISPMV_OK;
}

HISPMV_API int hispmv_svds_device(hispmv_ctx* c, int idx, int64_t k, int64_t ncv, double tol, int64_t max_products, const float* d_v0, int vectors,
                                  float* d_u, int64_t ld_u, float* d_v, int64_t ld_v, double* s_out, double* res_out, void* d_work, int64_t work_bytes,
                                  void* stream, hispmv_eigsh_result* result) {
    if (!c || !result) return HISPMV_EINVAL;
    Gk v;
    const std::string w("svds_device");
    {
        std::lock_guard<std::mutex> g(c->mu);
        if (k < 1) return fail(c, HISPMV_EINVAL, w + ": k must be at least 1");
        if (ncv < k + 1 || ncv > kM) return fail(c, HISPMV_EINVAL, w + ": ncv must be k + 1 .. " + std::to_string(kM));
        if (!(tol >= 0.0)) return fail(c, HISPMV_EINVAL, w + ": tol must not be negative");
        if (max_products < 2 || max_products > (1LL << 30)) return fail(c, HISPMV_EINVAL, w + ": max_products must be at least 2 (and at most 2^30)");
        if (!s_out || !res_out) return fail(c, HISPMV_EINVAL, w + ": s_out and res_out must not be NULL");
        if (const int rc = krylov_check_operands(c, w, !d_v0 || (vectors && (!d_u || !d_v)), d_v0, d_u, d_v)) return rc;
        if (const int rc = gk_enter(c, "svds_device", idx, k, ncv, d_work, work_bytes, stream, v)) return rc;
        if (vectors && (ld_u < v.rows || ld_v < v.cols)) return fail(c, HISPMV_EINVAL, w + ": ld_u must be at least rows and ld_v at least cols");
    }
    v.vectors = vectors; v.d_u = d_u; v.ld_u = ld_u; v.d_v = d_v; v.ld_v = ld_v;
    v.P.assign((size_t)kM * kC, 0.0); v.Pt.resize((size_t)kM * kM); v.Qt.resize((size_t)kM * kC); v.vals.resize(kM); v.res.resize(kM);
    return thick_restart_run(v, k, ncv, tol, max_products, d_v0, s_out, res_out, result);
}
