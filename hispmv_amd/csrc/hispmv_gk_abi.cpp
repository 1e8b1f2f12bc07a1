// hispmv_gk_abi.cpp -- the thick-restart Golub-Kahan entries of the C ABI (include/hispmv.h: hispmv_prep_gk, hispmv_prep_bsvd,
// hispmv_gk_info, hispmv_gk_steps_device, hispmv_gk_status, hispmv_svds_device) over the launcher of hispmv_gk.h, Lanczos's open and
// rotation and the two GMRES launchers a step shares.  The products go through hispmv_spmv_device and hispmv_spmv_device_t like any
// caller's, the checks are hispmv_krylov_solve.h's, and the whole state of a run lies in the caller's workspace in the layout of
// gk_layout.  The host half -- the SVD of the projected matrix, its order, the stopping rule -- is hispmv_prep_bsvd, which needs no
// device.
#include <algorithm>
#include <numeric>
#include <vector>

#include "hispmv_gk.h"
#include "hispmv_krylov_solve.h"

using namespace hispmv;

namespace {

constexpr int kM = kGkMaxNcv;
constexpr int kC = kGkMaxNcv + 1;          // columns of the widest projected matrix
constexpr int64_t kStateBytes = kKrylovState * 8;

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

// The order of launches of a run.  A step: the forward product into U slot j, the multi-dot pass over U slots 0 .. j - 1, the
// subtract-and-dot kernel twice, the U side's record kernel (j = 0: the dot kernel and the record kernel); the transposed product into V
// slot j + 1, the multi-dot pass over V slots 0 .. j, the subtract-and-dot kernel twice, the V side's record kernel.  The kernels of a
// step that write the scalar block pass it on by ONE rule: a kernel reads the block the kernel before it wrote; every kernel but the
// last writes block 1 or 2, whichever it does not read; the last -- the V side's record kernel -- writes block 0.  The kernel before
// the last wrote 1 or 2, so no kernel writes the block it reads, whether a step has six such kernels (0 -> 1 -> 2 -> 1 -> 2 -> 1 -> 0)
// or, at j = 0, four (0 -> 1 -> 2 -> 1 -> 0), and every step -- so every call -- leaves the state in block 0.
struct Gk : KrylovSolve {
    int64_t rows = 0, cols = 0;
    GkLayout l;
    int cur = 0;

    template <class P> P* at(int64_t off) const { return (P*)(work + off); }
    double* state(int64_t which) const { return at<double>(which * kStateBytes); }
    float* vvec(int64_t i) const { return at<float>(l.off_v) + i * l.stride_v; }
    float* uvec(int64_t i) const { return at<float>(l.off_u) + i * l.stride_u; }
    template <class K> void turn(K& k, bool last = false) {
        k.s_in = state(cur);
        cur = last ? 0 : cur == 1 ? 2 : 1;
        k.s_out = state(cur);
    }
    // side 0: the U basis, n = rows; side 1: the V basis, n = cols.  j = the index GmresStep counts with: w is basis vector j + 1
    GmresStep gstep(int side, int64_t j, bool second) {
        GmresStep k;
        k.n = side ? cols : rows; k.j = (int)j; k.second = second; k.gp = l.gp; k.V = side ? vvec(0) : uvec(0); k.stride = side ? l.stride_v : l.stride_u;
        k.parts_in = at<double>(second ? l.off_pb : l.off_pa); k.parts_out = at<double>(l.off_pb); k.part_ww = at<double>(l.off_ww);
        k.h1 = at<double>(l.off_g1); k.h = at<double>(l.off_g);
        turn(k);
        return k;
    }
    GkStep rstep(int side, int64_t j) {
        GkStep k;
        k.n = side ? cols : rows; k.j = (int)j; k.W = side ? vvec(0) : uvec(0); k.stride = side ? l.stride_v : l.stride_u;
        k.part = at<double>(l.off_ww); k.g = at<double>(l.off_g);
        k.Gc = at<double>(l.off_gc); k.alpha = at<double>(l.off_alpha); k.beta = at<double>(l.off_beta);
        turn(k, side == 1);
        return k;
    }
    int open(const float* d_v0) {
        LAUNCH_TRY(c, launch_krylov_dot, d_v0, d_v0, cols, at<double>(l.off_vv), s);
        LanczosStep k;          // Lanczos's open on V slot 0: the block from nothing, into block 0
        k.n = cols; k.V = vvec(0); k.stride = l.stride_v; k.v0 = d_v0; k.part = at<double>(l.off_vv);
        k.s_in = state(0); k.s_out = state(cur = 0);
        LAUNCH_TRY(c, launch_lanczos_open, k, s);
        return HISPMV_OK;
    }
    int steps(int64_t j0, int64_t j1) {
        for (int64_t j = j0; j < j1; ++j) {
            if (const int rc = hispmv_spmv_device(c, idx, vvec(j), nullptr, uvec(j), 1.0f, 0.0f, stream_arg)) return rc;
            if (j == 0) {
                LAUNCH_TRY(c, launch_krylov_dot, uvec(0), uvec(0), rows, at<double>(l.off_ww), s);
            } else {
                LAUNCH_TRY(c, launch_gmres_multi_dot, uvec(0), l.stride_u, j, uvec(j), rows, at<double>(l.off_pa), l.gp, state(cur), s);
                LAUNCH_TRY(c, launch_gmres_sub, gstep(0, j - 1, false), s);
                LAUNCH_TRY(c, launch_gmres_sub, gstep(0, j - 1, true), s);
            }
            LAUNCH_TRY(c, launch_gk_record, rstep(0, j), 0, s);
            if (const int rc = hispmv_spmv_device_t(c, idx, uvec(j), nullptr, vvec(j + 1), 1.0f, 0.0f, stream_arg)) return rc;
            LAUNCH_TRY(c, launch_gmres_multi_dot, vvec(0), l.stride_v, j + 1, vvec(j + 1), cols, at<double>(l.off_pa), l.gp, state(cur), s);
            LAUNCH_TRY(c, launch_gmres_sub, gstep(1, j, false), s);
            LAUNCH_TRY(c, launch_gmres_sub, gstep(1, j, true), s);
            LAUNCH_TRY(c, launch_gk_record, rstep(1, j), 1, s);
        }
        return HISPMV_OK;
    }
};

// what the two entries that take a handle and a workspace check alike; fills v
int gk_enter(hispmv_ctx* c, const char* name, int idx, int64_t k, int64_t basis_ncv, const void* d_work, int64_t work_bytes, void* stream, Gk& v) {
    const std::string w(name);
    Matrix* mp = nullptr;
    if (const int rc = find_handle(c, idx, name, &mp)) return rc;
    const Matrix& m = *mp;
    if (!m.companion && !transposable_handle(m)) return refuse_tile_stream(c, m, "spmv_device_t", "transposed product");
    if (k > std::min(m.rows, m.cols))
        return fail(c, HISPMV_EINVAL, w + ": the handle is " + std::to_string(m.rows) + " x " + std::to_string(m.cols) + ", k must be at most the smaller of the two");
    v.rows = m.rows; v.cols = m.cols;
    v.l = gk_layout(v.rows, v.cols, basis_ncv);
    if (const int rc = krylov_check_work(c, w, d_work, work_bytes, v.l.work_bytes, "hispmv_gk_info asks for")) return rc;
    if (const int rc = adopt_stream(c, stream, &v.s)) return rc;
    v.c = c; v.idx = idx; v.work = (char*)d_work; v.stream_arg = stream;
    return HISPMV_OK;
}

}  // namespace

HISPMV_API int hispmv_prep_gk(int64_t rows, int64_t cols, int64_t ncv, int64_t out[8]) {
    if (!out || rows < 0 || cols < 0 || ncv < 2 || ncv > kGkMaxNcv) return HISPMV_EINVAL;
    const GkLayout l = gk_layout(rows, cols, ncv);
    out[0] = l.work_bytes; out[1] = l.off_v; out[2] = l.stride_v; out[3] = l.off_u; out[4] = l.stride_u; out[5] = l.off_gc; out[6] = l.off_yt;
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
    if (!c || !out || idx < 0 || idx >= (int)c->mats.size() || ncv < 2 || ncv > kGkMaxNcv) return HISPMV_EINVAL;
    for (int i = 0; i < 8; ++i) out[i] = 0;
    const Matrix& m = *c->mats[(size_t)idx];
    if (!m.loaded || (!m.companion && !transposable_handle(m))) return HISPMV_OK;
    const GkLayout l = gk_layout(m.rows, m.cols, ncv);
    out[0] = 1; out[1] = l.work_bytes; out[2] = l.off_v; out[3] = l.stride_v; out[4] = l.off_u; out[5] = l.stride_u; out[6] = l.off_gc; out[7] = l.off_yt;
    return HISPMV_OK;
}

HISPMV_API int hispmv_gk_steps_device(hispmv_ctx* c, int idx, int64_t ncv, int64_t j0, int64_t j1, int first, const float* d_v0, void* d_work,
                                      int64_t work_bytes, void* stream) {
    if (!c) return HISPMV_EINVAL;
    Gk v;
    const std::string w("gk_steps_device");
    {
        std::lock_guard<std::mutex> g(c->mu);
        if (ncv < 2 || ncv > kGkMaxNcv) return fail(c, HISPMV_EINVAL, w + ": ncv must be 2 .. " + std::to_string(kGkMaxNcv));
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
    hipStream_t s;
    {
        std::lock_guard<std::mutex> g(c->mu);
        if (!d_work || ((uintptr_t)d_work & 15)) return fail(c, HISPMV_EINVAL, "gk_status: the workspace must be the 16-byte aligned one of the run");
        if (const int rc = adopt_stream(c, stream, &s)) return rc;
    }
    double S[kKrylovState];
    HIP_TRY(c, hipStreamSynchronize(s));
    HIP_TRY(c, hipMemcpy(S, d_work, kStateBytes, hipMemcpyDeviceToHost));          // block 0: where every call leaves the state
    out[0] = (int64_t)S[kGkSteps]; out[1] = S[kGkInvariant] != 0.0; out[2] = S[kGkClosedU] != 0.0; out[3] = S[kKsBreakdown] != 0.0;
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
        if (ncv < k + 1 || ncv > kGkMaxNcv) return fail(c, HISPMV_EINVAL, w + ": ncv must be k + 1 .. " + std::to_string(kGkMaxNcv));
        if (!(tol >= 0.0)) return fail(c, HISPMV_EINVAL, w + ": tol must not be negative");
        if (max_products < 2 || max_products > (1LL << 30)) return fail(c, HISPMV_EINVAL, w + ": max_products must be at least 2 (and at most 2^30)");
        if (!s_out || !res_out) return fail(c, HISPMV_EINVAL, w + ": s_out and res_out must not be NULL");
        if (const int rc = krylov_check_operands(c, w, !d_v0 || (vectors && (!d_u || !d_v)), d_v0, d_u, d_v)) return rc;
        if (const int rc = gk_enter(c, "svds_device", idx, k, ncv, d_work, work_bytes, stream, v)) return rc;
        if (vectors && (ld_u < v.rows || ld_v < v.cols)) return fail(c, HISPMV_EINVAL, w + ": ld_u must be at least rows and ld_v at least cols");
    }
    // pinned: the scalar block, then Gc, the alphas and the betas as the workspace holds them, then the fp32 coefficients of the two
    // rotations of a look -- one area each, because the second is filled while the copy of the first may still be in flight
    const int64_t gc_doubles = (int64_t)(kM + 2) * kGkGcLd, yt_floats = (int64_t)kRotateMaxOut * kRotateMaxIn;
    HIP_TRY(c, hipHostMalloc((void**)&v.pinned, (size_t)((kKrylovState + gc_doubles) * 8 + 2 * yt_floats * 4), hipHostMallocDefault));
    const double* S = v.pinned;
    const double *Gc = v.pinned + kKrylovState, *alphas = Gc + (int64_t)kM * kGkGcLd, *betas = alphas + kGkGcLd;
    float* y32 = (float*)(v.pinned + kKrylovState + gc_doubles);
    std::vector<double> B((size_t)kM * kC, 0.0), Pt((size_t)kM * kM), Qt((size_t)kM * kC), sv(kM), res(kM);
    const int n_cv = (int)ncv, kk = (int)k;
    int64_t cycles = 0, counts[2] = {0, 0};
    *result = hispmv_eigsh_result{HISPMV_KRYLOV_BREAKDOWN, 0, 0, 0, 0.0};
    if (const int rc = v.open(d_v0)) return rc;
    // the coefficients of `outs` vectors over `ins` basis vectors (rows of Y, `ins` long) into the workspace, then the rotation into out
    auto rotate = [&](int side, const double* Y, int ins, int outs, float* out, int64_t ld_out, const float* xsrc, float* xdst) -> int {
        float* y = y32 + side * yt_floats;
        for (int col = 0; col < outs; ++col)
            for (int i = 0; i < ins; ++i) y[col * ins + i] = (float)Y[(size_t)col * ins + i];
        HIP_TRY(c, hipMemcpyAsync(v.at<float>(v.l.off_yt), y, (size_t)outs * ins * 4, hipMemcpyHostToDevice, v.s));
        LAUNCH_TRY(c, launch_basis_rotate, side ? v.vvec(0) : v.uvec(0), side ? v.l.stride_v : v.l.stride_u, ins, outs, v.at<float>(v.l.off_yt), out, ld_out,
                   side ? v.cols : v.rows, xsrc, xdst, v.s);
        return HISPMV_OK;
    };
    for (int j0 = 0;;) {
        if (const int rc = v.steps(j0, n_cv)) return rc;
        ++cycles;
        HIP_TRY(c, hipMemcpyAsync(v.pinned, v.state(0), kStateBytes, hipMemcpyDeviceToHost, v.s));
        HIP_TRY(c, hipMemcpyAsync(v.pinned + kKrylovState, v.at<double>(v.l.off_gc), (size_t)gc_doubles * 8, hipMemcpyDeviceToHost, v.s));
        HIP_TRY(c, hipStreamSynchronize(v.s));
        result->products = (int64_t)S[kKsProducts];
        result->cycles = cycles;
        const int m = (int)S[kGkSteps];
        const bool closed = S[kGkClosedU] != 0.0, invariant = S[kGkInvariant] != 0.0;
        if (S[kKsBreakdown] != 0.0 || m < 0 || m > n_cv || (m == 0 && !closed)) return HISPMV_OK;          // BREAKDOWN: d_u and d_v untouched
        if (m == 0) {          // A v0 = 0: nothing found, and no breakdown
            result->status = HISPMV_KRYLOV_INVARIANT;
            return HISPMV_OK;
        }
        const int mc = closed ? m + 1 : m;
        for (int j = j0; j < mc; ++j) {
            for (int i = 0; i < j && i < m; ++i) B[(size_t)i * kC + j] = Gc[(int64_t)j * kGkGcLd + i];
            if (j < m) B[(size_t)j * kC + j] = alphas[j];
        }
        result->scale = bsvd(B.data(), kC, m, mc, kk, closed ? 0.0 : betas[m - 1], tol, sv.data(), Pt.data(), Qt.data(), res.data(), counts);
        const int found = std::min(kk, m);
        int status = -1;
        if (counts[0] == found && m >= kk) status = HISPMV_KRYLOV_CONVERGED;
        else if (invariant) status = HISPMV_KRYLOV_INVARIANT;
        else if (result->products >= max_products) status = HISPMV_KRYLOV_MAX_ITERS;
        if (status >= 0) {
            for (int i = 0; i < found; ++i) { s_out[i] = sv[i]; res_out[i] = res[i]; }
            if (vectors) {
                if (const int rc = rotate(0, Pt.data(), m, found, d_u, ld_u, nullptr, nullptr)) return rc;
                if (const int rc = rotate(1, Qt.data(), mc, found, d_v, ld_v, nullptr, nullptr)) return rc;
            }
            HIP_TRY(c, hipStreamSynchronize(v.s));
            result->status = status; result->found = found;
            return HISPMV_OK;
        }
        const int keep = std::min(kk + (n_cv - kk) / 2, n_cv - 1);
        if (const int rc = rotate(0, Pt.data(), m, keep, v.uvec(0), v.l.stride_u, nullptr, nullptr)) return rc;
        if (const int rc = rotate(1, Qt.data(), m, keep, v.vvec(0), v.l.stride_v, v.vvec(m), v.vvec(keep))) return rc;
        std::fill(B.begin(), B.end(), 0.0);
        for (int i = 0; i < keep; ++i) B[(size_t)i * kC + i] = sv[i];
        j0 = keep;
    }
}
