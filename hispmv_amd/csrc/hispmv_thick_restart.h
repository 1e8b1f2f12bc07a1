// hispmv_thick_restart.h -- what the two thick-restart backends share on the host (hispmv_lanczos_abi.cpp: Lanczos, eigsh;
// hispmv_gk_abi.cpp: Golub-Kahan, svds): the rule that passes the scalar block from kernel to kernel, the open, the orthogonalisation
// and the record launch of a step's work on one basis, the rotation of a basis, the checks of the entries, the status look, and
// thick_restart_run, THE driver loop.  A backend derives from ThickRestart and supplies its bases and products (steps), how it reads a
// look, its small decomposition and which bases it rotates; the decompositions stay beside their backend.
#pragma once
#include <algorithm>

#include "hispmv_krylov_solve.h"
#include "hispmv_lanczos.h"

namespace hispmv {

constexpr int64_t kThickStateBytes = kKrylovState * 8;
constexpr int64_t kThickYtFloats = (int64_t)kRotateMaxOut * kRotateMaxIn;          // the fp32 coefficients of one rotation

struct ThickRestart : KrylovSolve {
    LanczosLayout l;
    int cur = 0;          // the block the last kernel wrote; 0 between steps, so at the start of every call

    template <class P> P* at(int64_t off) const { return (P*)(work + off); }
    double* state(int64_t which) const { return at<double>(which * kThickStateBytes); }
    // The kernels of a step that write the scalar block pass it on by ONE rule: a kernel reads the block the kernel before it wrote;
    // every kernel but the last of the step writes block 1 or 2, whichever it does not read; the last -- the record kernel of the step's
    // last basis -- writes block 0.  The kernel before the last wrote 1 or 2, so no kernel writes the block it reads, however many such
    // kernels a step has: Lanczos's three (0 -> 1 -> 2 -> 0), Golub-Kahan's six (0 -> 1 -> 2 -> 1 -> 2 -> 1 -> 0) or, at j = 0, four
    // (0 -> 1 -> 2 -> 1 -> 0); and every step -- so every call -- leaves the state in block 0, which the open kernel writes, the
    // multi-dot kernel and the next step read and the status entries report.
    template <class K> void turn(K& k, bool last) {
        k.s_in = state(cur);
        cur = last ? 0 : cur == 1 ? 2 : 1;
        k.s_out = state(cur);
    }
    // the block from nothing, into block 0; slot 0 of `basis` = v0 / |v0|
    int open(const float* d_v0, int64_t n, float* basis, int64_t stride) {
        LAUNCH_TRY(c, launch_krylov_dot, d_v0, d_v0, n, at<double>(l.off_vv), s);
        RecordStep k;
        k.n = n; k.V = basis; k.stride = stride; k.v0 = d_v0; k.part = at<double>(l.off_vv);
        k.s_in = state(0); k.s_out = state(cur = 0);
        LAUNCH_TRY(c, launch_lanczos_open, k, s);
        return HISPMV_OK;
    }
    // w = slot j + 1 of `basis` against slots 0 .. j: the multi-dot pass and the subtract-and-dot kernel twice, h = h1 + h2 (GMRES's
    // kernels as they are: j is the index GmresStep counts with)
    int orthogonalise(int64_t n, float* basis, int64_t stride, int64_t j) {
        LAUNCH_TRY(c, launch_gmres_multi_dot, basis, stride, j + 1, basis + (j + 1) * stride, n, at<double>(l.off_pa), l.gp, state(cur), s);
        for (int second = 0; second < 2; ++second) {
            GmresStep k;
            k.n = n; k.j = (int)j; k.second = second; k.gp = l.gp; k.V = basis; k.stride = stride;
            k.parts_in = at<double>(second ? l.off_pb : l.off_pa); k.parts_out = at<double>(l.off_pb); k.part_ww = at<double>(l.off_ww);
            k.h1 = at<double>(l.off_h1); k.h = at<double>(l.off_h);
            turn(k, false);
            LAUNCH_TRY(c, launch_gmres_sub, k, s);
        }
        return HISPMV_OK;
    }
    // the record kernel of step j on `basis` behind the partials of (w, w); last: the step's last kernel
    int record(int64_t n, float* basis, int64_t stride, int64_t j, RecordRule rule, double* alpha, bool last) {
        RecordStep k;
        k.n = n; k.j = (int)j; k.V = basis; k.stride = stride; k.part = at<double>(l.off_ww); k.h = at<double>(l.off_h);
        k.Hc = at<double>(l.off_hc); k.beta = at<double>(l.off_beta); k.alpha = alpha;
        turn(k, last);
        LAUNCH_TRY(c, launch_basis_record, k, rule, s);
        return HISPMV_OK;
    }
    // The coefficients of `outs` vectors over the first `ins` of `basis` (rows of Y, `ins` long) through `y32`, a pinned area of
    // kThickYtFloats, into the workspace, then the rotation into out.  The copy is asynchronous: two rotations of one look take an
    // area each, because the second is filled while the copy of the first may still be in flight.
    int rotate(float* y32, const double* Y, int64_t n, const float* basis, int64_t stride, int ins, int outs, float* out, int64_t ld_out, const float* xsrc,
               float* xdst) {
        for (int col = 0; col < outs; ++col)
            for (int i = 0; i < ins; ++i) y32[col * ins + i] = (float)Y[(size_t)col * ins + i];
        HIP_TRY(c, hipMemcpyAsync(at<float>(l.off_yt), y32, (size_t)outs * ins * 4, hipMemcpyHostToDevice, s));
        LAUNCH_TRY(c, launch_basis_rotate, basis, stride, ins, outs, at<float>(l.off_yt), out, ld_out, n, xsrc, xdst, s);
        return HISPMV_OK;
    }
};

// What the entries that take a handle and a workspace check alike, under the context's lock; fills v.  shape(m): the solver's own
// checks of the handle, between the handle's and the workspace's as the first error of a bad call has it; it sets v.l.
template <class Shape>
int thick_restart_enter(hispmv_ctx* c, const char* name, int idx, const void* d_work, int64_t work_bytes, const char* asks, void* stream, ThickRestart& v,
                        Shape&& shape) {
    Matrix* mp = nullptr;
    if (const int rc = find_handle(c, idx, name, &mp)) return rc;
    if (const int rc = shape(*mp)) return rc;
    if (const int rc = krylov_check_work(c, name, d_work, work_bytes, v.l.work_bytes, asks)) return rc;
    if (const int rc = adopt_stream(c, stream, &v.s)) return rc;
    v.c = c; v.idx = idx; v.work = (char*)d_work; v.stream_arg = stream;
    return HISPMV_OK;
}

// The look of the two status entries: waits for the stream and copies block 0, where every call leaves the state, into S.
inline int thick_restart_status(hispmv_ctx* c, const std::string& w, const void* d_work, void* stream, double S[kKrylovState]) {
    hipStream_t s;
    {
        std::lock_guard<std::mutex> g(c->mu);
        if (!d_work || ((uintptr_t)d_work & 15)) return fail(c, HISPMV_EINVAL, w + ": the workspace must be the 16-byte aligned one of the run");
        if (const int rc = adopt_stream(c, stream, &s)) return rc;
    }
    HIP_TRY(c, hipStreamSynchronize(s));
    HIP_TRY(c, hipMemcpy(S, d_work, kThickStateBytes, hipMemcpyDeviceToHost));
    return HISPMV_OK;
}

// The driver: cycles of steps j0 .. ncv - 1, one look per cycle, until the stopping rule ends the run; called behind the entry's
// checks, outside the context's lock.  The backend B supplies
//   kLookDoubles, kRotations   the doubles behind the scalar block a look copies from off_hc on; the rotations of one look
//   open(d_v0), steps(j0, j1)  its launches
//   verdict(S, ncv, &m, &invariant, result)   reads the block; false ends the run as result stands (BREAKDOWN unless it says otherwise)
//   P, kLd                     its projected matrix, zero at the start, and the doubles between two of its rows
//   project(look, j0, m)       the columns j0 .. of the look into P
//   decompose(look, m, k, tol, counts)   its small decomposition of P into vals and res; returns the scale
//   finish(y32, m, found), restart(y32, m, keep)   its rotations, into the caller's vectors or in place
template <class B>
int thick_restart_run(B& v, int64_t k, int64_t ncv, double tol, int64_t max_products, const float* d_v0, double* vals_out, double* res_out,
                      hispmv_eigsh_result* result) {
    hipStream_t s = v.s;
    hispmv_ctx* c = v.c;
    // pinned: the scalar block, then the look as the workspace holds it, then the fp32 coefficients of a look's rotations
    HIP_TRY(c, hipHostMalloc((void**)&v.pinned, (size_t)((kKrylovState + B::kLookDoubles) * 8 + B::kRotations * kThickYtFloats * 4), hipHostMallocDefault));
    const double *S = v.pinned, *look = v.pinned + kKrylovState;
    float* y32 = (float*)(v.pinned + kKrylovState + B::kLookDoubles);
    const int n_cv = (int)ncv, kk = (int)k;
    int64_t cycles = 0, counts[2] = {0, 0};
    *result = hispmv_eigsh_result{HISPMV_KRYLOV_BREAKDOWN, 0, 0, 0, 0.0};
    if (const int rc = v.open(d_v0)) return rc;
    for (int j0 = 0;;) {
        if (const int rc = v.steps(j0, n_cv)) return rc;
        ++cycles;
        HIP_TRY(c, hipMemcpyAsync(v.pinned, v.state(0), kThickStateBytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(v.pinned + kKrylovState, v.template at<double>(v.l.off_hc), (size_t)B::kLookDoubles * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        result->products = (int64_t)S[kKsProducts];
        result->cycles = cycles;
        int m = 0;
        bool invariant = false;
        if (!v.verdict(S, n_cv, &m, &invariant, result)) return HISPMV_OK;          // the caller's vectors untouched
        v.project(look, j0, m);
        result->scale = v.decompose(look, m, kk, tol, counts);
        const int found = std::min(kk, m);
        int status = -1;
        if (counts[0] == found && m >= kk) status = HISPMV_KRYLOV_CONVERGED;
        else if (invariant) status = HISPMV_KRYLOV_INVARIANT;
        else if (result->products >= max_products) status = HISPMV_KRYLOV_MAX_ITERS;
        if (status >= 0) {
            for (int i = 0; i < found; ++i) { vals_out[i] = v.vals[i]; res_out[i] = v.res[i]; }
            if (const int rc = v.finish(y32, m, found)) return rc;
            HIP_TRY(c, hipStreamSynchronize(s));
            result->status = status; result->found = found;
            return HISPMV_OK;
        }
        const int keep = std::min(kk + (n_cv - kk) / 2, n_cv - 1);
        if (const int rc = v.restart(y32, m, keep)) return rc;
        std::fill(v.P.begin(), v.P.end(), 0.0);
        for (int i = 0; i < keep; ++i) v.P[(size_t)i * B::kLd + i] = v.vals[i];
        j0 = keep;
    }
}

}  // namespace hispmv
