// hispmv_krylov_abi.cpp -- the Krylov entries of the C ABI (include/hispmv.h: hispmv_prep_krylov_groups, hispmv_krylov_info,
// hispmv_dot_device, hispmv_cg_device, hispmv_bicgstab_device, hispmv_cgls_device, hispmv_krylov_status) over the launchers of
// hispmv_krylov.h.  A translation unit of its own: the solve loop (krylov_run, hispmv_krylov_solve.h) issues its products through
// hispmv_spmv_device and hispmv_spmv_device_t like any caller (so the context's lock is held for the argument checks only), runs
// everything between two products in the vector kernels, and keeps its whole state in the caller's workspace.
#include "hispmv_krylov_solve.h"

using namespace hispmv;

namespace {

// The workspace: two scalar blocks (a kernel reads one and writes the other), one double for hispmv_dot_device-style results, the
// partial arrays, then the solver's vectors, each of `stride` floats (a multiple of 4: every one 16-byte aligned).
constexpr int64_t kStateBytes = kKrylovState * 8;
constexpr int64_t kScratchOff = 2 * kStateBytes;
constexpr int64_t kPartsOff = 512;
constexpr int64_t kVecsOff = kPartsOff + (int64_t)kKrylovSlots * kKrylovMaxGroups * 8;
const char* const kNames[3] = {"cg_device", "bicgstab_device", "cgls_device"};

int64_t stride_of(const Matrix& m) { return ((int64_t)std::max(m.rows, m.cols) + 3) / 4 * 4; }
int64_t work_bytes_of(const Matrix& m, int solver) { return kVecsOff + kKrylovVectors[solver] * stride_of(m) * 4; }
bool accepts(const Matrix& m, int solver) {
    if (!m.loaded) return false;
    return solver == HISPMV_KRYLOV_CGLS ? (m.companion || transposable_handle(m)) : m.rows == m.cols;
}

// The single-vector backend of krylov_run: products through hispmv_spmv_device and hispmv_spmv_device_t, one scalar block, one result.
struct Solve : KrylovSolve {
    static constexpr bool kCgls = true;
    int64_t rows = 0, cols = 0, stride = 0;          // elements of b; of x
    hispmv_krylov_result* result = nullptr;
    KrylovStep base;

    float* vec(int i) const { return (float*)(work + kVecsOff) + i * stride; }
    double* state(int64_t which) const { return (double*)(work + which * kStateBytes); }
    double* parts() const { return (double*)(work + kPartsOff); }
    double* slot(int k) const { return parts() + (int64_t)k * kKrylovMaxGroups; }
    int product(const float* x, float* y) { ++products; return hispmv_spmv_device(c, idx, x, nullptr, y, 1.0f, 0.0f, stream_arg); }
    int product_t(const float* x, float* y) { ++products; return hispmv_spmv_device_t(c, idx, x, nullptr, y, 1.0f, 0.0f, stream_arg); }
    int residual(float* r) { ++products; return hispmv_spmv_device(c, idx, d_x, d_b, r, -1.0f, 1.0f, stream_arg); }
    int dot_bb() { LAUNCH_TRY(c, launch_krylov_dot, d_b, d_b, rows, slot(kSlotB2), s); return HISPMV_OK; }
    // one look at (b, b); zero: x = 0
    int zero_rhs(bool* zero) {
        double* d_scratch = (double*)(work + kScratchOff);
        LAUNCH_TRY(c, launch_krylov_dot_finish, slot(kSlotB2), krylov_groups(rows), d_scratch, s);
        HIP_TRY(c, hipMemcpyAsync(pinned, d_scratch, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        *zero = pinned[0] == 0.0;
        if (*zero) HIP_TRY(c, hipMemsetAsync(d_x, 0, (size_t)cols * 4, s));
        return HISPMV_OK;
    }
    // CGLS: sv = A^T b and the partials of (sv, sv)
    int reference(float* sv) {
        if (const int rc = product_t(d_b, sv)) return rc;
        LAUNCH_TRY(c, launch_krylov_dot, sv, sv, cols, slot(kSlotBb), s);
        return HISPMV_OK;
    }
    // the three kernels that precondition: bs = 0, d_minv an inverse diagonal; bs > 0 (hispmv_cg_bj_device), the block area of a buffer
    int bs = 0;
    int init(const KrylovStep& k) { LAUNCH_TRY(c, launch_krylov_init, k, s, bs); return HISPMV_OK; }
    int cg_update(const KrylovStep& k) { LAUNCH_TRY(c, launch_krylov_cg_update, k, s, bs); return HISPMV_OK; }
    int direction(const KrylovStep& k) { LAUNCH_TRY(c, launch_krylov_direction, k, s, bs); return HISPMV_OK; }
    KRYLOV_LAUNCHER(step_dot, launch_krylov_step_dot)
    KRYLOV_LAUNCHER(cgls_update, launch_krylov_cgls_update)
    KRYLOV_LAUNCHER(bicg_s, launch_krylov_bicg_s)
    KRYLOV_LAUNCHER(bicg_x, launch_krylov_bicg_x)
    KRYLOV_LAUNCHER(bicg_p, launch_krylov_bicg_p)
    // One host look at the scalar block: copy, wait, read.  *stop = the solve has ended on the device.
    int check(bool* stop) {
        HIP_TRY(c, hipMemcpyAsync(pinned, state(current()), kStateBytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        *stop = pinned[kKsDone] != 0.0 || pinned[kKsBreakdown] != 0.0;
        return HISPMV_OK;
    }
    void report(const hispmv_krylov_result& r) { *result = r; }
    void report_looked() { fill_result(pinned, false, products, result); }
};

// bs > 0 (hispmv_cg_bj_device): d_minv is the block-Jacobi buffer of that block size, 16-byte aligned, and may not be NULL
int solve(hispmv_ctx* c, int idx, int solver, const float* d_b, float* d_x, const float* d_minv, double rtol, int64_t max_iters, int64_t check_every,
          void* d_work, int64_t work_bytes, void* stream, hispmv_krylov_result* result, int64_t bs = 0) {
    if (!c || !result) return HISPMV_EINVAL;
    Solve v;
    const char* const name = bs != 0 ? "cg_bj_device" : kNames[solver];
    const std::string w(name);
    const bool cgls = solver == HISPMV_KRYLOV_CGLS;
    {
        std::lock_guard<std::mutex> g(c->mu);
        if (const int rc = krylov_check_scalars(c, w, rtol, max_iters, check_every)) return rc;
        Matrix* mp = nullptr;
        if (const int rc = find_handle(c, idx, name, &mp)) return rc;
        const Matrix& m = *mp;
        if (!cgls)
            if (const int rc = krylov_check_square(c, w, m)) return rc;
        if (cgls && !m.companion && !transposable_handle(m)) return refuse_tile_stream(c, m, kNames[solver], "transposed product");
        if (bs != 0)
            if (const int rc = krylov_check_blocks(c, w, d_minv, bs)) return rc;
        if (const int rc = krylov_check_operands(c, w, !d_b || !d_x, d_b, d_x, d_minv)) return rc;
        if (const int rc = krylov_check_work(c, w, d_work, work_bytes, work_bytes_of(m, solver), "hispmv_krylov_info asks for")) return rc;
        if (const int rc = adopt_stream(c, stream, &v.s)) return rc;
        v.rows = m.rows; v.cols = m.cols; v.stride = stride_of(m);
    }
    v.c = c; v.idx = idx; v.solver = solver; v.max_iters = max_iters; v.check_every = check_every; v.work = (char*)d_work; v.stream_arg = stream;
    v.d_b = d_b; v.d_x = d_x; v.d_minv = d_minv; v.result = result; v.bs = (int)bs;
    v.blocks.kernels = 1 + max_iters * kKrylovLaunches[solver];
    v.base.n = v.cols; v.base.n2 = v.rows; v.base.x = d_x; v.base.parts = v.parts(); v.base.tol2 = rtol * rtol;
    v.base.slot_bb = cgls ? kSlotBb : kSlotB2;
    v.base.products = (double)((cgls ? 3 : 1) + max_iters * (kKrylovProducts[solver] + kKrylovProductsT[solver]));
    if (check_every > 0) HIP_TRY(c, hipHostMalloc((void**)&v.pinned, kStateBytes, hipHostMallocDefault));
    return krylov_run(v);
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
    out[0] = 1; out[1] = work_bytes_of(m, solver); out[2] = kKrylovLaunches[solver]; out[3] = kKrylovProducts[solver]; out[4] = kKrylovProductsT[solver];
    out[5] = kVecsOff; out[6] = m.cols; out[7] = m.rows;
    return HISPMV_OK;
}

HISPMV_API int hispmv_dot_device(hispmv_ctx* c, int64_t n, const float* d_a, const float* d_b, double* d_out, void* d_work, int64_t work_bytes, void* stream) {
    if (!c) return HISPMV_EINVAL;
    hipStream_t s;
    const std::string w("dot_device");
    {
        std::lock_guard<std::mutex> g(c->mu);
        if (n < 0) return fail(c, HISPMV_EINVAL, w + ": n must not be negative");
        if (const int rc = krylov_check_dot(c, w, n, d_a, d_b, d_out)) return rc;
        if (const int rc = krylov_check_work(c, w, d_work, work_bytes, krylov_groups(n) * 8, "the " + std::to_string(krylov_groups(n)) + " partials take")) return rc;
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

HISPMV_API int hispmv_cg_bj_device(hispmv_ctx* c, int idx, const float* d_b, float* d_x, const void* d_pre, int64_t block_size, double rtol, int64_t max_iters,
                                   int64_t check_every, void* d_work, int64_t work_bytes, void* stream, hispmv_krylov_result* result) {
    if (block_size == 0) return c ? fail(c, HISPMV_EINVAL, "cg_bj_device: block_size must be 4, 8, 16 or 32") : HISPMV_EINVAL;
    return solve(c, idx, HISPMV_KRYLOV_CG, d_b, d_x, (const float*)d_pre, rtol, max_iters, check_every, d_work, work_bytes, stream, result, block_size);
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
