// hispmv_block_jacobi_abi.cpp -- the block-Jacobi entries of the C ABI (include/hispmv.h: hispmv_block_jacobi_info, _extract_device,
// _setup_device, _status, _apply_device and hispmv_block_invert_device; the host-only hispmv_prep_block_jacobi lies in
// hispmv_prep_abi.cpp, and the two solver entries that take the buffer, hispmv_cg_bj_device and hispmv_gmres_bj_device, beside the
// loops they share with their inverse-diagonal variants in hispmv_krylov_abi.cpp and hispmv_gmres_abi.cpp) over the launchers of
// hispmv_block_jacobi.h.  Nothing is kept in the handle or the context: the preconditioner is the caller's buffer in the layout of
// block_jacobi_layout.
#include "hispmv_block_jacobi.h"
#include "hispmv_gmres.h"
#include "hispmv_krylov_solve.h"

using namespace hispmv;

namespace {

// what hispmv_krylov_abi.cpp's layout gives a CG solve of n unknowns: the scalar blocks and partials, then 3 vectors
int64_t cg_work_bytes(int64_t n) { return 512 + (int64_t)kKrylovSlots * kKrylovMaxGroups * 8 + kKrylovVectors[HISPMV_KRYLOV_CG] * ((n + 3) / 4 * 4) * 4; }

bool has_tile_stream(const Matrix& m) {
    if (m.dense) return false;
    if (m.format != 0) return true;
    for (auto& p : m.parts)
        if (p.is_tts) return true;
    return false;
}
// launches of a setup: the fill and one walk per part that holds slices (dense: one kernel), then the inversion
int64_t setup_launches(const Matrix& m) {
    int64_t n = 2;
    if (!m.dense)
        for (auto& p : m.parts) n += p.dev.n_slices > 0 && p.dev.n_groups > 0 ? 1 : 0;
    return n;
}

int check_size(hispmv_ctx* c, const std::string& w, int64_t bs) {
    if (block_jacobi_size_ok(bs)) return HISPMV_OK;
    return fail(c, HISPMV_EINVAL, w + ": block_size must be 4, 8, 16 or 32");
}
int check_buffer(hispmv_ctx* c, const std::string& w, const void* d_pre, int64_t pre_bytes, int64_t need) {
    if (!d_pre || pre_bytes < need)
        return fail(c, HISPMV_EINVAL, w + ": the buffer holds " + std::to_string(d_pre ? pre_bytes : 0) + " bytes, hispmv_prep_block_jacobi asks for " + std::to_string(need));
    if ((uintptr_t)d_pre & 15) return fail(c, HISPMV_EINVAL, w + ": the buffer must be 16-byte aligned");
    return HISPMV_OK;
}

// The checks of the extraction and of the setup, under the context's lock, all before any launch.
int extract_target(hispmv_ctx* c, const char* who, int idx, int64_t bs, const void* d_pre, int64_t pre_bytes, Matrix** out, hipStream_t* s, void* stream) {
    const std::string w(who);
    if (const int rc = find_handle(c, idx, who, out)) return rc;
    const Matrix& m = **out;
    if (const int rc = check_size(c, w, bs)) return rc;
    if (m.rows != m.cols)
        return fail(c, HISPMV_EINVAL, w + ": the handle is " + std::to_string(m.rows) + " x " + std::to_string(m.cols) + ", a block-Jacobi preconditioner needs a square matrix");
    if (has_tile_stream(m)) {
        if (m.format == 1 && !m.keep_format) return refuse_tile_stream(c, m, who, "block extraction");
        return fail(c, HISPMV_ENOTSUP, w + ": this handle is a transposed tile stream, which has no block extraction; create it after hispmv_set_transposable(ctx, 1) "
                                           "(FpgaHandle.set_transposable(True)) so that it keeps the slice stream");
    }
    if (const int rc = check_buffer(c, w, d_pre, pre_bytes, block_jacobi_layout(m.rows, bs).pre_bytes)) return rc;
    return adopt_stream(c, stream, s);
}

int extract(hispmv_ctx* c, const Matrix& m, int bs, float* blocks, hipStream_t s) {
    if (m.dense) {
        LAUNCH_TRY(c, launch_block_jacobi_dense, m.d_dense, m.value_storage == HISPMV_VALUES_BF16, blocks, m.rows, bs, s);
        return HISPMV_OK;
    }
    LAUNCH_TRY(c, launch_block_jacobi_fill, blocks, m.rows, bs, s);
    for (auto& p : m.parts) LAUNCH_TRY(c, launch_block_jacobi_walk, p.dev, blocks, m.rows, bs, s);
    return HISPMV_OK;
}

}  // namespace

HISPMV_API int hispmv_block_jacobi_info(const hispmv_ctx* c, int idx, int64_t bs, int64_t out[8]) {
    if (!c || !out || idx < 0 || idx >= (int)c->mats.size() || !block_jacobi_size_ok(bs)) return HISPMV_EINVAL;
    for (int i = 0; i < 8; ++i) out[i] = 0;
    const Matrix& m = *c->mats[(size_t)idx];
    if (!m.loaded || m.rows != m.cols || has_tile_stream(m)) return HISPMV_OK;
    const BlockJacobiLayout l = block_jacobi_layout(m.rows, bs);
    out[0] = 1; out[1] = l.n_blocks; out[2] = l.pre_bytes; out[3] = setup_launches(m); out[4] = cg_work_bytes(m.rows);
    out[5] = gmres_layout(m.rows, 1, true).work_bytes; out[6] = gmres_layout(m.rows, 1, true).stride * 4; out[7] = m.rows;
    return HISPMV_OK;
}

HISPMV_API int hispmv_block_jacobi_extract_device(hispmv_ctx* c, int idx, int64_t bs, void* d_pre, int64_t pre_bytes, void* stream) {
    if (!c) return HISPMV_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    Matrix* m = nullptr;
    hipStream_t s;
    if (const int rc = extract_target(c, "block_jacobi_extract_device", idx, bs, d_pre, pre_bytes, &m, &s, stream)) return rc;
    return extract(c, *m, (int)bs, (float*)d_pre, s);
}

HISPMV_API int hispmv_block_invert_device(hispmv_ctx* c, void* d_pre, int64_t n_blocks, int64_t bs, void* stream) {
    if (!c) return HISPMV_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    const std::string w("block_invert_device");
    if (const int rc = check_size(c, w, bs)) return rc;
    if (n_blocks < 0 || n_blocks > (1LL << 31) / bs) return fail(c, HISPMV_EINVAL, w + ": n_blocks must not be negative (and n_blocks * block_size at most 2^31)");
    const BlockJacobiLayout l = block_jacobi_layout(n_blocks * bs, bs);
    if (const int rc = check_buffer(c, w, d_pre, l.pre_bytes, l.pre_bytes)) return rc;
    hipStream_t s;
    if (const int rc = adopt_stream(c, stream, &s)) return rc;
    LAUNCH_TRY(c, launch_block_invert, (float*)d_pre, (int32_t*)((char*)d_pre + l.off_flags), n_blocks, (int)bs, s);
    return HISPMV_OK;
}

HISPMV_API int hispmv_block_jacobi_setup_device(hispmv_ctx* c, int idx, int64_t bs, void* d_pre, int64_t pre_bytes, void* stream) {
    if (!c) return HISPMV_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    Matrix* m = nullptr;
    hipStream_t s;
    if (const int rc = extract_target(c, "block_jacobi_setup_device", idx, bs, d_pre, pre_bytes, &m, &s, stream)) return rc;
    if (const int rc = extract(c, *m, (int)bs, (float*)d_pre, s)) return rc;
    const BlockJacobiLayout l = block_jacobi_layout(m->rows, bs);
    LAUNCH_TRY(c, launch_block_invert, (float*)d_pre, (int32_t*)((char*)d_pre + l.off_flags), l.n_blocks, (int)bs, s);
    return HISPMV_OK;
}

HISPMV_API int hispmv_block_jacobi_status(hispmv_ctx* c, const void* d_pre, int64_t n, int64_t bs, void* stream, int64_t* out) {
    if (!c || !out) return HISPMV_EINVAL;
    hipStream_t s;
    BlockJacobiLayout l;
    {
        std::lock_guard<std::mutex> g(c->mu);
        const std::string w("block_jacobi_status");
        if (const int rc = check_size(c, w, bs)) return rc;
        if (n < 0 || n > 0x7fffffffLL) return fail(c, HISPMV_EINVAL, w + ": n must not be negative");
        l = block_jacobi_layout(n, bs);
        if (const int rc = check_buffer(c, w, d_pre, l.pre_bytes, l.pre_bytes)) return rc;
        if (const int rc = adopt_stream(c, stream, &s)) return rc;
    }
    std::vector<int32_t> flags((size_t)l.n_blocks);
    HIP_TRY(c, hipStreamSynchronize(s));
    if (l.n_blocks > 0) HIP_TRY(c, hipMemcpy(flags.data(), (const char*)d_pre + l.off_flags, (size_t)l.n_blocks * 4, hipMemcpyDeviceToHost));
    int64_t bad = 0;
    for (const int32_t f : flags) bad += f != 0 ? 1 : 0;
    *out = bad;
    return HISPMV_OK;
}

HISPMV_API int hispmv_block_jacobi_apply_device(hispmv_ctx* c, const void* d_pre, int64_t n, int64_t bs, const float* d_r, float* d_z, void* stream) {
    if (!c) return HISPMV_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    const std::string w("block_jacobi_apply_device");
    if (const int rc = check_size(c, w, bs)) return rc;
    if (n < 0 || n > 0x7fffffffLL) return fail(c, HISPMV_EINVAL, w + ": n must not be negative");
    const int64_t need = block_jacobi_layout(n, bs).pre_bytes;
    if (const int rc = check_buffer(c, w, d_pre, need, need)) return rc;
    if (const int rc = krylov_check_operands(c, w, n > 0 && (!d_r || !d_z), d_r, d_z)) return rc;
    hipStream_t s;
    if (const int rc = adopt_stream(c, stream, &s)) return rc;
    LAUNCH_TRY(c, launch_block_jacobi_apply, (const float*)d_pre, n, (int)bs, d_r, d_z, s);
    return HISPMV_OK;
}
