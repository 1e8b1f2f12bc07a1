// hispmv_spmm_abi.cpp -- the wide-batch entries of the C ABI (include/hispmv.h: hispmv_spmm_device, hispmv_spmm_device_t,
// hispmv_spmm_info, hispmv_prep_spmm_tiles, hispmv_spmm_value_grad_device, hispmv_spmm_value_grad_info, and the bf16-activation forms
// hispmv_spmm_device_bf16, hispmv_spmm_device_t_bf16, hispmv_spmm_bf16_info, hispmv_prep_spmm_bf16_tiles,
// hispmv_spmm_value_grad_device_bf16, hispmv_spmm_value_grad_bf16_info) over the launchers of
// hispmv_spmm.h and hispmv_spmm_grad.h.  A translation unit of its own: the entries read a loaded handle's device tables and keep
// nothing in it, so the other entry points are not touched.
#include "hispmv_ctx.h"
#include "hispmv_spmm.h"
#include "hispmv_spmm_grad.h"

using namespace hispmv;

namespace {

bool spmm_accepts(const Matrix& m) {
    if (m.dense || m.format != 0 || m.parts.empty()) return false;
    for (auto& p : m.parts)
        if (p.is_tts) return false;
    return true;
}
const Matrix* spmm_companion(const Matrix& m) { return (m.companion && spmm_accepts(*m.companion)) ? m.companion.get() : nullptr; }

int refuse_tile_stream(hispmv_ctx* c, const char* who) {
    return fail(c, HISPMV_ENOTSUP, std::string(who) + ": this handle is a transposed tile stream, which has no wide-batch kernel; create it after "
                                       "hispmv_set_transposable(ctx, 1) (FpgaHandle.set_transposable(True)) so that it keeps the slice stream");
}
// *out = the matrix a wide-batch product of handle `idx` runs over: the handle itself, transposed its stored transpose -- a slice stream either way
int spmm_target(hispmv_ctx* c, int idx, const char* who, bool transposed, const Matrix** out) {
    Matrix* m = nullptr;
    if (const int rc = find_handle(c, idx, who, &m)) return rc;
    if (!transposed) {
        if (m->dense)
            return fail(c, HISPMV_ENOTSUP, std::string(who) + ": this is a dense handle; a wide batch against a dense W is a GEMM, which this library leaves to a GEMM library");
        if (!spmm_accepts(*m)) return refuse_tile_stream(c, who);
        *out = m;
        return HISPMV_OK;
    }
    *out = spmm_companion(*m);
    if (!*out)
        return fail(c, HISPMV_ENOTSUP, std::string(who) + ": the transposed wide batch runs over a stored transpose that is a slice stream, and this handle " +
                                           (m->companion ? "stores its transpose as a tile stream" : "has none") +
                                           "; create it after hispmv_set_transposable(ctx, 3) (FpgaHandle.set_transposable(\"companion\"))");
    if (!(*out)->loaded) return fail(c, HISPMV_ESTATE, "internal: the stored transpose is not loaded");
    return HISPMV_OK;
}

// What the fp32 entries and the ones with bf16 activations (`bf16`) differ in outside their launch loops: the tile rule, the workspace,
// two message texts and the alignment the operands need.
SpmmTiles tiles_of(bool bf16, int64_t cols, int64_t num_vecs, int64_t ld_x, int64_t ld_y, int64_t align_bytes) {
    return bf16 ? spmm_bf16_tiles(cols, num_vecs, ld_x, ld_y, align_bytes) : spmm_tiles(cols, num_vecs, ld_x, ld_y, align_bytes);
}
// bytes of the workspace for tiles of 64 * vl vectors: the fp32 partials of the largest part (the parts run one after the other and
// reuse them; spmm_bf16_work_bytes is spmm_work_bytes), then -- bf16, more than one part -- the fp32 tile accumulator the parts add into
int64_t partials_of(const Matrix& t, int vl) {
    int64_t n = 0;
    for (auto& p : t.parts) n = std::max(n, spmm_work_bytes(p.dev, vl));
    return n;
}
int64_t work_bytes_of(bool bf16, const Matrix& t, int vl) { return partials_of(t, vl) + (bf16 && t.parts.size() > 1 ? spmm_bf16_acc_bytes(t.rows, vl) : 0); }
int64_t launches_of(const Matrix& t, int64_t tiles) {
    int64_t n = 0;
    for (auto& p : t.parts) n += spmm_part_launches(p.dev);
    return n * tiles;
}

// widest aligned access at p: 16, 8, 4 or -- 2-byte operands -- 2 bytes
int64_t pointer_align(const void* p) {
    const uintptr_t u = (uintptr_t)p;
    return (u & 15) == 0 ? 16 : (u & 7) == 0 ? 8 : (u & 3) == 0 ? 4 : 2;
}

// The argument checks of a product over `t`, in the order a caller sees them refused.
int check_spmm(hispmv_ctx* c, const Matrix& t, bool bf16, const char* who, const void* d_xt, int64_t num_vecs, int64_t ld_x, const void* d_bias,
               int64_t bias_stride, const void* d_yt, int64_t ld_y, float beta, const void* d_work, int64_t work_bytes) {
    const std::string w(who);
    if (num_vecs < 1) return fail(c, HISPMV_EINVAL, w + ": num_vecs must be at least 1");
    if (num_vecs > 0x7fffffffLL) return fail(c, HISPMV_EINVAL, w + ": num_vecs must stay below 2^31");
    if (ld_x < num_vecs || ld_y < num_vecs) return fail(c, HISPMV_EINVAL, w + ": ld_x and ld_y must be at least num_vecs");
    if (!d_xt || !d_yt || (beta != 0.0f && !d_bias)) return fail(c, HISPMV_EINVAL, "NULL device vector");
    if (d_xt == d_yt) return fail(c, HISPMV_EINVAL, w + ": xt and yt must not be the same matrix");
    if (bias_stride != 0 && bias_stride != ld_y) return fail(c, HISPMV_EINVAL, w + ": bias_stride must be 0 (one " + (bf16 ? "fp32 " : "") + "bias[row] for all vectors) or ld_y");
    if (beta != 0.0f && d_bias == d_yt && bias_stride == 0) return fail(c, HISPMV_EINVAL, w + ": d_bias == d_yt needs bias_stride = ld_y");
    if (!bf16) {
        if (((uintptr_t)d_xt | (uintptr_t)d_yt | (uintptr_t)d_bias | (uintptr_t)d_work) & 3) return fail(c, HISPMV_EINVAL, w + ": device pointers must be 4-byte aligned");
    } else {          // xt, yt and a bias laid out like yt hold halves; the workspace and a shared bias hold floats
        if (((uintptr_t)d_xt | (uintptr_t)d_yt | (bias_stride != 0 ? (uintptr_t)d_bias : 0)) & 1)
            return fail(c, HISPMV_EINVAL, w + ": bf16 device pointers must be 2-byte aligned");
        if (((uintptr_t)d_work | (bias_stride == 0 ? (uintptr_t)d_bias : 0)) & 3)
            return fail(c, HISPMV_EINVAL, w + ": the workspace and a shared fp32 bias must be 4-byte aligned");
    }
    // what the info entry reports for these leading dimensions (16-byte aligned pointers: the widest lanes, the largest workspace)
    const int64_t need = work_bytes_of(bf16, t, tiles_of(bf16, t.cols, num_vecs, ld_x, ld_y, 16).vl_first);
    if (work_bytes < need || (need > 0 && !d_work))
        return fail(c, HISPMV_EINVAL, w + ": the workspace holds " + std::to_string(work_bytes) + " bytes, " + (bf16 ? "hispmv_spmm_bf16_info" : "hispmv_spmm_info") + " asks for " + std::to_string(need));
    return HISPMV_OK;
}

// The launches of one call over `t` (the handle, or its stored transpose): vector tiles one after the other, inside a tile the parts
// one after the other -- part 0 with the caller's beta * bias, each later part adding into yt in place.
int run_spmm(hispmv_ctx* c, const Matrix& t, const char* who, const float* d_xt, int64_t num_vecs, int64_t ld_x, const float* d_bias,
             int64_t bias_stride, float* d_yt, int64_t ld_y, float alpha, float beta, void* d_work, int64_t work_bytes, void* stream) {
    if (const int rc = check_spmm(c, t, false, who, d_xt, num_vecs, ld_x, d_bias, bias_stride, d_yt, ld_y, beta, d_work, work_bytes)) return rc;
    hipStream_t s;
    if (const int rc = adopt_stream(c, stream, &s)) return rc;
    SpmmOperands a{};
    a.xt = d_xt; a.yt = d_yt; a.work = (float*)d_work; a.ld_x = ld_x; a.ld_y = ld_y; a.n_vecs = (int)num_vecs;
    if (alpha == 0.0f) {          // yt is exactly beta * bias; neither xt nor the matrix is read
        a.bias = d_bias; a.bias_stride = bias_stride; a.alpha = 0.0f; a.beta = beta;
        LAUNCH_TRY(c, launch_spmm_bias, a, t.rows, s);
        return HISPMV_OK;
    }
    // a lane's VL floats must be one aligned access in every row of xt, yt and a bias laid out like yt
    int64_t align = std::min({pointer_align(d_xt), pointer_align(d_yt), pointer_align(d_work)});
    if (beta != 0.0f && bias_stride != 0) align = std::min(align, pointer_align(d_bias));
    for (int64_t k = 0; k < num_vecs;) {
        const int vl = spmm_vl(t.cols, num_vecs - k, ld_x, ld_y, align);
        a.tile0 = (int)k;
        for (size_t q = 0; q < t.parts.size(); ++q) {
            const SpmvDeviceMatrix& d = t.parts[q].dev;
            if (q == 0) { a.bias = d_bias; a.bias_stride = bias_stride; a.alpha = alpha; a.beta = beta; }
            else { a.bias = d_yt; a.bias_stride = ld_y; a.alpha = alpha; a.beta = 1.0f; }
            if (d.n_slices <= 0) continue;          // (only a matrix without rows has no slice: every row owns a slot)
            LAUNCH_TRY(c, launch_spmm_part, d, vl, a, s);
        }
        k += std::min<int64_t>(num_vecs - k, 64 * vl);
    }
    return HISPMV_OK;
}

// run_spmm for 2-byte operands (the same kernels over uint16_t): the same tiles-then-parts order of launches.  More than one part:
// every part but the last stores fp32 into the tile accumulator (part 0 with the caller's beta * bias, a later one adding in place),
// the last reads it as its bias and is the only one that rounds and stores to yt.
int run_spmm_bf16(hispmv_ctx* c, const Matrix& t, const char* who, const uint16_t* d_xt, int64_t num_vecs, int64_t ld_x, const void* d_bias,
                  int64_t bias_stride, uint16_t* d_yt, int64_t ld_y, float alpha, float beta, void* d_work, int64_t work_bytes, void* stream) {
    if (const int rc = check_spmm(c, t, true, who, d_xt, num_vecs, ld_x, d_bias, bias_stride, d_yt, ld_y, beta, d_work, work_bytes)) return rc;
    hipStream_t s;
    if (const int rc = adopt_stream(c, stream, &s)) return rc;
    SpmmBf16Operands a{};
    a.xt = d_xt; a.yt = d_yt; a.work = (float*)d_work; a.ld_x = ld_x; a.ld_y = ld_y; a.n_vecs = (int)num_vecs;
    const int caller_bias = bias_stride == 0 ? kBf16BiasShared : kBf16BiasMatrix;
    if (alpha == 0.0f) {          // yt is exactly bf16(beta * bias); neither xt nor the matrix is read
        a.bias = d_bias; a.bias_kind = caller_bias; a.alpha = 0.0f; a.beta = beta;
        LAUNCH_TRY(c, launch_spmm_bf16_bias, a, t.rows, s);
        return HISPMV_OK;
    }
    // a lane's VB halves must be one aligned access in every row of xt, yt and a bias laid out like yt; its fp32 partials go in two
    // accesses of VB / 2 floats, which the same alignment of the workspace covers
    int64_t align = std::min({pointer_align(d_xt), pointer_align(d_yt), pointer_align(d_work)});
    if (beta != 0.0f && bias_stride != 0) align = std::min(align, pointer_align(d_bias));
    size_t first = t.parts.size(), last = 0;          // the parts that hold slices (only a matrix without rows has a part without)
    for (size_t q = 0; q < t.parts.size(); ++q)
        if (t.parts[q].dev.n_slices > 0) { first = std::min(first, q); last = q; }
    for (int64_t k = 0; k < num_vecs;) {
        const int vb = spmm_bf16_vb(t.cols, num_vecs - k, ld_x, ld_y, align);
        a.tile0 = (int)k;
        a.acc = t.parts.size() > 1 ? (float*)((char*)d_work + partials_of(t, vb)) : nullptr;
        for (size_t q = first; q <= last && q < t.parts.size(); ++q) {
            const SpmvDeviceMatrix& d = t.parts[q].dev;
            if (d.n_slices <= 0) continue;
            if (q == first) { a.bias = d_bias; a.bias_kind = caller_bias; a.alpha = alpha; a.beta = beta; }
            else { a.bias = nullptr; a.bias_kind = kBf16BiasAcc; a.alpha = alpha; a.beta = 1.0f; }
            a.to_acc = q == last ? 0 : 1;
            LAUNCH_TRY(c, launch_spmm_bf16_part, d, vb, a, s);
        }
        k += std::min<int64_t>(num_vecs - k, 64 * vb);
    }
    return HISPMV_OK;
}

int prep_tiles(bool bf16, int64_t cols, int64_t num_vecs, int64_t ld, int64_t align_bytes, int64_t out[4]) {
    if (!out || cols < 1 || num_vecs < 1 || ld < 1 || align_bytes < 1) return HISPMV_EINVAL;
    if (ld < num_vecs) return HISPMV_EINVAL;
    const SpmmTiles t = tiles_of(bf16, cols, num_vecs, ld, ld, align_bytes);
    out[0] = t.vl_first; out[1] = t.tiles; out[2] = t.last_vecs; out[3] = t.vl_last;
    return HISPMV_OK;
}

int spmm_info(bool bf16, const hispmv_ctx* c, int idx, int64_t num_vecs, int64_t ld, int64_t out[8]) {
    if (!c || !out || idx < 0 || idx >= (int)c->mats.size() || num_vecs < 1 || ld < num_vecs) return HISPMV_EINVAL;
    for (int i = 0; i < 8; ++i) out[i] = 0;
    const Matrix& m = *c->mats[(size_t)idx];
    if (!m.loaded) return HISPMV_OK;
    const bool fwd = spmm_accepts(m);
    const Matrix* t = spmm_companion(m);
    out[0] = fwd ? 1 : 0; out[1] = t ? 1 : 0;
    if (fwd) {
        const SpmmTiles tl = tiles_of(bf16, m.cols, num_vecs, ld, ld, 16);
        out[2] = tl.vl_first; out[3] = tl.tiles; out[4] = launches_of(m, tl.tiles); out[5] = work_bytes_of(bf16, m, tl.vl_first);
    }
    if (t) out[6] = work_bytes_of(bf16, *t, tiles_of(bf16, t->cols, num_vecs, ld, ld, 16).vl_first);
    return HISPMV_OK;
}

}  // namespace

HISPMV_API int hispmv_prep_spmm_tiles(int64_t cols, int64_t num_vecs, int64_t ld, int64_t align_bytes, int64_t out[4]) {
    return prep_tiles(false, cols, num_vecs, ld, align_bytes, out);
}
HISPMV_API int hispmv_prep_spmm_bf16_tiles(int64_t cols, int64_t num_vecs, int64_t ld, int64_t align_bytes, int64_t out[4]) {
    return prep_tiles(true, cols, num_vecs, ld, align_bytes, out);
}
HISPMV_API int hispmv_spmm_info(const hispmv_ctx* c, int idx, int64_t num_vecs, int64_t ld, int64_t out[8]) { return spmm_info(false, c, idx, num_vecs, ld, out); }
HISPMV_API int hispmv_spmm_bf16_info(const hispmv_ctx* c, int idx, int64_t num_vecs, int64_t ld, int64_t out[8]) { return spmm_info(true, c, idx, num_vecs, ld, out); }

HISPMV_API int hispmv_spmm_device(hispmv_ctx* c, int idx, const float* d_xt, int64_t num_vecs, int64_t ld_x, const float* d_bias, int64_t bias_stride,
                                  float* d_yt, int64_t ld_y, float alpha, float beta, void* d_work, int64_t work_bytes, void* stream) {
    if (!c) return HISPMV_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    const Matrix* t = nullptr;
    if (const int rc = spmm_target(c, idx, "spmm_device", false, &t)) return rc;
    return run_spmm(c, *t, "spmm_device", d_xt, num_vecs, ld_x, d_bias, bias_stride, d_yt, ld_y, alpha, beta, d_work, work_bytes, stream);
}

HISPMV_API int hispmv_spmm_device_t(hispmv_ctx* c, int idx, const float* d_xt, int64_t num_vecs, int64_t ld_x, const float* d_bias, int64_t bias_stride,
                                    float* d_yt, int64_t ld_y, float alpha, float beta, void* d_work, int64_t work_bytes, void* stream) {
    if (!c) return HISPMV_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    const Matrix* t = nullptr;
    if (const int rc = spmm_target(c, idx, "spmm_device_t", true, &t)) return rc;
    return run_spmm(c, *t, "spmm_device_t", d_xt, num_vecs, ld_x, d_bias, bias_stride, d_yt, ld_y, alpha, beta, d_work, work_bytes, stream);
}

HISPMV_API int hispmv_spmm_device_bf16(hispmv_ctx* c, int idx, const uint16_t* d_xt, int64_t num_vecs, int64_t ld_x, const void* d_bias, int64_t bias_stride,
                                       uint16_t* d_yt, int64_t ld_y, float alpha, float beta, void* d_work, int64_t work_bytes, void* stream) {
    if (!c) return HISPMV_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    const Matrix* t = nullptr;
    if (const int rc = spmm_target(c, idx, "spmm_device_bf16", false, &t)) return rc;
    return run_spmm_bf16(c, *t, "spmm_device_bf16", d_xt, num_vecs, ld_x, d_bias, bias_stride, d_yt, ld_y, alpha, beta, d_work, work_bytes, stream);
}

HISPMV_API int hispmv_spmm_device_t_bf16(hispmv_ctx* c, int idx, const uint16_t* d_xt, int64_t num_vecs, int64_t ld_x, const void* d_bias, int64_t bias_stride,
                                         uint16_t* d_yt, int64_t ld_y, float alpha, float beta, void* d_work, int64_t work_bytes, void* stream) {
    if (!c) return HISPMV_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    const Matrix* t = nullptr;
    if (const int rc = spmm_target(c, idx, "spmm_device_t_bf16", true, &t)) return rc;
    return run_spmm_bf16(c, *t, "spmm_device_t_bf16", d_xt, num_vecs, ld_x, d_bias, bias_stride, d_yt, ld_y, alpha, beta, d_work, work_bytes, stream);
}

// ---- wide-batch value gradient (include/hispmv.h: hispmv_spmm_value_grad_device, hispmv_spmm_value_grad_device_bf16; kernels:
// hispmv_spmm_grad.hip) ---------------------------------------------------------------------------------------------------------------
namespace {

// launches of one vector tile: one per part that holds slices (none for a handle without entries)
int64_t grad_launches_of(const Matrix& m) {
    if (m.upd_n <= 0) return 0;
    int64_t n = 0;
    for (auto& p : m.parts) n += (p.dev.n_slices > 0 && p.dev.n_groups > 0) ? 1 : 0;
    return n;
}

// bf16 operands take the product's bf16 rule as it stands (spmm_bf16_tiles); its 8 MiB of rule (b) was measured for neither bf16 kernel
int value_grad_info(bool bf16, const hispmv_ctx* c, int idx, int64_t num_vecs, int64_t ld, int64_t out[4]) {
    if (!c || !out || idx < 0 || idx >= (int)c->mats.size() || num_vecs < 1 || ld < num_vecs) return HISPMV_EINVAL;
    for (int i = 0; i < 4; ++i) out[i] = 0;
    const Matrix& m = *c->mats[(size_t)idx];
    if (!m.loaded || !m.updatable || !spmm_accepts(m)) return HISPMV_OK;
    const SpmmTiles tl = tiles_of(bf16, m.cols, num_vecs, ld, ld, 16);
    out[0] = 1; out[1] = tl.vl_first; out[2] = tl.tiles; out[3] = grad_launches_of(m) * tl.tiles;
    return HISPMV_OK;
}

// One call of either entry; Half = uint16_t for bf16 operands, float otherwise.  Checks, order and return codes are the same; the
// operands' alignment, the tile rule and the launcher differ.
template <class Half>
int run_value_grad(hispmv_ctx* c, int idx, const char* who, const Half* d_gyt, int64_t ld_gy, const Half* d_xt, int64_t ld_x, int64_t num_vecs, float* d_grad,
                   float alpha, float beta, void* stream) {
    constexpr bool bf16 = sizeof(Half) == 2;
    if (!c) return HISPMV_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    Matrix* mp = nullptr;
    if (const int rc = find_handle(c, idx, who, &mp)) return rc;
    Matrix& m = *mp;
    const std::string w(who);
    if (m.dense)
        return fail(c, HISPMV_ENOTSUP, w + ": this is a dense handle; the value gradient of a dense W over a wide batch is a GEMM (gyt * xt^T), "
                                           "which this library leaves to a GEMM library");
    if (!spmm_accepts(m)) return refuse_tile_stream(c, who);
    if (!m.updatable) return fail(c, HISPMV_ESTATE, w + ": handle was not created with value updates on (hispmv_set_value_updates)");
    if (num_vecs < 1) return fail(c, HISPMV_EINVAL, w + ": num_vecs must be at least 1");
    if (num_vecs > 0x7fffffffLL) return fail(c, HISPMV_EINVAL, w + ": num_vecs must stay below 2^31");
    if (ld_gy < num_vecs || ld_x < num_vecs) return fail(c, HISPMV_EINVAL, w + ": ld_gy and ld_x must be at least num_vecs");
    if (!d_gyt || !d_xt || (m.upd_n > 0 && !d_grad)) return fail(c, HISPMV_EINVAL, "NULL device vector");
    if (d_grad && ((const void*)d_grad == (const void*)d_gyt || (const void*)d_grad == (const void*)d_xt)) return fail(c, HISPMV_EINVAL, w + ": grad must not be gyt or xt");
    if constexpr (!bf16) {
        if (((uintptr_t)d_gyt | (uintptr_t)d_xt | (uintptr_t)d_grad) & 3) return fail(c, HISPMV_EINVAL, w + ": device pointers must be 4-byte aligned");
    } else {
        if (((uintptr_t)d_gyt | (uintptr_t)d_xt) & 1) return fail(c, HISPMV_EINVAL, w + ": bf16 device pointers must be 2-byte aligned");
        if ((uintptr_t)d_grad & 3) return fail(c, HISPMV_EINVAL, w + ": grad must be 4-byte aligned");
    }
    if (m.upd_n == 0) return HISPMV_OK;
    hipStream_t s;
    if (const int rc = adopt_stream(c, stream, &s)) return rc;
    if (alpha == 0.0f) return scale_in_place(c, d_grad, m.upd_n, beta, s);          // grad = beta * grad exactly, gyt and xt not read
    // Vector tiles one after the other -- the first with the caller's beta, every later one adding in place -- and inside a tile the
    // parts one after the other, each with its own chunks of the value map: every input entry lives in exactly one slot over all
    // parts, so a part writes only its own entries.  A lane's VL floats (VB halves) must be one aligned load in every row of gyt and xt.
    const int64_t align = std::min(pointer_align(d_gyt), pointer_align(d_xt));
    std::conditional_t<bf16, SpmmGradBf16Operands, SpmmGradOperands> a{};
    a.gyt = d_gyt; a.xt = d_xt; a.grad = d_grad; a.ld_gy = ld_gy; a.ld_x = ld_x; a.n = m.upd_n; a.n_vecs = (int)num_vecs; a.alpha = alpha;
    for (int64_t k = 0; k < num_vecs;) {
        const int vl = bf16 ? spmm_bf16_vb(m.cols, num_vecs - k, ld_x, ld_gy, align) : spmm_vl(m.cols, num_vecs - k, ld_x, ld_gy, align);
        a.tile0 = (int)k; a.beta = k == 0 ? beta : 1.0f;
        for (auto& p : m.parts) {
            if (p.dev.n_slices <= 0) continue;
            if constexpr (bf16) { LAUNCH_TRY(c, launch_spmm_grad_bf16_part, p.dev, vl, m.d_map + p.map_chunk_base * kValueChunk, a, s); }
            else { LAUNCH_TRY(c, launch_spmm_grad_part, p.dev, vl, m.d_map + p.map_chunk_base * kValueChunk, a, s); }
        }
        k += std::min<int64_t>(num_vecs - k, 64 * vl);
    }
    return HISPMV_OK;
}

}  // namespace

HISPMV_API int hispmv_spmm_value_grad_info(const hispmv_ctx* c, int idx, int64_t num_vecs, int64_t ld, int64_t out[4]) {
    return value_grad_info(false, c, idx, num_vecs, ld, out);
}
HISPMV_API int hispmv_spmm_value_grad_bf16_info(const hispmv_ctx* c, int idx, int64_t num_vecs, int64_t ld, int64_t out[4]) {
    return value_grad_info(true, c, idx, num_vecs, ld, out);
}

HISPMV_API int hispmv_spmm_value_grad_device(hispmv_ctx* c, int idx, const float* d_gyt, int64_t ld_gy, const float* d_xt, int64_t ld_x, int64_t num_vecs,
                                             float* d_grad, float alpha, float beta, void* stream) {
    return run_value_grad<float>(c, idx, "spmm_value_grad_device", d_gyt, ld_gy, d_xt, ld_x, num_vecs, d_grad, alpha, beta, stream);
}

HISPMV_API int hispmv_spmm_value_grad_device_bf16(hispmv_ctx* c, int idx, const uint16_t* d_gyt, int64_t ld_gy, const uint16_t* d_xt, int64_t ld_x, int64_t num_vecs,
                                                  float* d_grad, float alpha, float beta, void* stream) {
    return run_value_grad<uint16_t>(c, idx, "spmm_value_grad_device_bf16", d_gyt, ld_gy, d_xt, ld_x, num_vecs, d_grad, alpha, beta, stream);
}
