// hispmv_launch.cpp -- the entries of the C ABI (include/hispmv.h) that launch a product, a gradient or an update on a loaded handle:
// the forward pass plan (forward_width, launch_forward) with the host-vector path over it, the transposed and stored-transpose
// entries, the value gradient, the value updates, and the info getters that walk the same pass plan.  Host-side HIP calls only.
#include "hispmv_ctx.h"

using namespace hispmv;

namespace {

int launch_matrix(hispmv_ctx* c, Matrix& m, const float* d_x, const float* d_bias, float* d_y,
                  float alpha, float beta, hipStream_t s, bool fixup_only = false) {
    if (!m.dense && (m.parts.size() > 1 || (m.format == 1 && m.parts[0].tdev.zero_fill)) && m.index >= 0) {
        // (a stored transpose goes the same way under its internal id, hispmv_ctx::matrix: the bits of a handle made from the swapped input)
        // column tiles: all of them in ONE grid (+ one fix-up, one merge launch) through the batch machinery -- launched
        // one after the other each tile had the chip to itself for half the work (mouse_gene 48 -> 40 us)
        const int32_t idx = m.index;
        return spmv_batch_locked(c, 1, &idx, &d_x, &d_bias, &d_y, alpha, beta, s, idx >= kCompanionId);
    }
    if (m.dense) {
        LAUNCH_TRY(c, launch_gemv, m.d_dense, m.rows, m.cols, d_x, d_bias, d_y, alpha, beta, s, m.value_storage == HISPMV_VALUES_BF16);
        return HISPMV_OK;
    }
    if (m.format == 1) {
        LAUNCH_TRY(c, launch_tts, m.parts[0].tdev, d_x, d_bias, d_y, alpha, beta, s);
        return HISPMV_OK;
    }
    for (size_t t = 0; t < m.parts.size(); ++t) {
        // column tile 0 computes alpha*A_0*x + beta*bias into y; tile t > 0 writes alpha*A_t*x into its partial vector
        if (t == 0) LAUNCH_TRY(c, launch_spmv, m.parts[t].dev, d_x, d_bias, d_y, alpha, beta, s, fixup_only);
        else LAUNCH_TRY(c, launch_spmv, m.parts[t].dev, d_x, nullptr, m.d_ypart + (t - 1) * (size_t)kMaxBatch * m.rows, alpha, 0.0f, s, fixup_only);
    }
    if (m.parts.size() > 1) LAUNCH_TRY(c, launch_merge_parts, d_y, m.d_ypart, (int)m.parts.size() - 1, (int64_t)kMaxBatch * m.rows, m.rows, 1, 0, 0, s);
    return HISPMV_OK;
}

// ---- the forward pass plan: one width rule, one launch loop ---------------------------------------------------------------------------
// Vectors of the next forward pass over `m` with `left` vectors to go: what launch_forward launches and hispmv_linear_info reports
// (the transposed side: transposed_width).  Dense 8, 4, 2, 1.  A tile stream of one part without zero_fill: 4 or 2 vectors through
// every pass over the words where the tiles are small enough, else up to kTtsMaxVectors in one launch, one after the other.  A slice
// stream: what every part takes (spmv_batch_width), kMaxBatch at most.  Everything else one vector.  Two things differ by caller:
//   slices_batched  false: a slice stream goes one vector per launch -- hispmv_linear_device with beta == 0 (the batched slice kernel's
//                   tile 0 reads a bias); hispmv_linear has beta = 1, and the stored transpose takes the batched widths for every beta
//   per_vector_bias the batched tile kernel takes one shared bias: such a call goes one vector per launch on a tile stream
int forward_width(const Matrix& m, int64_t left, bool slices_batched, bool per_vector_bias) {
    if (left < 2) return 1;
    if (m.dense) return left >= 8 ? 8 : left >= 4 ? 4 : 2;
    if (m.format == 1) {
        if (m.parts.size() != 1 || m.parts[0].tdev.zero_fill || per_vector_bias) return 1;
        const int nv = tts_batch_width(m.parts[0].tdev, left);
        return nv >= 2 ? nv : (int)std::min<int64_t>(left, kTtsMaxVectors);
    }
    if (!slices_batched) return 1;
    int nv = kMaxBatch;
    for (auto& p : m.parts) nv = std::min(nv, spmv_batch_width(p.dev, left));
    return nv;
}
// ... of the next transposed pass (a handle without a stored transpose): launch loops, hispmv_linear_info, hispmv_value_grad_info
int transposed_width(const Matrix& m, int64_t left) {
    if (m.dense) return gemv_t_width(left);
    if (m.format == 1) return tts_t_width(m.parts[0].tdev, left);      // (an accepted tile stream: one part)
    int nv = kMaxBatch;
    for (auto& p : m.parts) nv = std::min(nv, spmv_t_width(p.dev, left));
    return nv;
}

// y_k = alpha * A * x_k + beta * bias_k for `vecs` vectors (x_k = d_x + k * cols, y_k = d_y + k * rows, bias_k = d_bias + k * bias_stride):
// passes of forward_width vectors, every vector with the bits of a one-vector call.  The reference relaunches its kernel per vector
// (FpgaHandle::linear, fpga_handle.cpp:366-379).  Serves hispmv_run_kernel and hispmv_linear, hispmv_linear_device (bias_stride 0) and,
// over a stored transpose, the transposed entries.  fixup_only: the carry variant of a one-vector slice pass -- `linear` and the device
// entries always take the fix-up one (one vector or many, every vector gets the same bits), hispmv_run_kernel the plan's own.
// unbiased_batched: a slice stream takes its batched widths with beta == 0 too (the stored transpose; forward_width: slices_batched).
int launch_forward(hispmv_ctx* c, Matrix& m, int64_t vecs, const float* d_x, const float* d_bias, int64_t bias_stride, float* d_y,
                   float alpha, float beta, hipStream_t s, bool fixup_only, bool unbiased_batched = false) {
    // A d_x off the 16-byte alignment takes one vector per pass (the same bits): the launches hispmv_spmv_device makes for such a
    // pointer.  Single- and multi-vector kernels alike stage x with 16-byte global loads (stage_fragments, the dense and tile-stream
    // bodies), so this does not align those loads -- the hardware executes them at any 4-byte address --; it keeps an unusual
    // pointer off the batched passes, whose only stated condition is on cols (spmv_batch_width).
    const bool batched = vecs > 1 && ((uintptr_t)d_x & 15) == 0;
    const bool has_bias = beta != 0.0f;
    for (int64_t k = 0; k < vecs;) {
        const int nv = batched ? forward_width(m, vecs - k, has_bias || unbiased_batched, has_bias && bias_stride != 0) : 1;
        const float* xk = d_x + k * m.cols;
        const float* bk = has_bias ? d_bias + k * bias_stride : nullptr;
        float* yk = d_y + k * m.rows;
        if (batched && m.dense) {          // (a last pass of one vector too: the launch of launch_gemv)
            LAUNCH_TRY(c, launch_gemv_batched, m.d_dense, m.rows, m.cols, nv, xk, bk, yk, alpha, beta, s, m.value_storage == HISPMV_VALUES_BF16);
        } else if (nv < 2) {
            const int rc = launch_matrix(c, m, xk, bk, yk, alpha, beta, s, fixup_only);
            if (rc != HISPMV_OK) return rc;
        } else if (m.format == 1) {
            LAUNCH_TRY(c, launch_tts_batched, m.parts[0].tdev, nv, xk, bk, yk, alpha, beta, s);
        } else {
            for (size_t t = 0; t < m.parts.size(); ++t) {
                // tile 0: the bias (shared, or one per vector); tile t > 0: the nv partial vectors of that tile, no bias
                if (t == 0) LAUNCH_TRY(c, launch_spmv_batched, m.parts[t].dev, nv, xk, bk, (int)bias_stride, yk, alpha, beta, s);
                else LAUNCH_TRY(c, launch_spmv_batched, m.parts[t].dev, nv, xk, nullptr, 0, m.d_ypart + (t - 1) * (size_t)kMaxBatch * m.rows, alpha, 0.0f, s);
            }
            if (m.parts.size() > 1) LAUNCH_TRY(c, launch_merge_parts, yk, m.d_ypart, (int)m.parts.size() - 1, (int64_t)kMaxBatch * m.rows, m.rows, nv, m.rows, m.rows, s);
        }
        k += nv;
    }
    return HISPMV_OK;
}

int run_host_vectors(hispmv_ctx* c, Matrix& m, const float* x, int64_t num_vecs, const float* bias,
                     float* y, float alpha, float beta, bool is_linear) {
    HIP_TRY(c, hipSetDevice(c->device));
    int rc;
    // device side: [x (num_vecs * cols) | bias (rows)] in one block, y in another
    const int64_t nx = (((int64_t)m.cols * num_vecs + 63) / 64) * 64, nb = m.rows, ny = (int64_t)m.rows * num_vecs;
    // launch_fetch_vectors moves whole float4s and nb need not be a multiple of 4: the device block ends on a float4, the pinned
    // block has 3 floats of slack behind y.  No pointer a kernel receives depends on either.
    if ((rc = ensure_vec(c, &c->d_x, &c->cap_x, nx + ((nb + 3) & ~(int64_t)3))) != HISPMV_OK) return rc;
    if ((rc = ensure_vec(c, &c->d_y, &c->cap_y, ny)) != HISPMV_OK) return rc;
    float* const d_x = c->d_x;
    float* const d_bias = c->d_x + nx;
    const size_t bx = (size_t)m.cols * num_vecs * sizeof(float), bb = (size_t)nb * sizeof(float), by = (size_t)ny * sizeof(float);
    const bool staged = (nx + nb + ny) * (int64_t)sizeof(float) <= (8 << 20);     // small vectors: through pinned memory
    if (staged) {
        if (nx + nb + ny + 3 > c->cap_stage) {
            host_free(c->h_stage);      // (the staging block only; the batch tables are not touched by this path)
            c->cap_stage = 0;
            const int64_t want = std::max<int64_t>(nx + nb + ny + 3, 1 << 16);
            HIP_TRY(c, hipHostMalloc((void**)&c->h_stage, (size_t)want * sizeof(float), hipHostMallocDefault));
            c->cap_stage = want;
            c->d_stage = nullptr;
            // (HISPMV_HOST_Y=copy: y through a device buffer and a copy back, as until round 4)
            const bool direct_y = !(std::getenv("HISPMV_HOST_Y") && !std::strcmp(std::getenv("HISPMV_HOST_Y"), "copy"));
            if (direct_y && hipHostGetDevicePointer((void**)&c->d_stage, c->h_stage, 0) != hipSuccess) { (void)hipGetLastError(); c->d_stage = nullptr; }
        }
        std::memcpy(c->h_stage, x, bx);
        if (beta != 0.0f) std::memcpy(c->h_stage + nx, bias, bb);
        // (x and bias cross PCIe through a copy KERNEL that reads the pinned block: the DMA path costs ~10 us per call; HISPMV_HOST_Y=copy: as before)
        if (c->d_stage && (nx + nb) * (int64_t)sizeof(float) <= (1 << 20)) {
            LAUNCH_TRY(c, launch_fetch_vectors, c->d_stage, d_x, beta != 0.0f ? nx + nb : (int64_t)m.cols * num_vecs, c->stream);
        } else {
            HIP_TRY(c, hipMemcpyAsync(d_x, c->h_stage, beta != 0.0f ? (size_t)nx * sizeof(float) + bb : bx, hipMemcpyHostToDevice, c->stream));
        }
    } else {
        HIP_TRY(c, hipMemcpyAsync(d_x, x, bx, hipMemcpyHostToDevice, c->stream));
        if (beta != 0.0f) HIP_TRY(c, hipMemcpyAsync(d_bias, bias, bb, hipMemcpyHostToDevice, c->stream));
    }
    // Small vectors: the kernels write y STRAIGHT into the pinned staging block (its device address; coherent host memory), so the
    // call has no copy back -- one DMA round trip (~10 us of a ~50 us call around a 10 - 20 us kernel) less.  The few read-modify-writes
    // of y (rows cut by slice boundaries, the merge of column parts) cross PCIe; they run in the tail launch, one round trip deep.
    float* const h_y = staged ? c->h_stage + nx + nb : y;
    float* const d_y = (staged && c->d_stage) ? c->d_stage + nx + nb : c->d_y;
    HIP_TRY(c, hipEventRecord(c->ev0, c->stream));
    if ((rc = launch_forward(c, m, num_vecs, d_x, d_bias, 0, d_y, alpha, beta, c->stream, is_linear)) != HISPMV_OK) return rc;
    HIP_TRY(c, hipEventRecord(c->ev1, c->stream));
    if (d_y == c->d_y) HIP_TRY(c, hipMemcpyAsync(h_y, c->d_y, by, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (staged) std::memcpy(y, h_y, by);
    if (hipEventElapsedTime(&c->last_ms, c->ev0, c->ev1) != hipSuccess) c->last_ms = -1.0f;
    return check_device_error(c);
}

}  // namespace

HISPMV_API int hispmv_run_kernel(hispmv_ctx* c, const float* x, const float* bias, float* y, float alpha, float beta) {
    if (!c) return HISPMV_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    if (c->selected < 0) return fail(c, HISPMV_ESTATE, "Run Kernel called before selecting a matrix");   // assert :292
    Matrix& m = *c->mats[c->selected];
    if (!m.loaded) return fail(c, HISPMV_ESTATE, "run_kernel called before load_matrices");
    if (!x || !y || (beta != 0.0f && !bias)) return fail(c, HISPMV_EINVAL, "NULL vector");
    return run_host_vectors(c, m, x, 1, bias, y, alpha, beta, false);
}

HISPMV_API int hispmv_linear(hispmv_ctx* c, int idx, const float* x, int64_t x_len, const float* bias, float* y_out) {
    if (!c) return HISPMV_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    Matrix* mp = nullptr;
    if (const int rc = find_handle(c, idx, "linear", &mp)) return rc;
    Matrix& m = *mp;
    if (!x || !bias || !y_out) return fail(c, HISPMV_EINVAL, "NULL vector");
    const int64_t num_vecs = x_len / m.cols;   // fpga_handle.cpp:336
    if (num_vecs <= 0) return fail(c, HISPMV_EINVAL, "x shorter than one input vector");
    return run_host_vectors(c, m, x, num_vecs, bias, y_out, 1.0f, 1.0f, true);   // alpha = beta = 1, :351-352
}

HISPMV_API int hispmv_spmv_device(hispmv_ctx* c, int idx, const float* d_x, const float* d_bias, float* d_y,
                                  float alpha, float beta, void* stream) {
    if (!c) return HISPMV_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    Matrix* m = nullptr;
    if (const int rc = find_handle(c, idx, "spmv_device", &m)) return rc;
    if (!d_x || !d_y || (beta != 0.0f && !d_bias)) return fail(c, HISPMV_EINVAL, "NULL device vector");
    hipStream_t s;
    if (const int rc = adopt_stream(c, stream, &s)) return rc;
    return launch_matrix(c, *m, d_x, d_bias, d_y, alpha, beta, s);
}

HISPMV_API float hispmv_time_device(hispmv_ctx* c, int idx, const float* d_x, const float* d_bias, float* d_y,
                                    float alpha, float beta, int reps) {
    if (!c || reps <= 0) return -1.0f;
    std::lock_guard<std::mutex> g(c->mu);
    if (idx < 0 || idx >= (int)c->mats.size() || !c->mats[idx]->loaded) { c->err = "bad matrix for time_device"; return -1.0f; }
    Matrix& m = *c->mats[idx];
    if (hipSetDevice(c->device) != hipSuccess) return -1.0f;
    if (hipEventRecord(c->ev0, c->stream) != hipSuccess) return -1.0f;
    for (int i = 0; i < reps; ++i)
        if (launch_matrix(c, m, d_x, d_bias, d_y, alpha, beta, c->stream) != HISPMV_OK) return -1.0f;
    if (hipEventRecord(c->ev1, c->stream) != hipSuccess) return -1.0f;
    if (hipStreamSynchronize(c->stream) != hipSuccess) return -1.0f;
    float ms = -1.0f;
    if (hipEventElapsedTime(&ms, c->ev0, c->ev1) != hipSuccess) return -1.0f;
    return ms / reps;
}

// ---- transposed product (include/hispmv.h: hispmv_spmv_device_t; kernels: hispmv_transpose.hip) ---------------------------------
// what the transposed and gradient entries accept and refuse: transposable_handle, refuse_tile_stream (hispmv_abi.cpp)
namespace {
// ---- the stored transpose (include/hispmv.h: HISPMV_TRANSPOSABLE_COMPANION) ------------------------------------------------------------
// The transposed entries of a handle that owns one run the FORWARD launches of `t` = *owner.companion (t.rows = owner.cols): no atomic,
// per vector the bits of a one-vector hispmv_linear_device call on a handle made from the swapped input.  Widths and launch loop
// are the forward ones (forward_width, launch_forward) with the batched slice widths for every beta.
// Launches of one pass of nv vectors (alpha != 0).  A one-vector pass over a cut matrix is a batch call of one matrix (launch_matrix):
// one grid per workgroup size (and stray class) among its parts, then its tail -- one launch where the merge applies the fix-ups itself.
int64_t companion_pass_launches(const Matrix& t, int nv) {
    auto chains = [](const SpmvDeviceMatrix& d) { return (d.n_fix_short > 0 ? 1 : 0) + (d.n_fix_long > 0 ? 1 : 0); };
    if (t.format == 1 && t.parts.size() == 1 && !t.parts[0].tdev.zero_fill) {
        const TtsDeviceMatrix& d = t.parts[0].tdev;
        return d.n_tiles > 0 ? 1 + (d.n_fix > 0 ? 1 : 0) : 0;
    }
    if (t.parts.size() == 1) return (t.parts[0].dev.n_slices > 0 ? 1 : 0) + chains(t.parts[0].dev);
    int64_t n = 0;
    if (nv > 1) {
        for (auto& p : t.parts) n += (p.dev.n_slices > 0 ? 1 : 0) + chains(p.dev);
        return n + 1;       // + the merge
    }
    std::vector<int> classes;
    for (auto& p : t.parts) {
        const int cls = p.is_tts ? -1 : p.dev.block_threads * 2 + (p.dev.has_strays ? 1 : 0);
        if (std::find(classes.begin(), classes.end(), cls) == classes.end()) classes.push_back(cls);
        if (!p.is_tts && p.dev.n_fix_long > 0) n += 1;
    }
    return n + (int64_t)classes.size() + (t.d_fix_of_row ? 1 : 2);
}

int launch_companion(hispmv_ctx* c, Matrix& owner, int64_t vecs, const float* d_x, const float* d_bias, int64_t bias_stride, float* d_y,
                     float alpha, float beta, hipStream_t s) {
    Matrix& t = *owner.companion;
    if (!t.loaded) return fail(c, HISPMV_ESTATE, "internal: the stored transpose is not loaded");
    if (alpha == 0.0f) {          // y is exactly beta * bias, per vector; neither x nor the matrix is read (hispmv_linear_device runs its kernels)
        LAUNCH_TRY(c, launch_transpose_prologue, d_bias, d_y, t.rows, beta, s, vecs, bias_stride);
        return HISPMV_OK;
    }
    return launch_forward(c, t, vecs, d_x, d_bias, bias_stride, d_y, alpha, beta, s, true, true);
}

// y_k = alpha * A^T * x_k + beta * bias_k behind the checks of hispmv_spmv_device_t (one vector) and hispmv_linear_device_t
int launch_transposed(hispmv_ctx* c, Matrix& m, int64_t vecs, const float* d_x, const float* d_bias, int64_t bias_stride, float* d_y,
                      float alpha, float beta, hipStream_t s) {
    if (m.companion) return launch_companion(c, m, vecs, d_x, d_bias, bias_stride, d_y, alpha, beta, s);
    // ONE prologue y = beta * bias for all vectors, then every part of the matrix adds alpha * A_t^T * x into it -- no partial vectors,
    // no merge -- in passes of the widest width that fits (4, 2, 1; dense 8, 4, 2, 1)
    LAUNCH_TRY(c, launch_transpose_prologue, d_bias, d_y, m.cols, beta, s, vecs, bias_stride);
    if (alpha == 0.0f) return HISPMV_OK;          // y is exactly beta * bias, per vector
    for (int64_t k = 0; k < vecs;) {
        const int nv = transposed_width(m, vecs - k);
        const float* xk = d_x + k * m.rows;
        float* yk = d_y + k * m.cols;
        if (m.dense) {
            LAUNCH_TRY(c, launch_gemv_t, m.d_dense, m.rows, m.cols, m.value_storage == HISPMV_VALUES_BF16, nv, xk, yk, alpha, s);
        } else if (m.format == 1) {
            LAUNCH_TRY(c, launch_tts_t, m.parts[0].tdev, nv, xk, yk, alpha, s);      // an accepted tile stream: one launch, no carries, no fix-up
        } else {
            for (auto& p : m.parts) LAUNCH_TRY(c, launch_spmv_t, p.dev, nv, xk, yk, alpha, s);
        }
        k += nv;
    }
    return HISPMV_OK;
}

// ---- several vectors on device pointers (include/hispmv.h: hispmv_linear_device, hispmv_linear_device_t) ---------------------------
// `who`'s refusal of a batch whose vectors an int32 offset cannot span
int check_batch_extent(hispmv_ctx* c, const Matrix& m, int64_t num_vecs, const char* who) {
    if ((int64_t)m.rows * num_vecs >= (1LL << 30) || (int64_t)m.cols * num_vecs >= (1LL << 30))
        return fail(c, HISPMV_EINVAL, std::string(who) + ": rows * num_vecs and cols * num_vecs must stay below 2^30 floats; split the batch");
    return HISPMV_OK;
}
// The checks both entries share, all before any device call; on success *out is the handle.
int linear_device_target(hispmv_ctx* c, int idx, const float* d_x, int64_t num_vecs, const float* d_bias, const float* d_y, float beta,
                         const char* who, Matrix** out) {
    if (const int rc = find_handle(c, idx, who, out)) return rc;
    if (num_vecs < 1) return fail(c, HISPMV_EINVAL, std::string(who) + ": num_vecs must be at least 1");
    if (!d_x || !d_y || (beta != 0.0f && !d_bias)) return fail(c, HISPMV_EINVAL, "NULL device vector");
    if (d_x == d_y) return fail(c, HISPMV_EINVAL, std::string(who) + ": x and y must not be the same vectors");
    return check_batch_extent(c, **out, num_vecs, who);
}

// The passes of a forward call with beta != 0 and a shared bias on an aligned d_x, walked along forward_width: widest pass, number of
// passes and -- `launches` given, m a stored transpose -- their launches.
void forward_passes(const Matrix& m, int64_t vecs, int64_t& widest, int64_t& passes, int64_t* launches = nullptr) {
    for (int64_t k = 0; k < vecs;) {
        const int nv = forward_width(m, vecs - k, true, false);
        widest = std::max<int64_t>(widest, nv); passes += 1; k += nv;
        if (launches) *launches += companion_pass_launches(m, nv);
    }
}

// the entry accepts the handle: loaded, updatable (so it has a map, or is dense), and a slice stream or an accepted tile stream
bool value_grad_accepts(const Matrix& m) {
    if (!m.loaded || !m.updatable) return false;
    if (m.dense) return true;
    if (m.format != 0) return transposable_handle(m);      // (an accepted tile stream)
    for (auto& p : m.parts)
        if (p.is_tts) return false;
    return true;
}

}  // namespace

HISPMV_API int hispmv_transpose_info(const hispmv_ctx* c, int idx, int64_t out[4]) {
    if (!c || !out || idx < 0 || idx >= (int)c->mats.size()) return HISPMV_EINVAL;
    const Matrix& m = *c->mats[(size_t)idx];
    if (m.companion) {          // forward launches over the stored transpose: no atomic
        out[0] = m.loaded ? 1 : 0; out[1] = m.loaded ? companion_pass_launches(*m.companion, 1) : 0; out[2] = 0; out[3] = 0;
        return HISPMV_OK;
    }
    const bool ok = m.loaded && transposable_handle(m);
    out[0] = ok ? 1 : 0; out[1] = ok ? m.t_launches : 0; out[2] = ok ? m.t_atomic_bytes : 0; out[3] = ok ? m.t_direct : 0;
    return HISPMV_OK;
}

HISPMV_API int hispmv_spmv_device_t(hispmv_ctx* c, int idx, const float* d_x, const float* d_bias, float* d_y,
                                    float alpha, float beta, void* stream) {
    if (!c) return HISPMV_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    Matrix* mp = nullptr;
    if (const int rc = find_handle(c, idx, "spmv_device_t", &mp)) return rc;
    Matrix& m = *mp;
    if (!d_x || !d_y || (beta != 0.0f && !d_bias)) return fail(c, HISPMV_EINVAL, "NULL device vector");
    if (d_x == d_y) return fail(c, HISPMV_EINVAL, "spmv_device_t: x and y must not be the same vector");
    if (!m.companion && !transposable_handle(m)) return refuse_tile_stream(c, m, "spmv_device_t", "transposed product");
    hipStream_t s;
    if (const int rc = adopt_stream(c, stream, &s)) return rc;
    return launch_transposed(c, m, 1, d_x, d_bias, 0, d_y, alpha, beta, s);
}

HISPMV_API int hispmv_linear_info(const hispmv_ctx* c, int idx, int64_t num_vecs, int64_t out[5]) {
    if (!c || !out || idx < 0 || idx >= (int)c->mats.size() || num_vecs < 1) return HISPMV_EINVAL;
    const Matrix& m = *c->mats[(size_t)idx];
    for (int i = 0; i < 5; ++i) out[i] = 0;
    if (!m.loaded) return HISPMV_OK;
    forward_passes(m, num_vecs, out[0], out[1]);
    if (m.companion) {          // the passes of launch_companion
        forward_passes(*m.companion, num_vecs, out[2], out[3], &out[4]);
        return HISPMV_OK;
    }
    if (!transposable_handle(m)) return HISPMV_OK;
    int64_t launches = 1;           // the prologue
    for (int64_t k = 0; k < num_vecs;) {
        const int nv = transposed_width(m, num_vecs - k);
        out[2] = std::max<int64_t>(out[2], nv); out[3] += 1; k += nv;
        if (m.dense) launches += 1;
        else if (m.format == 1) launches += m.parts[0].tdev.n_tiles > 0 ? 1 : 0;
        else for (auto& p : m.parts) launches += p.dev.n_groups > 0 ? 1 : 0;
    }
    out[4] = launches;
    return HISPMV_OK;
}

HISPMV_API int hispmv_linear_device(hispmv_ctx* c, int idx, const float* d_x, int64_t num_vecs, const float* d_bias, float* d_y,
                                    float alpha, float beta, void* stream) {
    if (!c) return HISPMV_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    Matrix* mp = nullptr;
    const int rc = linear_device_target(c, idx, d_x, num_vecs, d_bias, d_y, beta, "linear_device", &mp);
    if (rc != HISPMV_OK) return rc;
    hipStream_t s;
    if (const int r = adopt_stream(c, stream, &s)) return r;
    return launch_forward(c, *mp, num_vecs, d_x, d_bias, 0, d_y, alpha, beta, s, true);
}

HISPMV_API int hispmv_linear_device_t(hispmv_ctx* c, int idx, const float* d_x, int64_t num_vecs, const float* d_bias, int64_t bias_stride,
                                      float* d_y, float alpha, float beta, void* stream) {
    if (!c) return HISPMV_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    Matrix* mp = nullptr;
    const int rc = linear_device_target(c, idx, d_x, num_vecs, d_bias, d_y, beta, "linear_device_t", &mp);
    if (rc != HISPMV_OK) return rc;
    Matrix& m = *mp;
    if (bias_stride != 0 && bias_stride != m.cols) return fail(c, HISPMV_EINVAL, "linear_device_t: bias_stride must be 0 (one bias for all vectors) or cols");
    if (beta != 0.0f && d_bias == d_y && bias_stride == 0 && num_vecs > 1)
        return fail(c, HISPMV_EINVAL, "linear_device_t: d_bias == d_y needs bias_stride = cols (a shared bias would be overwritten by vector 0)");
    if (!m.companion && !transposable_handle(m)) return refuse_tile_stream(c, m, "spmv_device_t", "transposed product");
    hipStream_t s;
    if (const int r = adopt_stream(c, stream, &s)) return r;
    return launch_transposed(c, m, num_vecs, d_x, d_bias, bias_stride, d_y, alpha, beta, s);
}

// ---- value gradient (include/hispmv.h: hispmv_value_grad_device; kernels: hispmv_value_grad.hip) ---------------------------------
HISPMV_API int hispmv_value_grad_info(const hispmv_ctx* c, int idx, int64_t num_vecs, int64_t out[4]) {
    if (!c || !out || idx < 0 || idx >= (int)c->mats.size() || num_vecs < 1) return HISPMV_EINVAL;
    const Matrix& m = *c->mats[(size_t)idx];
    for (int i = 0; i < 4; ++i) out[i] = 0;
    if (!value_grad_accepts(m)) return HISPMV_OK;
    out[0] = 1;
    if (m.dense) { out[1] = num_vecs; out[2] = 1; out[3] = (m.rows > 0 && m.cols > 0) ? 1 : 0; return HISPMV_OK; }
    for (int64_t k = 0; k < num_vecs;) {
        const int nv = transposed_width(m, num_vecs - k);
        out[1] = std::max<int64_t>(out[1], nv); out[2] += 1; k += nv;
        if (m.format == 1) out[3] += (m.parts[0].tdev.n_tiles > 0 && m.upd_n > 0) ? 1 : 0;
        else for (auto& p : m.parts) out[3] += (p.dev.n_groups > 0 && m.upd_n > 0) ? 1 : 0;
    }
    return HISPMV_OK;
}

HISPMV_API int hispmv_value_grad_device(hispmv_ctx* c, int idx, const float* d_gy, const float* d_x, int64_t num_vecs, float* d_grad,
                                        float alpha, float beta, void* stream) {
    if (!c) return HISPMV_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    Matrix* mp = nullptr;
    if (const int rc = find_handle(c, idx, "value_grad_device", &mp)) return rc;
    Matrix& m = *mp;
    if (!m.updatable) return fail(c, HISPMV_ESTATE, "value_grad_device: handle was not created with value updates on (hispmv_set_value_updates)");
    if (!value_grad_accepts(m)) return refuse_tile_stream(c, m, "value_grad_device", "value-gradient kernel");
    if (num_vecs < 1) return fail(c, HISPMV_EINVAL, "value_grad_device: num_vecs must be at least 1");
    if (!d_gy || !d_x || (m.upd_n > 0 && !d_grad)) return fail(c, HISPMV_EINVAL, "NULL device vector");
    if (d_grad && (d_grad == d_gy || d_grad == d_x)) return fail(c, HISPMV_EINVAL, "value_grad_device: grad must not be gy or x");
    if (const int rc = check_batch_extent(c, m, num_vecs, "value_grad_device")) return rc;
    if (m.upd_n == 0) return HISPMV_OK;
    hipStream_t s;
    if (const int rc = adopt_stream(c, stream, &s)) return rc;
    if (alpha == 0.0f) return scale_in_place(c, d_grad, m.upd_n, beta, s);          // grad = beta * grad exactly, gy and x not read
    if (m.dense) {                // all vectors in one launch
        LAUNCH_TRY(c, launch_value_grad_dense, m.rows, m.cols, num_vecs, d_gy, d_x, d_grad, alpha, beta, s);
        return HISPMV_OK;
    }
    // passes of the widest width that fits (4, 2, 1: the rule of hispmv_linear_device_t); the first stores alpha * s_0 + beta * grad,
    // every later one grad + alpha * s_p
    for (int64_t k = 0; k < num_vecs;) {
        const int nv = transposed_width(m, num_vecs - k);
        if (m.format == 1) {
            const Matrix::Part& p = m.parts[0];
            LAUNCH_TRY(c, launch_tts_value_grad, p.tdev, nv, m.d_map + p.map_chunk_base * kValueChunk, d_gy + k * m.rows, d_x + k * m.cols, d_grad, m.upd_n, alpha,
                       k == 0 ? beta : 1.0f, s);
        } else for (auto& p : m.parts) {
            LAUNCH_TRY(c, launch_value_grad, p.dev, nv, m.d_map + p.map_chunk_base * kValueChunk, d_gy + k * m.rows, d_x + k * m.cols, d_grad, m.upd_n, alpha,
                       k == 0 ? beta : 1.0f, s);
        }
        k += nv;
    }
    return HISPMV_OK;
}

// ---- in-place value updates (include/hispmv.h: hispmv_update_values, hispmv_update_values_device; kernels: hispmv_update.hip) ----
namespace {

// The checks both update entries share; on success *out is the handle.
int update_target(hispmv_ctx* c, int idx, const float* values, int64_t n, Matrix** out) {
    if (const int rc = find_handle(c, idx, nullptr, out)) return rc;      // (this entry asks for `updatable` before `loaded`)
    const Matrix& m = **out;
    if (!m.updatable) return fail(c, HISPMV_ESTATE, "handle was not created with value updates on (hispmv_set_value_updates)");
    if (!m.loaded) return fail(c, HISPMV_ESTATE, "update_values called before load_matrices");
    if (n != m.upd_n) return fail(c, HISPMV_EINVAL, "update_values: n is not the number of values the handle was created with");
    if (n > 0 && !values) return fail(c, HISPMV_EINVAL, "update_values: values is NULL");
    return HISPMV_OK;
}

// d_values (device) into the layouts of m, asynchronous on s
int issue_update(hispmv_ctx* c, Matrix& m, const float* d_values, hipStream_t s) {
    if (m.upd_n == 0) return HISPMV_OK;
    const bool bf16 = m.value_storage == HISPMV_VALUES_BF16;
    if (m.dense && bf16) {
        LAUNCH_TRY(c, launch_update_dense_bf16, (uint16_t*)m.d_dense, d_values, m.upd_n, s);
        return HISPMV_OK;
    }
    if (m.dense) {
        HIP_TRY(c, hipMemcpyAsync(m.d_dense, d_values, (size_t)m.upd_n * 4, hipMemcpyDeviceToDevice, s));
        return HISPMV_OK;
    }
    LAUNCH_TRY_AS(c, "launch_update_values", bf16 ? launch_update_values_bf16(m.d_upd_table, m.map_slots / kValueChunk, m.d_map, d_values, m.upd_n, s)
                                                  : launch_update_values(m.d_upd_table, m.map_slots / kValueChunk, m.d_map, d_values, m.upd_n, s));
    return m.companion ? issue_update(c, *m.companion, d_values, s) : HISPMV_OK;      // the stored transpose: the same values through its own map
}

}  // namespace

HISPMV_API int hispmv_update_values(hispmv_ctx* c, int idx, const float* values, int64_t n) {
    if (!c) return HISPMV_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    Matrix* m = nullptr;
    int rc = update_target(c, idx, values, n, &m);
    if (rc != HISPMV_OK || n == 0) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    // pinned staging, ONE copy into the context's scratch, the kernel, a synchronise
    if (n > c->cap_h_upd) {
        host_free(c->h_upd);
        c->cap_h_upd = 0;
        HIP_TRY(c, hipHostMalloc((void**)&c->h_upd, (size_t)n * sizeof(float), hipHostMallocDefault));
        c->cap_h_upd = n;
    }
    if ((rc = ensure_vec(c, &c->d_upd, &c->cap_d_upd, n)) != HISPMV_OK) return rc;
    std::memcpy(c->h_upd, values, (size_t)n * sizeof(float));
    HIP_TRY(c, hipMemcpyAsync(c->d_upd, c->h_upd, (size_t)n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if ((rc = issue_update(c, *m, c->d_upd, c->stream)) != HISPMV_OK) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return HISPMV_OK;
}

HISPMV_API int hispmv_update_values_device(hispmv_ctx* c, int idx, const float* d_values, int64_t n, void* stream) {
    if (!c) return HISPMV_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    Matrix* m = nullptr;
    const int rc = update_target(c, idx, d_values, n, &m);
    if (rc != HISPMV_OK) return rc;
    hipStream_t s;
    if (const int r = adopt_stream(c, stream, &s)) return r;
    return issue_update(c, *m, d_values, s);
}
