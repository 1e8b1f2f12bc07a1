// hispmv_abi.cpp -- the context of libhispmv.so's C ABI (include/hispmv.h): error reporting, creation and teardown, arena
// accounting, the hispmv_set_* switches and the info getters that only read a handle's fields.  MI355X counterpart of the
// reference's FpgaHandle (pyhispmv/src/fpga_handle.cpp:40-388), which owns the XRT device, the per-channel matrix arena and the
// kernel run object.  Handles are made in hispmv_create.cpp, uploaded in hispmv_load.cpp, launched from hispmv_launch.cpp (hispmv_ctx.h).
#include "hispmv_ctx.h"

using namespace hispmv;

static thread_local std::string g_create_err, g_prep_err;

namespace hispmv {
int fail(hispmv_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg; else g_create_err = msg;
    return code;
}
int hip_fail(hispmv_ctx* c, hipError_t e, const char* what) {
    return fail(c, HISPMV_EDEVICE, std::string(what) + ": " + hipGetErrorString(e));
}
std::string& prep_error() { return g_prep_err; }
std::atomic<int64_t> g_free_failures{0};
// A bounded in-kernel wait that expired leaves 1 in the context's error word.
int check_device_error(hispmv_ctx* c) {
    // callers have synchronised the stream the kernels ran on; the word lives in host memory
    const int flag = *(volatile int*)c->h_err;
    if (flag) {
        *(volatile int*)c->h_err = 0;
        return fail(c, HISPMV_EDEVICE, "carry hand-off between slices timed out (lost or overlapping launch on one handle)");
    }
    return HISPMV_OK;
}
int ensure_vec(hispmv_ctx* c, float** p, int64_t* cap, int64_t n) {
    if (n <= *cap) return HISPMV_OK;
    dev_free(*p);
    *cap = 0;
    const int64_t want = std::max<int64_t>(n, 1024);
    HIP_TRY(c, hipMalloc((void**)p, (size_t)want * sizeof(float)));
    *cap = want;
    return HISPMV_OK;
}

// ---- what the transposed and gradient entries accept (hispmv_launch.cpp, hispmv_krylov_abi.cpp) --------------------------------
// A tile-stream handle the transposed and gradient entries accept (hispmv_tts_transpose.h): created in state _KEEP_FORMAT, one part,
// stream words for every row -- the standard and the small geometry.
static bool tts_transposable(const Matrix& m) {
    return !m.dense && m.format == 1 && m.keep_format && m.parts.size() == 1 && m.parts[0].is_tts && tts_t_accepts(m.parts[0].tdev);
}
// the transposed and gradient entries accept the (loaded) handle: dense, a slice stream, or such a tile stream
bool transposable_handle(const Matrix& m) { return m.dense || m.format == 0 || tts_transposable(m); }
// HISPMV_ENOTSUP for a tile stream that is not accepted, with the remedies (or the geometry that has no kernel) in the message
int refuse_tile_stream(hispmv_ctx* c, const Matrix& m, const char* who, const char* what) {
    if (m.keep_format) {
        const TtsDeviceMatrix& d = m.parts[0].tdev;
        const char* geometry = d.zero_fill == 2 ? "tallgap" : d.threads == kTtsPairedThreads ? "paired" : "tall";
        return fail(c, HISPMV_ENOTSUP, std::string(who) + ": this handle is a transposed tile stream in the " + geometry + " geometry (HISPMV_TTS_GEOMETRY), which has no " + what +
                                           "; create it under the standard geometry, or after hispmv_set_transposable(ctx, 1) (FpgaHandle.set_transposable(True)) so that "
                                           "it keeps the slice stream");
    }
    return fail(c, HISPMV_ENOTSUP, std::string(who) + ": this handle is a transposed tile stream created with hispmv_set_transposable off, which has no " + what +
                                       "; create it after hispmv_set_transposable(ctx, 1) (FpgaHandle.set_transposable(True)) so that it keeps the slice stream, or after "
                                       "hispmv_set_transposable(ctx, 2) (FpgaHandle.set_transposable(\"keep_format\")) so that the tile stream itself is accepted");
}

}  // namespace hispmv

// ------------------------------------------------------------------------------------------------
// `stream` NULL = the context's stream, exactly as in hispmv_spmv_device / hispmv_spmv_device_batch: a caller that passes NULL
// everywhere gets its SpMVs and its boundary kernels on ONE queue, in order.  (Until round 3 NULL meant HIP's null stream here:
// the boundary kernels then did not wait for SpMVs issued with NULL on the context's non-blocking stream.)
HISPMV_API int hispmv_boundary_pack(hispmv_ctx* c, const float* const* d_last, const float* d_mask, float* d_send, int32_t n, void* stream) {
    if (!c) return HISPMV_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    if (n < 0 || (n > 0 && (!d_last || !d_mask || !d_send))) return fail(c, HISPMV_EINVAL, "bad boundary_pack arguments");
    hipStream_t s;
    if (const int rc = adopt_stream(c, stream, &s)) return rc;
    LAUNCH_TRY(c, launch_boundary_pack, d_last, d_mask, d_send, n, s);
    return HISPMV_OK;
}

HISPMV_API int hispmv_boundary_apply(hispmv_ctx* c, float* const* d_first, const float* d_recv, const float* d_weights, int32_t n,
                                     int32_t world, void* stream) {
    if (!c) return HISPMV_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    if (n < 0 || world < 1 || (n > 0 && (!d_first || !d_recv || !d_weights))) return fail(c, HISPMV_EINVAL, "bad boundary_apply arguments");
    hipStream_t s;
    if (const int rc = adopt_stream(c, stream, &s)) return rc;
    LAUNCH_TRY(c, launch_boundary_apply, d_first, d_recv, d_weights, n, world, s);
    return HISPMV_OK;
}

HISPMV_API const char* hispmv_version(void) { return "hispmv-amd 0.2.0 gfx950"; }
HISPMV_API int64_t hispmv_free_failures(void) { return g_free_failures.load(); }
HISPMV_API const char* hispmv_last_error(const hispmv_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

HISPMV_API int hispmv_create(hispmv_ctx** out, const char* xclbin_path, int device_id, int a, int b, int cc,
                             int urams, int fp_acc_latency, int dense, int pre_acc, int row_dist) {
    if (!out) return fail(nullptr, HISPMV_EINVAL, "out is NULL");
    *out = nullptr;
    host_threads();       // OpenMP threads of the preprocessor = the CPUs this process may use (cgroup quota)
    // same argument checks as fpga_handle.cpp:51-52,70-71
    if (device_id < 0) return fail(nullptr, HISPMV_EINVAL, "Device ID must be a non-negative integer.");
    if (!xclbin_path || !*xclbin_path) return fail(nullptr, HISPMV_EINVAL, "XCLBIN path is empty.");
    if (a <= 0 || b <= 0 || cc <= 0) return fail(nullptr, HISPMV_EINVAL, "channel counts must be positive");
    if ((a * 8) % (cc * 16) != 0)   // spmv-helper.cpp:15
        return fail(nullptr, HISPMV_EINVAL, "Number of PEs should be an integer multiple of Number of FP32 elements in output vector");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, HISPMV_EDEVICE, std::string("no HIP device available: ") + (e != hipSuccess ? hipGetErrorString(e) : "device count is 0"));
    if (device_id >= ndev) return fail(nullptr, HISPMV_EDEVICE, "device_id out of range");
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device_id)) != hipSuccess) return hip_fail(nullptr, e, "hipGetDeviceProperties");
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, HISPMV_EDEVICE, std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
    if ((e = hipSetDevice(device_id)) != hipSuccess) return hip_fail(nullptr, e, "hipSetDevice");

    auto c = std::make_unique<hispmv_ctx>();
    c->device = device_id;
    c->num_ch_A = a; c->num_ch_B = b; c->num_ch_C = cc; c->urams_per_pe = urams; c->fp_acc_latency = fp_acc_latency;
    c->dense_overlay = dense != 0; c->pre_accumulator = pre_acc != 0; c->row_dist_net = row_dist != 0;
    c->arena_budget = (int64_t)a * 256 * 1024 * 1024;      // fpga_handle.h:12, one 256 MiB bank per A channel
    if (const char* env = std::getenv("HISPMV_ARENA_BYTES")) { long long v = std::atoll(env); if (v > 0) c->arena_budget = v; }
    // from here on the context owns HIP objects: a failure releases them through hispmv_destroy
    auto give_up = [&](hipError_t err, const char* what) { hispmv_destroy(c.release()); return hip_fail(nullptr, err, what); };
    if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess) return give_up(e, "hipStreamCreate");
    if ((e = hipEventCreate(&c->ev0)) != hipSuccess || (e = hipEventCreate(&c->ev1)) != hipSuccess) return give_up(e, "hipEventCreate");
    if ((e = hipHostMalloc((void**)&c->h_err, sizeof(int), hipHostMallocMapped)) != hipSuccess) return give_up(e, "hipHostMalloc(err flag)");
    *c->h_err = 0;
    if ((e = hipHostGetDevicePointer((void**)&c->d_err, c->h_err, 0)) != hipSuccess) return give_up(e, "hipHostGetDevicePointer(err flag)");
    c->format_opts = FormatOptions::from_env();
    if (const char* env = std::getenv("HISPMV_CARRY"))
        c->carry_mode = !std::strcmp(env, "fixup") ? 0 : !std::strcmp(env, "lookback") ? 1 : !std::strcmp(env, "ticket") ? 3 : !std::strcmp(env, "resident") ? 5 : 2;
    if (const char* env = std::getenv("HISPMV_BATCH_GRAPH")) c->batch_graphs = std::atoi(env) != 0;
    if (const char* env = std::getenv("HISPMV_STEP_KERNEL")) c->step_kernel = std::atoi(env) != 0;
    if (const char* env = std::getenv("HISPMV_STEP_HALF")) c->step_half = std::atoi(env) != 0;      // (hispmv_set_step_half; HISPMV_STEP_KERNEL=0 still wins)
    if (const char* env = std::getenv("HISPMV_STEP_ORDER")) c->step_order = !std::strcmp(env, "lpt") ? 1 : !std::strcmp(env, "grid") ? 2 : !std::strcmp(env, "alt2") ? 3 : !std::strcmp(env, "alt3") ? 4 : std::atoi(env) >= 16 ? std::atoi(env) : 0;
    if (const char* env = std::getenv("HISPMV_BATCH_ORDER")) c->batch_order = !std::strcmp(env, "small_first") ? 1 : 0;
    if (const char* env = std::getenv("HISPMV_BATCH_LANES")) c->batch_lanes_heavy_first = std::strcmp(env, "rr") != 0;
    if (const char* env = std::getenv("HISPMV_BATCH_STREAMS")) { c->batch_streams = std::max(1, std::min(3, std::atoi(env))); c->batch_streams_min_bytes = 0; }
    // Experiment (HISPMV_CU_SPLIT=<hexA>:<hexB>, round 4): the two side streams get CU masks (the 32-bit pattern repeated over the
    // device's CUs) and a batch call sends its slice / dense grids to side stream 0 and its tile-stream grids to side stream 1 --
    // an HBM-bound grid does not need every CU to saturate the memory, a cache-bound one wants as many as it can get.
    uint32_t cu_pat[2] = {0, 0};
    if (const char* env = std::getenv("HISPMV_CU_SPLIT")) {
        char* end = nullptr;
        cu_pat[0] = (uint32_t)std::strtoul(env, &end, 16);
        if (end && *end == ':') cu_pat[1] = (uint32_t)std::strtoul(end + 1, nullptr, 16);
        c->cu_split = cu_pat[0] != 0 && cu_pat[1] != 0;
    }
    for (int i = 0; i < 2; ++i) {
        if (c->cu_split) {
            std::vector<uint32_t> mask((size_t)(prop.multiProcessorCount + 31) / 32, cu_pat[i]);
            if ((e = hipExtStreamCreateWithCUMask(&c->side[i], (uint32_t)mask.size(), mask.data())) != hipSuccess) return give_up(e, "hipExtStreamCreateWithCUMask");
        } else
        if ((e = hipStreamCreateWithFlags(&c->side[i], hipStreamNonBlocking)) != hipSuccess) return give_up(e, "hipStreamCreate(side)");
        if ((e = hipEventCreateWithFlags(&c->ev_join[i], hipEventDisableTiming)) != hipSuccess) return give_up(e, "hipEventCreate(join)");
    }
    if ((e = hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming)) != hipSuccess) return give_up(e, "hipEventCreate(fork)");
    if (const char* env = std::getenv("HISPMV_PREP"))
        c->prep_mode = !std::strcmp(env, "host") ? 0 : !std::strcmp(env, "device") ? 1 : 2;
    c->n_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (const char* env = std::getenv("HISPMV_PLAN_CUS")) { const int v = std::atoi(env); if (v > 0) c->n_cus = v; }   // experiments
    *out = c.release();
    return HISPMV_OK;
}

HISPMV_API void hispmv_destroy(hispmv_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (auto& m : c->mats) free_matrix_device(*m);
    dev_free(c->d_x);
    dev_free(c->d_y);
    host_free(c->h_err);
    host_free(c->h_stage);
    host_free(c->h_upd);
    dev_free(c->d_upd);
    free_batch_plans(c);
    for (int i = 0; i < 2; ++i) { if (c->side[i]) (void)hipStreamDestroy(c->side[i]); if (c->ev_join[i]) (void)hipEventDestroy(c->ev_join[i]); }
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

HISPMV_API int hispmv_set_arena_bytes(hispmv_ctx* c, int64_t bytes) {
    if (!c || bytes < 0) return HISPMV_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    c->arena_budget = bytes;
    return HISPMV_OK;
}
HISPMV_API int64_t hispmv_arena_bytes_used(const hispmv_ctx* c) { return c ? c->arena_used : 0; }
HISPMV_API int hispmv_select_matrix(hispmv_ctx* c, uint32_t idx) {
    if (!c) return HISPMV_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    if (idx >= c->mats.size()) return idx_out_of_range(c);
    c->selected = (int)idx;
    return HISPMV_OK;
}

HISPMV_API int hispmv_synchronize(hispmv_ctx* c) {
    if (!c) return HISPMV_EINVAL;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->user_stream) {
        const hipError_t e = hipStreamSynchronize(c->user_stream);
        if (e == hipErrorInvalidHandle || e == hipErrorInvalidResourceHandle || e == hipErrorContextIsDestroyed) {
            (void)hipGetLastError();          // the caller has destroyed that stream since: nothing left to wait for
            c->user_stream = nullptr;
        } else if (e != hipSuccess) return hip_fail(c, e, "hipStreamSynchronize(caller stream)");
    }
    return check_device_error(c);
}
HISPMV_API float hispmv_last_kernel_ms(hispmv_ctx* c) { return c ? c->last_ms : -1.0f; }

// ---- the switches handles are created under (include/hispmv.h) ------------------------------------------------------------------
// transposed product: hispmv_spmv_device_t; kernels: hispmv_transpose.hip
HISPMV_API int hispmv_set_transposable(hispmv_ctx* c, int enable) {
    if (!c) return HISPMV_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    if (enable != HISPMV_TRANSPOSABLE_OFF && enable != HISPMV_TRANSPOSABLE_SLICES && enable != HISPMV_TRANSPOSABLE_KEEP_FORMAT && enable != HISPMV_TRANSPOSABLE_COMPANION)
        return fail(c, HISPMV_EINVAL, "set_transposable: unknown state (HISPMV_TRANSPOSABLE_OFF, _SLICES, _KEEP_FORMAT or _COMPANION)");
    c->transposable = enable;
    return HISPMV_OK;
}
// bf16 value storage
HISPMV_API int hispmv_set_value_storage(hispmv_ctx* c, int storage) {
    if (!c) return HISPMV_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    if (storage != HISPMV_VALUES_FP32 && storage != HISPMV_VALUES_BF16) return fail(c, HISPMV_EINVAL, "unknown value storage (HISPMV_VALUES_FP32 or HISPMV_VALUES_BF16)");
    c->value_storage = storage;
    return HISPMV_OK;
}
// in-place value updates
HISPMV_API int hispmv_set_value_updates(hispmv_ctx* c, int enable) {
    if (!c) return HISPMV_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    c->value_updates = enable != 0;          // (any value but 0 and _ANY_STORAGE is _ON, as before the third state existed)
    c->updates_any_storage = enable == HISPMV_VALUE_UPDATES_ANY_STORAGE;
    return HISPMV_OK;
}

// ---- the getters that only read a handle's fields (those that walk the pass plan: hispmv_launch.cpp) ---------------------------
HISPMV_API int hispmv_num_matrices(const hispmv_ctx* c) { return c ? (int)c->mats.size() : 0; }
HISPMV_API int hispmv_get_matrix_info(const hispmv_ctx* c, int idx, hispmv_matrix_info* out) {
    if (!c || !out || idx < 0 || idx >= (int)c->mats.size()) return HISPMV_EINVAL;
    const Matrix& m = *c->mats[idx];
    out->rows = m.rows; out->cols = m.cols; out->nnz = m.nnz; out->is_dense = m.dense; out->loaded = m.loaded;
    out->n_slices = m.n_slices; out->n_elems = m.n_elems; out->n_split_rows = m.n_split;
    out->device_bytes = m.device_bytes; out->prep_seconds = m.prep_seconds;
    out->block_threads = m.plan_threads; out->group_slices = m.plan_group; out->lds_bytes = m.plan_lds * 4;
    out->col_tiles = (int32_t)m.parts.size();
    out->carry_lookback = (!m.dense && !m.parts.empty() && m.parts[0].dev.lookback) ? 1 : 0; out->col_tile_width = m.col_tile_width; out->col_tile_base = m.col_tile_base; out->compact_slices = (int32_t)std::min<int64_t>(m.compact_slices, INT32_MAX);
    out->format = m.format; out->tts_lines_per_gather = (float)m.tts_lines_per_gather;
    out->tile_kind = m.parts.size() > 1 ? (m.tile_kind ? m.tile_kind : 1) : 0;
    out->batch_group_slices = 0;
    if (m.parts.size() == 1 && !m.parts[0].is_tts)
        out->batch_group_slices = m.loaded ? (m.parts[0].has_batch_dev ? m.parts[0].batch_dev.group_slices : 0) : (m.parts[0].has_batch_layout ? m.parts[0].batch_plan.group_slices : 0);
    return HISPMV_OK;
}

HISPMV_API int hispmv_companion_info(const hispmv_ctx* c, int idx, int64_t out[6]) {
    if (!c || !out || idx < 0 || idx >= (int)c->mats.size()) return HISPMV_EINVAL;
    for (int i = 0; i < 6; ++i) out[i] = 0;
    const Matrix* t = c->mats[(size_t)idx]->companion.get();
    if (!t) return HISPMV_OK;
    out[0] = 1; out[1] = t->format; out[2] = (int64_t)t->parts.size(); out[3] = t->device_bytes; out[4] = t->map_slots;
    out[5] = t->parts.size() > 1 ? (t->tile_kind ? t->tile_kind : 1) : 0;
    return HISPMV_OK;
}

HISPMV_API int hispmv_value_storage_info(const hispmv_ctx* c, int idx, int64_t out[4]) {
    if (!c || !out || idx < 0 || idx >= (int)c->mats.size()) return HISPMV_EINVAL;
    const Matrix& m = *c->mats[(size_t)idx];
    out[0] = m.value_storage; out[1] = m.slots_2byte; out[2] = m.slots_4byte; out[3] = m.saved_bytes;
    return HISPMV_OK;
}

HISPMV_API int hispmv_value_update_info(const hispmv_ctx* c, int idx, int64_t out[4]) {
    if (!c || !out || idx < 0 || idx >= (int)c->mats.size()) return HISPMV_EINVAL;
    const Matrix& m = *c->mats[idx];
    out[0] = m.updatable ? 1 : 0; out[1] = m.upd_n; out[2] = m.map_slots; out[3] = m.upd_written + (m.companion ? m.companion->upd_written : 0);
    return HISPMV_OK;
}
