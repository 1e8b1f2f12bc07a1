// hispmv_create.cpp -- the four hispmv_create_*_handle* entries of the C ABI (include/hispmv.h): the creation checks, COO / CSR ->
// prepared matrix (choose_format, hispmv_choose.cpp), byte accounting and the arena charge.  Host work only, but for the device
// preprocessor (hispmv_prep_device.h); the upload is hispmv_load.cpp.
#include "hispmv_ctx.h"

using namespace hispmv;

namespace {

// Value updates: the layouts of an updatable handle are packed from these payloads instead of its values -- the bits of k + 1 for
// input position k, so that every value slot names the entry it holds (fp32 denormals below 2^23: nothing on the way does
// arithmetic on a value, and nothing is built with fast-math).  Capped below the bits of +inf.
constexpr int64_t kMaxUpdatableEntries = 0x7F7FFFFFll;
std::vector<float> index_payloads(int64_t n) {
    std::vector<float> p((size_t)n);
#pragma omp parallel for num_threads(host_threads()) schedule(static)
    for (int64_t k = 0; k < n; ++k) {
        const uint32_t b = (uint32_t)(k + 1);
        std::memcpy(&p[(size_t)k], &b, 4);
    }
    return p;
}

// The switches DESIGN records as negative experiments change the tile stream's words beyond what value_chunks describes: refused.
int check_updatable(hispmv_ctx* c, int64_t nnz) {
    if (nnz > kMaxUpdatableEntries) return fail(c, HISPMV_EINVAL, "value updates: more entries than an index payload can name");
    if (c->format_opts.tts_geometry != 0 || c->format_opts.tts_small)
        return fail(c, HISPMV_EINVAL, "value updates: not supported with HISPMV_TTS_GEOMETRY other than standard or HISPMV_TTS_SMALL (experiments)");
    return HISPMV_OK;
}

// bf16 value storage (include/hispmv.h: hispmv_set_value_storage): R over n values, once, before any packer sees them.
void round_values_to_bf16(const float* in, float* out, int64_t n) {
#pragma omp parallel for num_threads(host_threads()) schedule(static)
    for (int64_t k = 0; k < n; ++k) {
        uint32_t u;
        std::memcpy(&u, in + k, 4);
        u = round_bits_to_bf16(u);
        std::memcpy(out + k, &u, 4);
    }
}
// (HISPMV_VALUE_UPDATES_ANY_STORAGE lifts this: the map of a bf16 handle is read on the host, add_sparse)
int check_storage_and_updates(hispmv_ctx* c) {
    if (c->value_storage == HISPMV_VALUES_BF16 && c->value_updates && !c->updates_any_storage)
        return fail(c, HISPMV_EINVAL, "bf16 value storage and value updates are both on: the value map lives in 32-bit value slots (create the handle with one of the two switched off)");
    return HISPMV_OK;
}
// Creation in state HISPMV_TRANSPOSABLE_COMPANION: the rule of check_updatable -- the forward launches of a stored transpose are those of
// the standard tile geometry.
int check_companion(hispmv_ctx* c) {
    if (c->transposable == HISPMV_TRANSPOSABLE_COMPANION && (c->format_opts.tts_geometry != 0 || c->format_opts.tts_small))
        return fail(c, HISPMV_EINVAL, "set_transposable(companion): not supported with HISPMV_TTS_GEOMETRY other than standard or HISPMV_TTS_SMALL (experiments)");
    return HISPMV_OK;
}
// What the context's switches refuse for a sparse handle of nnz entries, in this order
int check_sparse_creation(hispmv_ctx* c, int64_t nnz) {
    int rc = check_storage_and_updates(c);
    if (rc == HISPMV_OK) rc = check_companion(c);
    if (rc == HISPMV_OK && c->value_updates) rc = check_updatable(c, nnz);
    return rc;
}

// Registers a prepared sparse matrix with the context (capacity check = the reference's
// "offset + size > MAX_BUFFER_SIZE_BYTES -> return -1", fpga_handle.cpp:192-195).  The format and tiling decision itself is
// host-only code: choose_format (hispmv_choose.cpp).
// real_values (updatable handles): the creation input's values in input order; csr then holds their index payloads.
// make_sparse prepares the matrix and counts its bytes, register_sparse charges the arena and lists it -- with its stored transpose
// (`companion`: made from the swapped input, Matrix::companion), when there is one, as ONE capacity check on the sum.
std::unique_ptr<Matrix> make_sparse(hispmv_ctx* c, Csr&& csr, double t_csr, SliceStream* prebuilt, const std::vector<float>* real_values, bool companion) {
    auto t0 = std::chrono::steady_clock::now();
    // HISPMV_PREP_TRACE=1: the phases of the host side of preprocessing on stderr (diagnostics)
    static const bool trace = std::getenv("HISPMV_PREP_TRACE") != nullptr;
    auto lap = [&, last = t0](const char* what) mutable {
        if (!trace) return;
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[hispmv prep] %-28s %7.1f ms\n", what, std::chrono::duration<double>(now - last).count() * 1e3);
        last = now;
    };
    if (trace) std::fprintf(stderr, "[hispmv prep] %-28s %7.1f ms (device: upload %.1f csr %.1f offsets %.1f stream %.1f download %.1f)\n", "COO -> CSR (-> stream)", t_csr * 1e3,
                            c->last_prep_times.upload * 1e3, c->last_prep_times.csr_device * 1e3, c->last_prep_times.offsets_host * 1e3,
                            c->last_prep_times.stream_device * 1e3, c->last_prep_times.download * 1e3);
    auto m = std::make_unique<Matrix>();
    m->rows = csr.rows; m->cols = csr.cols; m->nnz = csr.nnz();
    FormatOptions opts = c->format_opts;
    opts.half_values = c->value_storage == HISPMV_VALUES_BF16;      // (the values are rounded already: add_from_coo, _from_csr)
    opts.index_payloads = opts.half_values && real_values;          // ... or are index payloads: every part keeps its chunks of the map on the host
    if (c->transposable == HISPMV_TRANSPOSABLE_SLICES) opts.format_mode = 0;      // hispmv_set_transposable: keep the slice stream, as HISPMV_FORMAT=slices does
    // ... or the loader's own choice, a tile stream then marked as accepted (_COMPANION: the same, the stored transpose besides)
    m->keep_format = !companion && (c->transposable == HISPMV_TRANSPOSABLE_KEEP_FORMAT || c->transposable == HISPMV_TRANSPOSABLE_COMPANION);
    if (companion) opts.batch_layout = false;      // only step-kernel calls read a batch layout, and a companion is never part of one
    m->value_storage = c->value_storage;
    FormatChoice ch = choose_format(std::move(csr), prebuilt, c->n_cus, opts, lap);
    m->format = ch.format; m->tile_kind = ch.tile_kind; m->col_tile_width = ch.col_tile_width; m->col_tile_base = ch.col_tile_base;
    m->l2_tiles = ch.l2_tiles; m->tts_lines_per_gather = ch.tts_lines_per_gather;
    for (HostPart& hp : ch.parts) {
        m->parts.emplace_back();
        static_cast<HostPart&>(m->parts.back()) = std::move(hp);
    }
    for (auto& p : m->parts) {
        if (p.is_tts && opts.index_payloads) p.value_map = host_value_map(p);       // (slice parts: pack_part, before their words went)
        if (p.is_tts) {
            m->n_slices += (int64_t)p.tts.col_base.size(); m->n_elems += p.tts.nnz + p.tts.n_fillers; m->n_split += (int64_t)p.tts.fix.size() / 4;
            m->device_bytes += p.tts.bytes();
            m->slots_4byte += (int64_t)p.tts.words.size() / 8;
        } else {
            m->n_slices += p.st.n_slices; m->n_elems += p.st.n_elems; m->n_split += (int64_t)p.st.fix.size();
            // the first layout and what the part owns besides: its fix lists, 12 bytes of carries per slice and the ticket
            m->device_bytes += slice_layout_device_bytes(p.st, p.plan, p.dstream) + (int64_t)p.st.fix.size() * 16 + (int64_t)p.st.n_slices * 12 + 8;
            if (p.has_batch_layout) m->device_bytes += slice_layout_device_bytes(p.st, p.batch_plan, p.batch_dstream);
            m->compact_slices += p.dstream.compact_slices;
            // value slots by size: the slices of half groups hold bf16 values and are kSliceUnit bytes shorter than compact ones
            for (const DeviceStream* ds : {&p.dstream, p.has_batch_layout ? &p.batch_dstream : nullptr}) {
                if (!ds) continue;
                const int64_t half = ds->half_values ? ds->compact_slices : 0;
                m->slots_2byte += half * kSliceElems;
                m->slots_4byte += (p.st.n_slices - half) * kSliceElems;
                m->saved_bytes += half * (kCompactSliceBytes - kHalfSliceBytes);
            }
        }
    }
    if (m->parts.size() > 1) m->device_bytes += (int64_t)(m->parts.size() - 1) * kMaxBatch * m->rows * 4;   // partial vectors of parts t > 0
    if (real_values) {          // the map and its chunk table count against the arena
        m->updatable = true;
        m->upd_n = (int64_t)real_values->size();
        int64_t chunks = 0;
        for (const HostPart& p : m->parts)
            for (const ValueChunk& q : value_chunks(p)) { ++chunks; m->upd_written += kValueChunk * (q.off1 >= 0 ? 2 : 1); }
        m->map_slots = chunks * kValueChunk;
        m->device_bytes += m->map_slots * 4 + chunks * (int64_t)sizeof(ValueChunkDev);
    }
    if (m->format == 1) {
        m->plan_threads = m->parts[0].tts.geometry.threads; m->plan_group = m->parts[0].tts.geometry.max_slots / kTtsChunk; m->plan_lds = 0;
    } else {
        m->plan_threads = m->parts[0].plan.block_threads; m->plan_group = m->parts[0].plan.group_slices; m->plan_lds = m->parts[0].plan.lds_floats;
    }
    m->prep_seconds = t_csr + std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return m;
}
// The capacity check on a handle's device_bytes (its stored transpose's among them), the arena charge and its place in the list
int register_handle(hispmv_ctx* c, std::unique_ptr<Matrix> m) {
    if (c->arena_used + m->device_bytes > c->arena_budget) return HISPMV_FULL;
    c->arena_used += m->device_bytes;
    m->index = (int)c->mats.size();
    if (m->companion) m->companion->index = kCompanionId + m->index;
    c->mats.push_back(std::move(m));
    return (int)c->mats.size() - 1;
}
int register_sparse(hispmv_ctx* c, std::unique_ptr<Matrix> m, std::unique_ptr<Matrix> companion, std::vector<float>* real_values) {
    if (companion) { m->device_bytes += companion->device_bytes; m->prep_seconds += companion->prep_seconds; }
    if (real_values && companion) companion->upd_values = *real_values;      // (each load gathers the creation values into its own layouts)
    if (real_values) m->upd_values = std::move(*real_values);
    m->companion = std::move(companion);
    return register_handle(c, std::move(m));
}

// COO -> prepared matrix, on the device or on the host (hispmv_ctx::prep_mode); `v` as the packers take it (rounded, or index payloads)
int make_from_coo(hispmv_ctx* c, int32_t rows, int32_t cols, int64_t nnz, const int32_t* r, const int32_t* cl, const float* v,
                  std::chrono::steady_clock::time_point t0, const std::vector<float>* real_values, bool companion, std::unique_ptr<Matrix>& out) {
    const bool on_device = c->prep_mode == 1 || (c->prep_mode == 2 && nnz >= (2 << 20));
    if (on_device) {
        HIP_TRY(c, hipSetDevice(c->device));
        Csr csr; SliceStream st; std::string err;
        if (!prep_on_device(rows, cols, nnz, r, cl, v, csr, st, c->last_prep_times, err))
            return fail(c, err.find("outside") != std::string::npos || err.find("dimension") != std::string::npos ? HISPMV_EINVAL : HISPMV_EDEVICE, err);
        double t = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        out = make_sparse(c, std::move(csr), t, &st, real_values, companion);
        return HISPMV_OK;
    }
    Csr csr = coo_to_csr(rows, cols, nnz, r, cl, v);
    double t = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    out = make_sparse(c, std::move(csr), t, nullptr, real_values, companion);
    return HISPMV_OK;
}

// COO -> handle (and, in state HISPMV_TRANSPOSABLE_COMPANION, its stored transpose)
int add_from_coo(hispmv_ctx* c, int32_t rows, int32_t cols, int64_t nnz, const int32_t* r, const int32_t* cl, const float* v) {
    auto t0 = std::chrono::steady_clock::now();
    std::vector<float> real, payloads, rounded;
    if (const int rc = check_sparse_creation(c, nnz)) return rc;
    if (c->value_storage == HISPMV_VALUES_BF16) {      // rounded once, here: the host and the device preprocessor see R(v)
        rounded.resize((size_t)nnz);
        round_values_to_bf16(v, rounded.data(), nnz);
        v = rounded.data();
    }
    if (c->value_updates) {
        real.assign(v, v + nnz);
        payloads = index_payloads(nnz);
        v = payloads.data();
    }
    std::vector<float>* const real_values = c->value_updates ? &real : nullptr;
    std::unique_ptr<Matrix> m, companion;
    int rc = make_from_coo(c, rows, cols, nnz, r, cl, v, t0, real_values, false, m);
    // the stored transpose: the swapped input, the same values (rounded, or index payloads) in the same order
    if (rc == HISPMV_OK && c->transposable == HISPMV_TRANSPOSABLE_COMPANION)
        rc = make_from_coo(c, cols, rows, nnz, cl, r, v, std::chrono::steady_clock::now(), real_values, true, companion);
    if (rc != HISPMV_OK) return rc;
    return register_sparse(c, std::move(m), std::move(companion), real_values);
}

}  // namespace

HISPMV_API int hispmv_create_sparse_handle(hispmv_ctx* c, const int32_t* r, const int32_t* cl, const float* v,
                                           int64_t nnz, int32_t rows, int32_t cols) {
    if (!c) return HISPMV_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    if (rows <= 0 || cols <= 0 || nnz < 0 || (nnz > 0 && (!r || !cl || !v))) return fail(c, HISPMV_EINVAL, "bad sparse matrix arguments");
    try {
        return add_from_coo(c, rows, cols, nnz, r, cl, v);
    } catch (const std::out_of_range& ex) { return fail(c, HISPMV_EINVAL, ex.what());
    } catch (const std::bad_alloc&) { return fail(c, HISPMV_ENOMEM, "host out of memory");
    } catch (const std::exception& ex) { return fail(c, HISPMV_EINVAL, ex.what()); }
}

HISPMV_API int hispmv_create_sparse_handle_from_mtx(hispmv_ctx* c, const char* path, int flavor) {
    if (!c) return HISPMV_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    if (!path || (flavor != 0 && flavor != 1)) return fail(c, HISPMV_EINVAL, "bad arguments");
    // the reader drops zeros and mirrors symmetric entries: there is no input order an update could follow
    if (c->value_updates) return fail(c, HISPMV_EINVAL, "value updates: a MatrixMarket handle cannot be updated (create it from COO or CSR)");
    try {
        auto t0 = std::chrono::steady_clock::now();
        Coo coo = read_mtx(path, (MtxFlavor)flavor);
        (void)t0;                                     // like the reference, file parsing is not "Pre-processing Time"
        return add_from_coo(c, coo.rows, coo.cols, (int64_t)coo.r.size(), coo.r.data(), coo.c.data(), coo.v.data());
    } catch (const std::runtime_error& ex) { return fail(c, HISPMV_EIO, ex.what());
    } catch (const std::bad_alloc&) { return fail(c, HISPMV_ENOMEM, "host out of memory");
    } catch (const std::exception& ex) { return fail(c, HISPMV_EINVAL, ex.what()); }
}

HISPMV_API int hispmv_create_sparse_handle_from_csr(hispmv_ctx* c, const int32_t* rp, const int32_t* ci, const float* va,
                                                    int32_t rows, int32_t cols) {
    if (!c) return HISPMV_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    if (rows <= 0 || cols <= 0 || !rp) return fail(c, HISPMV_EINVAL, "bad CSR arguments");
    if (rows >= (1 << 30) || cols >= (1 << 30)) return fail(c, HISPMV_EINVAL, "dimension >= 2^30 is not supported");
    try {
        auto t0 = std::chrono::steady_clock::now();
        Csr csr;
        csr.rows = rows; csr.cols = cols;
        csr.row_ptr.resize((size_t)rows + 1);
        for (int32_t i = 0; i <= rows; ++i) csr.row_ptr[i] = rp[i];
        const int64_t nnz = rp[rows];
        if (rp[0] != 0 || nnz < 0) return fail(c, HISPMV_EINVAL, "row_ptr must start at 0");
        for (int32_t i = 0; i < rows; ++i) if (rp[i + 1] < rp[i]) return fail(c, HISPMV_EINVAL, "row_ptr must be non-decreasing");
        if (nnz > 0 && (!ci || !va)) return fail(c, HISPMV_EINVAL, "col_idx / values are NULL");
        std::vector<float> real;
        if (const int rc = check_sparse_creation(c, nnz)) return rc;
        csr.col.assign(ci, ci + nnz);
        if (c->value_updates) { real.assign(va, va + nnz); const std::vector<float> pl = index_payloads(nnz); csr.val.assign(pl.begin(), pl.end()); }   // input order: before the per-row sort
        else csr.val.assign(va, va + nnz);
        if (c->value_storage == HISPMV_VALUES_BF16 && !c->value_updates) round_values_to_bf16(csr.val.data(), csr.val.data(), nnz);      // (payloads stay whole; the load's update rounds the real values)
        for (int64_t k = 0; k < nnz; ++k) if (ci[k] < 0 || ci[k] >= cols) return fail(c, HISPMV_EINVAL, "CSR column outside matrix");
        std::vector<float>* const real_values = c->value_updates ? &real : nullptr;
        // the stored transpose: the swapped COO in input order -- row_ptr expanded BEFORE the per-row sort, so that entry k is entry k
        // of the value order -- with the values as the packers take them (rounded, or index payloads)
        std::unique_ptr<Matrix> companion;
        const double t_own = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (c->transposable == HISPMV_TRANSPOSABLE_COMPANION) {
            const auto tc = std::chrono::steady_clock::now();
            std::vector<int32_t> entry_rows((size_t)nnz);
            csr_entry_rows(rows, rp, entry_rows.data());
            const std::vector<float> vals(csr.val.begin(), csr.val.end());
            const int rc = make_from_coo(c, cols, rows, nnz, ci, entry_rows.data(), vals.data(), tc, real_values, true, companion);
            if (rc != HISPMV_OK) return rc;
        }
        const auto t1 = std::chrono::steady_clock::now();      // (the companion's time is in its own prep_seconds)
        sort_rows_by_column(csr);     // rows with unsorted columns (scipy: has_sorted_indices == False) are sorted, stably
        double t = std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count() + t_own;
        return register_sparse(c, make_sparse(c, std::move(csr), t, nullptr, real_values, false), std::move(companion), real_values);
    } catch (const std::bad_alloc&) { return fail(c, HISPMV_ENOMEM, "host out of memory");
    } catch (const std::exception& ex) { return fail(c, HISPMV_EINVAL, ex.what()); }
}

HISPMV_API int hispmv_create_dense_handle(hispmv_ctx* c, const float* vals, int32_t rows, int32_t cols) {
    if (!c) return HISPMV_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    if (!c->dense_overlay)   // assert at spmv-helper.cpp:718
        return fail(c, HISPMV_ENOTDENSE, "Hardware is not built with Dense Overlay, cannot support dense workload");
    if (rows <= 0 || cols <= 0 || !vals) return fail(c, HISPMV_EINVAL, "bad dense matrix arguments");
    try {
        auto t0 = std::chrono::steady_clock::now();
        auto m = std::make_unique<Matrix>();
        m->dense = true; m->rows = rows; m->cols = cols; m->nnz = (int64_t)rows * cols;   // spmv-helper.cpp:722
        if (const int rc = check_storage_and_updates(c)) return rc;
        m->value_storage = c->value_storage;
        const bool bf16 = m->value_storage == HISPMV_VALUES_BF16;
        m->device_bytes = m->nnz * (bf16 ? 2 : 4);
        (bf16 ? m->slots_2byte : m->slots_4byte) = m->nnz;
        m->saved_bytes = bf16 ? m->nnz * 2 : 0;
        if (bf16 && c->value_updates) m->dense_host.assign(vals, vals + m->nnz);      // rounded by the load's update (hispmv_update.h), as every later update is
        else if (bf16) {      // W row-major as bf16: the upper halves of R(w)
            m->dense_host16.resize((size_t)m->nnz);
#pragma omp parallel for num_threads(host_threads()) schedule(static)
            for (int64_t k = 0; k < m->nnz; ++k) {
                uint32_t u;
                std::memcpy(&u, vals + k, 4);
                m->dense_host16[(size_t)k] = (uint16_t)(round_bits_to_bf16(u) >> 16);
            }
        } else m->dense_host.assign(vals, vals + m->nnz);
        if (c->value_updates) { m->updatable = true; m->upd_n = m->nnz; m->upd_written = m->nnz; }    // an update is a copy into d_dense
        m->prep_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        return register_handle(c, std::move(m));
    } catch (const std::bad_alloc&) { return fail(c, HISPMV_ENOMEM, "host out of memory"); }
}
