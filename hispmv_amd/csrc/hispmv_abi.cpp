// hispmv_abi.cpp -- the C ABI of libhispmv.so (include/hispmv.h): context, matrix handles,
// arena accounting, HBM upload and launches.  MI355X counterpart of the reference's
// FpgaHandle (pyhispmv/src/fpga_handle.cpp:40-388), which owns the XRT device, the
// per-channel matrix arena and the kernel run object.  Host-side HIP runtime calls only;
// the kernels live in hispmv_kernels.hip, the preprocessor in hispmv_prep.cpp.
#include "hispmv_ctx.h"

using namespace hispmv;

namespace {

thread_local std::string g_create_err;
thread_local std::string g_prep_err;

}  // namespace

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
}  // namespace hispmv

namespace {

int64_t sparse_device_bytes(const SliceStream& st, const DeviceStream& ds) {
    return ds.n_bytes + (int64_t)st.hdr.size() * 16 + (int64_t)st.fix.size() * 16 +
           (int64_t)st.n_slices * 12 + 8;
}

void free_matrix_device(Matrix& m) {
    for (void*& p : m.allocs) dev_free(p);
    m.allocs.clear();
    for (auto& p : m.parts) p.dev = SpmvDeviceMatrix{};
    m.d_dense = nullptr; m.d_ypart = nullptr; m.d_fix_of_row = nullptr; m.d_map = nullptr; m.d_upd_table = nullptr;
    m.loaded = false;
    if (m.companion) free_matrix_device(*m.companion);
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
            m->device_bytes += sparse_device_bytes(p.st, p.dstream) + (int64_t)p.dstream.groups.size() * 4 + (int64_t)p.plan.frags.size() * 16 + (p.dstream.any_stray ? p.st.n_slices * (int64_t)kStraySlots * 4 : 0);
            m->compact_slices += p.dstream.compact_slices;
            // value slots by size: the slices of half groups hold bf16 values and are kSliceUnit bytes shorter than compact ones
            for (const DeviceStream* ds : {&p.dstream, p.has_batch_layout ? &p.batch_dstream : nullptr}) {
                if (!ds) continue;
                const int64_t half = ds->half_values ? ds->compact_slices : 0;
                m->slots_2byte += half * kSliceElems;
                m->slots_4byte += (p.st.n_slices - half) * kSliceElems;
                m->saved_bytes += half * (kCompactSliceBytes - kHalfSliceBytes);
            }
            if (p.has_batch_layout) m->device_bytes += p.batch_dstream.n_bytes + (int64_t)p.st.hdr.size() * 16 + (int64_t)p.batch_dstream.groups.size() * 4 + (int64_t)p.batch_plan.frags.size() * 16 +
                                                       (p.batch_dstream.any_stray ? p.st.n_slices * (int64_t)kStraySlots * 4 : 0);
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
int register_sparse(hispmv_ctx* c, std::unique_ptr<Matrix> m, std::unique_ptr<Matrix> companion, std::vector<float>* real_values) {
    if (companion) { m->device_bytes += companion->device_bytes; m->prep_seconds += companion->prep_seconds; }
    if (c->arena_used + m->device_bytes > c->arena_budget) return HISPMV_FULL;
    if (real_values && companion) companion->upd_values = *real_values;      // (each load gathers the creation values into its own layouts)
    if (real_values) m->upd_values = std::move(*real_values);
    c->arena_used += m->device_bytes;
    m->index = (int)c->mats.size();
    if (companion) { companion->index = kCompanionId + m->index; m->companion = std::move(companion); }
    c->mats.push_back(std::move(m));
    return (int)c->mats.size() - 1;
}
// Creation in state HISPMV_TRANSPOSABLE_COMPANION: the rule of check_updatable -- the forward launches of a stored transpose are those of
// the standard tile geometry.
int check_companion(hispmv_ctx* c) {
    if (c->transposable == HISPMV_TRANSPOSABLE_COMPANION && (c->format_opts.tts_geometry != 0 || c->format_opts.tts_small))
        return fail(c, HISPMV_EINVAL, "set_transposable(companion): not supported with HISPMV_TTS_GEOMETRY other than standard or HISPMV_TTS_SMALL (experiments)");
    return HISPMV_OK;
}

// The load's part of value updates, once the layouts of `m` are on the device (packed with index payloads): the chunk table, the
// map read out of the layouts, then the real values gathered in -- so the update kernel runs on every load of an updatable handle.
// `chunks`: value_chunks of every part, taken before the loader released the host tables; `layout_bytes`: {first, batch} layout
// sizes per part, every chunk is checked against them before anything is written.
int load_value_map(hispmv_ctx* c, Matrix& m, const std::vector<std::vector<ValueChunk>>& chunks, const std::vector<std::pair<int64_t, int64_t>>& layout_bytes) {
    std::vector<ValueChunkDev> tab;
    int64_t written = 0;
    const bool bf16 = m.value_storage == HISPMV_VALUES_BF16;
    for (size_t t = 0; t < m.parts.size(); ++t) {
        Matrix::Part& p = m.parts[t];
        uint8_t* base0 = p.is_tts ? (uint8_t*)p.tdev.words : (uint8_t*)p.dev.words;
        uint8_t* base1 = (!p.is_tts && p.has_batch_dev) ? (uint8_t*)p.batch_dev.words : nullptr;
        p.map_chunk_base = (int64_t)tab.size();           // (the value gradient reads the map by part and slice: hispmv_value_grad.h)
        for (const ValueChunk& q : chunks[t]) {
            if (q.off0 < 0 || q.off0 + kValueChunk * 4 > layout_bytes[t].first || (base1 && (q.off1 < 0 || q.off1 + kValueChunk * 4 > layout_bytes[t].second)))
                return fail(c, HISPMV_EINVAL, "internal: value region outside its layout");
            ValueChunkDev e;
            e.map_off = (int64_t)tab.size() * kValueChunk | (q.kind0 == kChunkHalfSlice ? kChunkHalf0 : 0) | (base1 && q.kind1 == kChunkHalfSlice ? kChunkHalf1 : 0);
            e.dst0 = (float*)(base0 + q.off0);
            e.dst1 = base1 ? (float*)(base1 + q.off1) : nullptr;
            written += kValueChunk * (e.dst1 ? 2 : 1);
            tab.push_back(e);
        }
    }
    if ((int64_t)tab.size() * kValueChunk != m.map_slots) return fail(c, HISPMV_EINVAL, "internal: value map size changed between creation and load");
    m.upd_written = written;
    if (!tab.empty()) {
        void* dm = nullptr; void* dt = nullptr;
        HIP_TRY(c, hipMalloc(&dm, (size_t)m.map_slots * 4));
        m.allocs.push_back(dm);
        HIP_TRY(c, hipMalloc(&dt, tab.size() * sizeof(ValueChunkDev)));
        m.allocs.push_back(dt);
        m.d_map = (int32_t*)dm; m.d_upd_table = (ValueChunkDev*)dt;
        HIP_TRY(c, hipMemcpyAsync(dt, tab.data(), tab.size() * sizeof(ValueChunkDev), hipMemcpyHostToDevice, c->stream));
        if (bf16) {               // the map was read on the host (HostPart::value_map): a half slice holds no payloads
            for (const Matrix::Part& p : m.parts) {
                if (p.value_map.size() != chunks[(size_t)(&p - m.parts.data())].size() * (size_t)kValueChunk) return fail(c, HISPMV_EINVAL, "internal: a part's host value map does not match its chunks");
                if (!p.value_map.empty()) HIP_TRY(c, hipMemcpyAsync(m.d_map + p.map_chunk_base * kValueChunk, p.value_map.data(), p.value_map.size() * 4, hipMemcpyHostToDevice, c->stream));
            }
        } else {
            LAUNCH_TRY(c, launch_build_value_map, m.d_upd_table, (int64_t)tab.size(), m.d_map, c->stream);
        }
        int rc;
        if ((rc = ensure_vec(c, &c->d_upd, &c->cap_d_upd, m.upd_n)) != HISPMV_OK) return rc;
        if (m.upd_n > 0) HIP_TRY(c, hipMemcpyAsync(c->d_upd, m.upd_values.data(), (size_t)m.upd_n * 4, hipMemcpyHostToDevice, c->stream));
        LAUNCH_TRY_AS(c, "launch_update_values", bf16 ? launch_update_values_bf16(m.d_upd_table, (int64_t)tab.size(), m.d_map, c->d_upd, m.upd_n, c->stream)
                                                      : launch_update_values(m.d_upd_table, (int64_t)tab.size(), m.d_map, c->d_upd, m.upd_n, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));      // (`tab` and the values are host locals / released next)
    }
    for (Matrix::Part& p : m.parts) p.value_map = std::vector<int32_t>();
    m.upd_values = std::vector<float>();
    return HISPMV_OK;
}

template <class T>
int upload(hispmv_ctx* c, Matrix& m, const T* host, size_t count, const T** dev_out) {
    *dev_out = nullptr;
    if (count == 0) return HISPMV_OK;
    void* d = nullptr;
    HIP_TRY(c, hipMalloc(&d, count * sizeof(T)));
    m.allocs.push_back(d);
    HIP_TRY(c, hipMemcpyAsync(d, host, count * sizeof(T), hipMemcpyHostToDevice, c->stream));
    *dev_out = (const T*)d;
    return HISPMV_OK;
}

// What one transposed call (hispmv_spmv_device_t) costs on slice part `p` of `m`, added to the handle's counts while the host
// tables of the plan exist: one launch; the window flush of every staged group (its fragments, clipped to `cols`); one float per
// stray of a stray-slot group; one float per element that adds to y directly -- the elements outside the window of a wide group,
// and every stored slot (fillers included, tail padding not) of a group without fragments or of a plan without a window.
void transpose_costs(Matrix& m, const HostPart& p, const SpmvDeviceMatrix& d) {
    if (d.n_groups <= 0) return;
    m.t_launches += 1;
    const int64_t G = d.group_slices, ns = d.n_slices;
    const int64_t padding = std::max<int64_t>(0, ns * kSliceElems - p.st.n_elems);
    int64_t flushed = 0, strays = 0, direct = 0;
    for (int64_t g = 0; g < d.n_groups; ++g) {
        const GroupDesc gd = (size_t)g < p.plan.groups.size() ? p.plan.groups[(size_t)g] : GroupDesc{0, 0, 0, 0};
        const int32_t gw = (size_t)g * 4 + 3 < p.dstream.groups.size() ? p.dstream.groups[(size_t)g * 4 + 3] : 0;
        const int64_t s0 = g * G, s1 = std::min(ns, s0 + G);
        if (p.plan.lds_floats > 0 && gd.frag_count > 0) {
            for (int32_t f = gd.frag_begin; f < gd.frag_begin + gd.frag_count && (size_t)f < p.plan.frags.size(); ++f)
                flushed += std::max<int64_t>(0, std::min<int64_t>(p.plan.frags[(size_t)f].len, (int64_t)m.cols - p.plan.frags[(size_t)f].col_start));
            if (gw & kGroupStrays) {
                for (int64_t sl = s0; sl < s1 && (size_t)sl < p.plan.slice_spills.size(); ++sl) strays += p.plan.slice_spills[(size_t)sl];
            } else if (!(gw & kGroupCompact)) {
                direct += gd.n_global;
            }
        } else {
            direct += (s1 - s0) * kSliceElems - (s1 == ns ? padding : 0);
        }
    }
    m.t_direct += direct;
    m.t_atomic_bytes += 4 * (flushed + strays + direct);
}

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

}  // namespace

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

HISPMV_API void hispmv_destroy(hispmv_ctx* c);

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

// COO -> prepared matrix, on the device or on the host (hispmv_ctx::prep_mode); `v` as the packers take it (rounded, or index payloads)
static int make_from_coo(hispmv_ctx* c, int32_t rows, int32_t cols, int64_t nnz, const int32_t* r, const int32_t* cl, const float* v,
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
static int add_from_coo(hispmv_ctx* c, int32_t rows, int32_t cols, int64_t nnz, const int32_t* r, const int32_t* cl, const float* v) {
    auto t0 = std::chrono::steady_clock::now();
    std::vector<float> real, payloads, rounded;
    {
        int rc = check_storage_and_updates(c);
        if (rc == HISPMV_OK) rc = check_companion(c);
        if (rc != HISPMV_OK) return rc;
    }
    if (c->value_storage == HISPMV_VALUES_BF16) {      // rounded once, here: the host and the device preprocessor see R(v)
        rounded.resize((size_t)nnz);
        round_values_to_bf16(v, rounded.data(), nnz);
        v = rounded.data();
    }
    if (c->value_updates) {
        const int rc = check_updatable(c, nnz);
        if (rc != HISPMV_OK) return rc;
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
        {
            int rc = check_storage_and_updates(c);
            if (rc == HISPMV_OK) rc = check_companion(c);
            if (rc != HISPMV_OK) return rc;
        }
        if (c->value_updates) {
            const int rc = check_updatable(c, nnz);
            if (rc != HISPMV_OK) return rc;
        }
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
        {
            const int rc = check_storage_and_updates(c);
            if (rc != HISPMV_OK) return rc;
        }
        m->value_storage = c->value_storage;
        const bool bf16 = m->value_storage == HISPMV_VALUES_BF16;
        m->device_bytes = m->nnz * (bf16 ? 2 : 4);
        (bf16 ? m->slots_2byte : m->slots_4byte) = m->nnz;
        m->saved_bytes = bf16 ? m->nnz * 2 : 0;
        if (c->arena_used + m->device_bytes > c->arena_budget) return HISPMV_FULL;
        if (bf16 && c->value_updates) m->dense_host.assign(vals, vals + m->nnz);      // rounded by the load's update (hispmv_update.h), as every later update is
        else if (bf16) {      // W row-major as bf16: the upper halves of R(w)
            m->dense_host16.resize((size_t)m->nnz);
#pragma omp parallel for num_threads(host_threads()) schedule(static)
            for (int64_t k = 0; k < m->nnz; ++k) {
                uint32_t u;
                std::memcpy(&u, vals + k, 4);
                m->dense_host16[(size_t)k] = (uint16_t)(round_bits_to_bf16(u) >> 16);
            }
        } else
        m->dense_host.assign(vals, vals + m->nnz);
        if (c->value_updates) { m->updatable = true; m->upd_n = m->nnz; m->upd_written = m->nnz; }    // an update is a copy into d_dense
        m->prep_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        c->arena_used += m->device_bytes;
        m->index = (int)c->mats.size();
    c->mats.push_back(std::move(m));
        return (int)c->mats.size() - 1;
    } catch (const std::bad_alloc&) { return fail(c, HISPMV_ENOMEM, "host out of memory"); }
}

// Uploads one prepared matrix (a handle, or the stored transpose of one) and releases its host tables.
static int load_matrix(hispmv_ctx* c, Matrix& m) {
    if (m.loaded) return HISPMV_OK;
    int rc;
    // (scratch of the device layout -- the uploaded host words of the parts --, freed once the stream has drained, also on an error return)
    struct Scratch { std::vector<void*> v; void push_back(void* p) { v.push_back(p); } ~Scratch() { for (void* p : v) (void)hipFree(p); } } layout_scratch;
    std::vector<std::vector<int32_t>> tts_fix_rows;       // tile streams: the rows cut into pieces, per part (fix list order)
    // value updates: the value regions of every part and the sizes of its layouts, while the host tables exist
    std::vector<std::vector<ValueChunk>> value_regions;
    std::vector<std::pair<int64_t, int64_t>> layout_bytes;
    if (m.updatable && !m.dense)
        for (const Matrix::Part& p : m.parts) {
            value_regions.push_back(value_chunks(p));
            layout_bytes.emplace_back(p.is_tts ? (int64_t)p.tts.words.size() : p.dstream.n_bytes, p.has_batch_layout ? p.batch_dstream.n_bytes : 0);
        }
    if (m.dense && m.value_storage == HISPMV_VALUES_BF16 && m.updatable) {
        // W is written by the update kernel from the fp32 creation values, staged in the context's update buffer
        void* d = nullptr;
        HIP_TRY(c, hipMalloc(&d, (size_t)m.nnz * 2));
        m.allocs.push_back(d);
        m.d_dense = (float*)d;
        if ((rc = ensure_vec(c, &c->d_upd, &c->cap_d_upd, m.nnz)) != HISPMV_OK) return rc;
        HIP_TRY(c, hipMemcpyAsync(c->d_upd, m.dense_host.data(), (size_t)m.nnz * 4, hipMemcpyHostToDevice, c->stream));
        const hipError_t e = launch_update_dense_bf16((uint16_t*)d, c->d_upd, m.nnz, c->stream);
        if (e != hipSuccess) return hip_fail(c, e, "launch_update_dense_bf16");
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    } else if (m.dense && m.value_storage == HISPMV_VALUES_BF16) {
        const uint16_t* d = nullptr;
        if ((rc = upload(c, m, m.dense_host16.data(), m.dense_host16.size(), &d)) != HISPMV_OK) return rc;
        m.d_dense = (float*)const_cast<uint16_t*>(d);      // (rows x cols bf16: every launch of this handle passes its storage along)
    } else if (m.dense) {
        const float* d = nullptr;
        if ((rc = upload(c, m, m.dense_host.data(), m.dense_host.size(), &d)) != HISPMV_OK) return rc;
        m.d_dense = const_cast<float*>(d);
    } else if (m.format == 1) {
      for (Matrix::Part& p : m.parts) {
        TtsStream& ts = p.tts;
        tts_fix_rows.emplace_back();
        for (size_t k = 0; k + 3 < ts.fix.size(); k += 4) tts_fix_rows.back().push_back(ts.fix[k]);
        const uint8_t* dw = nullptr; const int32_t* dcb = nullptr; const uint16_t* dfl = nullptr; const int32_t* dci = nullptr;
        const TtsTile* dt = nullptr; const TtsBlock* db = nullptr;
        if ((rc = upload(c, m, ts.words.data(), ts.words.size(), &dw)) != HISPMV_OK) return rc;
        if ((rc = upload(c, m, ts.col_base.data(), ts.col_base.size(), &dcb)) != HISPMV_OK) return rc;
        if ((rc = upload(c, m, ts.flags.data(), ts.flags.size(), &dfl)) != HISPMV_OK) return rc;
        const uint16_t* dfh = nullptr;
        std::vector<uint32_t> planes;          // gap-coded row ends: both planes of the codes in one word per lane and chunk
        if (!ts.flags_hi.empty()) {
            planes.resize(ts.flags.size());
            for (size_t q = 0; q < planes.size(); ++q) planes[q] = (uint32_t)ts.flags[q] | ((uint32_t)ts.flags_hi[q] << 16);
            const uint32_t* dp = nullptr;
            if ((rc = upload(c, m, planes.data(), planes.size(), &dp)) != HISPMV_OK) return rc;
            HIP_TRY(c, hipStreamSynchronize(c->stream));      // (`planes` is a local)
            dfh = (const uint16_t*)dp;
        }
        if ((rc = upload(c, m, ts.chunk_info.data(), ts.chunk_info.size(), &dci)) != HISPMV_OK) return rc;
        if ((rc = upload(c, m, ts.tiles.data(), ts.tiles.size(), &dt)) != HISPMV_OK) return rc;
        if ((rc = upload(c, m, ts.blocks.data(), ts.blocks.size(), &db)) != HISPMV_OK) return rc;
        TtsDeviceMatrix& d = p.tdev;
        d.words = dw; d.col_base = dcb; d.flags = dfl; d.flags_hi = dfh; d.chunk_info = (const int2*)dci; d.tiles = (const int4*)dt; d.blocks = (const int4*)db;
        d.n_tiles = (int32_t)ts.tiles.size(); d.rows = m.rows; d.cols = m.cols;
        if (!ts.fix.empty()) {       // rows cut into pieces: carry slots + the slice stream's fix-up entries
            const int32_t* dfix = nullptr;
            if ((rc = upload(c, m, ts.fix.data(), ts.fix.size(), &dfix)) != HISPMV_OK) return rc;
            void* carry = nullptr;
            HIP_TRY(c, hipMalloc(&carry, (size_t)std::max(ts.n_carry, 1) * kTtsMaxVectors * sizeof(float)));      // one set per vector of a batched launch
            m.allocs.push_back(carry);
            HIP_TRY(c, hipMemsetAsync(carry, 0, (size_t)std::max(ts.n_carry, 1) * kTtsMaxVectors * sizeof(float), c->stream));
            d.n_carry = ts.n_carry;
            d.fix = (const int4*)dfix; d.n_fix = (int32_t)(ts.fix.size() / 4); d.carry = (float*)carry;
            // (the same three fields where the multi-matrix fix-up launch looks for them)
            p.dev.fix_short = d.fix; p.dev.n_fix_short = d.n_fix; p.dev.carry = d.carry; p.dev.n_fix_long = 0;
        }
        d.acc_floats = (ts.max_rows + 63) & ~63; d.threads = ts.geometry.threads;
        d.zero_fill = ts.geometry.zero_fill ? 1 : ts.geometry.gap_rows ? 2 : 0;
        d.staging_floats = ts.geometry.max_slots + 64;        // (the dummy slot of padding words sits behind the last real one)
        d.batch_stage_floats = ((ts.max_slots + kTtsChunk - 1) / kTtsChunk) * kTtsChunk + 64;
        // x in the LDS for short x (HISPMV_TTS_XLDS=1; off by default -- measured slower on the 1024 x 8192 layer of
        // apps/model_test.py: 16.7 against 15.1 us alone, 8 vectors 74 against 58 us: that layer's tiles are latency chains
        // of 8 K elements, not gather-bound)
        d.xlds_floats = (m.cols <= kTtsXldsMax && std::getenv("HISPMV_TTS_XLDS")) ? ((m.cols + 63) & ~63) : 0;
        if (tts_tile_lds_bytes(d) > kDynLdsMax) return fail(c, HISPMV_EINVAL, "internal: tile stream exceeds the LDS of a CU");
        // a transposed call (hispmv_tts_transpose.h): one launch, one float atomic per stored word that is neither filler nor padding
        // (an upper bound: explicit zeros among them add nothing at run time)
        m.t_launches += 1; m.t_direct += ts.nnz; m.t_atomic_bytes += 4 * ts.nnz;
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        p.tts = TtsStream{};
      }
    } else {
        for (auto& p : m.parts) {
            const uint8_t* dw = nullptr; const SliceHdr* dh = nullptr; const FixEntry *fs = nullptr, *fl = nullptr;
            const int32_t* dg = nullptr; const Frag* dfr = nullptr;
            const int64_t ns = p.st.n_slices;
            if ((rc = upload(c, m, p.dstream.groups.data(), p.dstream.groups.size(), &dg)) != HISPMV_OK) return rc;
            if ((rc = upload(c, m, p.plan.frags.data(), p.plan.frags.size(), &dfr)) != HISPMV_OK) return rc;
            // the slices in their device layout: packed on the host (HISPMV_LAYOUT=host) or laid out HERE from the uploaded host words
            const bool lay_out = p.dstream.bytes.empty() && p.dstream.n_bytes > 0;
            uint64_t* d_host_words = nullptr;
            if (!lay_out) {
                if ((rc = upload(c, m, p.dstream.bytes.data(), p.dstream.bytes.size(), &dw)) != HISPMV_OK) return rc;
            } else {
                if ((int64_t)p.st.words.size() != ns * kSliceElems) return fail(c, HISPMV_EINVAL, "internal: host words missing for the device layout");
                void* blk = nullptr;
                HIP_TRY(c, hipMalloc(&blk, (size_t)p.dstream.n_bytes));
                m.allocs.push_back(blk);
                dw = (const uint8_t*)blk;
                HIP_TRY(c, hipMalloc((void**)&d_host_words, p.st.words.size() * sizeof(uint64_t)));
                layout_scratch.push_back(d_host_words);
                HIP_TRY(c, hipMemcpyAsync(d_host_words, p.st.words.data(), p.st.words.size() * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
            }
            // device header: {row_base, chain_len, rows ending in the slice, 1 if some of its elements lie outside
            // the group's x window} (the column window of a slice is only needed by the planner)
            std::vector<SliceHdr>& hh = p.st.hdr;
            int max_rows = 1;
            for (int64_t sl = 0; sl < ns; ++sl) {
                const int nr = (sl + 1 < ns ? hh[sl + 1].row_base : m.rows) - hh[sl].row_base;
                hh[sl].x_base = nr;
                hh[sl].x_span = (!p.plan.slice_spills.empty() && p.plan.slice_spills[(size_t)sl]) ? 1 : 0;
                max_rows = std::max(max_rows, nr);
            }
            uint32_t* d_stray_cols = nullptr;
            if (!p.dstream.any_stray) {
                if ((rc = upload(c, m, hh.data(), hh.size(), &dh)) != HISPMV_OK) return rc;
            } else if (lay_out) {
                void* blk = nullptr;
                const size_t hb = hh.size() * sizeof(SliceHdr), sb = (size_t)ns * kStraySlots * sizeof(uint32_t);
                HIP_TRY(c, hipMalloc(&blk, hb + sb));
                m.allocs.push_back(blk);
                HIP_TRY(c, hipMemcpyAsync(blk, hh.data(), hb, hipMemcpyHostToDevice, c->stream));
                HIP_TRY(c, hipMemsetAsync((char*)blk + hb, 0xff, sb, c->stream));        // 0xffffffff = no stray
                dh = (const SliceHdr*)blk;
                d_stray_cols = (uint32_t*)((char*)blk + hb);
            } else {
                // stray slots: the columns of every slice's strays (64 x u32 per slice) live BEHIND the headers in one
                // allocation -- the kernels reach them as hdr + n_slices, no further pointer to carry around
                void* blk = nullptr;
                const size_t hb = hh.size() * sizeof(SliceHdr), sb = p.dstream.stray_cols.size() * sizeof(uint32_t);
                HIP_TRY(c, hipMalloc(&blk, hb + sb));
                m.allocs.push_back(blk);
                HIP_TRY(c, hipMemcpyAsync(blk, hh.data(), hb, hipMemcpyHostToDevice, c->stream));
                HIP_TRY(c, hipMemcpyAsync((char*)blk + hb, p.dstream.stray_cols.data(), sb, hipMemcpyHostToDevice, c->stream));
                dh = (const SliceHdr*)blk;
            }
            if (lay_out) {
                const int e = layout_on_device(d_host_words, ns, p.plan.group_slices, dg, p.plan.lds_floats, p.plan.block_threads / 64,
                                               (uint8_t*)dw, d_stray_cols, c->stream);
                if (e != 0) return hip_fail(c, (hipError_t)e, "layout_on_device");
            }
            if ((rc = upload(c, m, p.fix_short.data(), p.fix_short.size(), &fs)) != HISPMV_OK) return rc;
            if ((rc = upload(c, m, p.fix_long.data(), p.fix_long.size(), &fl)) != HISPMV_OK) return rc;
            // carry per slice; {carry, launch tag} granules and the group ticket of the look-back variant
            void *carry = nullptr, *gran = nullptr, *ticket = nullptr;
            const size_t n1 = (size_t)std::max<int64_t>(ns, 1);
            HIP_TRY(c, hipMalloc(&carry, n1 * kMaxBatch * sizeof(float)));      // one set per vector of a batched pass
            m.allocs.push_back(carry);
            HIP_TRY(c, hipMemsetAsync(carry, 0, n1 * kMaxBatch * sizeof(float), c->stream));
            HIP_TRY(c, hipMalloc(&gran, n1 * sizeof(unsigned long long)));
            m.allocs.push_back(gran);
            HIP_TRY(c, hipMemsetAsync(gran, 0, n1 * sizeof(unsigned long long), c->stream));
            HIP_TRY(c, hipMalloc(&ticket, sizeof(unsigned long long)));
            m.allocs.push_back(ticket);
            HIP_TRY(c, hipMemsetAsync(ticket, 0, sizeof(unsigned long long), c->stream));
            SpmvDeviceMatrix& d = p.dev;
            d.words = dw; d.hdr = (const int4*)dh; d.groups = (const int4*)dg; d.frags = (const int4*)dfr;
            d.fix_short = (const int4*)fs; d.fix_long = (const int4*)fl;
            d.carry = (float*)carry; d.gran = (unsigned long long*)gran; d.ticket = (unsigned long long*)ticket;
            d.err = c->d_err; d.launches = 0; d.ticket_launches = 0;
            d.n_slices = ns; d.n_groups = (ns + p.plan.group_slices - 1) / p.plan.group_slices;
            d.group_slices = p.plan.group_slices; d.block_threads = p.plan.block_threads;
            d.lds_floats = p.plan.lds_floats + p.dstream.stray_floats;        // the x window + the wavefronts' stray areas behind it
            d.ytile_floats = std::min(kSliceElems, (max_rows + 63) & ~63);
            const size_t lds_plain = slice_lds_bytes(d);
            if (lds_plain > kDynLdsMax) return fail(c, HISPMV_EINVAL, "internal: launch plan exceeds the LDS of a CU");
            const bool mailbox_fits = slice_lds_bytes(d, 1, true) <= kDynLdsMax;
            d.n_fix_short = (int32_t)p.fix_short.size(); d.n_fix_long = (int32_t)p.fix_long.size();
            d.rows = m.rows; d.cols = m.cols;
            // co-residency of the whole grid: workgroups per CU by LDS and waves (conservative: <= 4 blocks,
            // <= 16 waves per CU; MI355X_MICROARCH.md "Residency")
            const int lds_b = std::max(1, (int)lds_plain + 64);
            const int per_cu = std::max(1, std::min({4, kLdsPerCu / lds_b, 16 / (d.block_threads / 64)}));
            const bool resident = d.n_groups <= (int64_t)c->n_cus * per_cu;
            const bool one_round = d.group_slices <= d.block_threads / 64;
            // carry_mode: 0 fix-up launch; 1 look-back for every plan, workgroups in blockIdx order (relies on the
            // dispatcher starting workgroups in increasing id order -- observed, not contractual; the wait is
            // bounded and reports instead of hanging); 3 the same with start-order tickets (contract-safe);
            // 2 (auto) look-back when the whole grid is co-resident (every workgroup is running, so waiting for an
            // earlier slice cannot deadlock) AND every wavefront has one slice (small matrices, where the second
            // launch costs as much as the kernel), fix-up otherwise; 5 ("resident") look-back for every co-resident
            // grid: correct, but measured slower than main kernel + fix-up launch on the large matrices
            // (PFlow_742 71.6 vs 65.2 us, TSOPF 35.5 vs 33.6: wavefronts that run ahead wait for slower neighbours)
            d.lookback = (c->carry_mode == 1 || c->carry_mode == 3 || (c->carry_mode == 2 && resident && one_round) ||
                          (c->carry_mode == 5 && resident)) && mailbox_fits;
            d.use_ticket = c->carry_mode == 3;
            if (m.parts.size() > 1) { d.lookback = false; d.use_ticket = false; }      // column tiles share one grid: fix-up launch
            // stray slots: the packer placed every slice's strays by the slice's position in the ROTATED walk of the fix-up
            // variant; the look-back variant walks its groups in slice order
            d.has_strays = p.dstream.stray_floats > 0;
            d.has_half = p.dstream.half_values && p.dstream.compact_slices > 0;
            if (d.has_strays) { d.lookback = false; d.use_ticket = false; }
            transpose_costs(m, p, d);
            // the batch layout (hispmv_choose.h): its own group table, fragments, slice bytes and headers (the spill flags differ);
            // rows, carries, fix lists and the error word are the part's
            if (p.has_batch_layout) {
                SpmvDeviceMatrix b = d;
                const int32_t* bg = nullptr; const Frag* bf = nullptr; const uint8_t* bw = nullptr; const SliceHdr* bh = nullptr;
                if ((rc = upload(c, m, p.batch_dstream.groups.data(), p.batch_dstream.groups.size(), &bg)) != HISPMV_OK) return rc;
                if ((rc = upload(c, m, p.batch_plan.frags.data(), p.batch_plan.frags.size(), &bf)) != HISPMV_OK) return rc;
                std::vector<SliceHdr> bhh = hh;
                for (int64_t sl = 0; sl < ns; ++sl) bhh[(size_t)sl].x_span = (!p.batch_plan.slice_spills.empty() && p.batch_plan.slice_spills[(size_t)sl]) ? 1 : 0;
                uint32_t* b_stray = nullptr;
                {
                    void* blk = nullptr;
                    const size_t hb = bhh.size() * sizeof(SliceHdr), sb = p.batch_dstream.any_stray ? (size_t)ns * kStraySlots * sizeof(uint32_t) : 0;
                    HIP_TRY(c, hipMalloc(&blk, hb + sb));
                    m.allocs.push_back(blk);
                    HIP_TRY(c, hipMemcpy(blk, bhh.data(), hb, hipMemcpyHostToDevice));            // (`bhh` is a local: synchronous)
                    if (sb && !p.batch_dstream.stray_cols.empty()) HIP_TRY(c, hipMemcpy((char*)blk + hb, p.batch_dstream.stray_cols.data(), sb, hipMemcpyHostToDevice));
                    else if (sb) HIP_TRY(c, hipMemsetAsync((char*)blk + hb, 0xff, sb, c->stream));
                    bh = (const SliceHdr*)blk;
                    b_stray = sb ? (uint32_t*)((char*)blk + hb) : nullptr;
                }
                if (!p.batch_dstream.bytes.empty()) {
                    if ((rc = upload(c, m, p.batch_dstream.bytes.data(), p.batch_dstream.bytes.size(), &bw)) != HISPMV_OK) return rc;
                } else {
                    void* blk = nullptr; uint64_t* tmp = nullptr;
                    HIP_TRY(c, hipMalloc(&blk, (size_t)p.batch_dstream.n_bytes));
                    m.allocs.push_back(blk);
                    bw = (const uint8_t*)blk;
                    HIP_TRY(c, hipMalloc((void**)&tmp, p.batch_words.size() * sizeof(uint64_t)));
                    layout_scratch.push_back(tmp);
                    HIP_TRY(c, hipMemcpyAsync(tmp, p.batch_words.data(), p.batch_words.size() * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
                    const int e = layout_on_device(tmp, ns, p.batch_plan.group_slices, bg, p.batch_plan.lds_floats, p.batch_plan.block_threads / 64, (uint8_t*)blk, b_stray, c->stream);
                    if (e != 0) return hip_fail(c, (hipError_t)e, "layout_on_device");
                }
                b.words = bw; b.hdr = (const int4*)bh; b.groups = (const int4*)bg; b.frags = (const int4*)bf;
                b.group_slices = p.batch_plan.group_slices; b.n_groups = (ns + p.batch_plan.group_slices - 1) / p.batch_plan.group_slices;
                b.lds_floats = p.batch_plan.lds_floats + p.batch_dstream.stray_floats;
                b.has_strays = p.batch_dstream.stray_floats > 0;
                b.has_half = p.batch_dstream.half_values && p.batch_dstream.compact_slices > 0;
                b.lookback = false; b.use_ticket = false;
                if (slice_lds_bytes(b) <= kDynLdsMax) { p.batch_dev = b; p.has_batch_dev = true; }
            }
        }
    }
    if (!m.dense && m.parts.size() > 1) {
        void* yp = nullptr;
        HIP_TRY(c, hipMalloc(&yp, (m.parts.size() - 1) * (size_t)kMaxBatch * m.rows * sizeof(float)));
        m.allocs.push_back(yp);
        m.d_ypart = (float*)yp;
        // row -> fix entry of every part (short chains only: a part with a long chain keeps the two-launch tail)
        bool fusable = m.parts.size() <= (size_t)kTailMaxParts;
        for (auto& p : m.parts) fusable = fusable && (p.is_tts || p.fix_long.empty());
        if (fusable) {
            std::vector<int32_t> of((size_t)m.parts.size() * m.rows, -1);
            for (size_t t = 0; t < m.parts.size(); ++t) {
                int32_t* o = of.data() + t * (size_t)m.rows;
                if (m.parts[t].is_tts) { const std::vector<int32_t>& f = tts_fix_rows[t]; for (size_t k = 0; k < f.size(); ++k) o[f[k]] = (int32_t)k; }
                else for (size_t k = 0; k < m.parts[t].fix_short.size(); ++k) o[m.parts[t].fix_short[k].row] = (int32_t)k;
            }
            const int32_t* d_of = nullptr;
            if ((rc = upload(c, m, of.data(), of.size(), &d_of)) != HISPMV_OK) return rc;
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            m.d_fix_of_row = const_cast<int32_t*>(d_of);
        }
    }
    if (m.updatable && !m.dense && (rc = load_value_map(c, m, value_regions, layout_bytes)) != HISPMV_OK) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    // host copies are no longer needed
    for (auto& p : m.parts) { p.st = SliceStream{}; p.fix_short = {}; p.fix_long = {}; p.plan.groups = {}; p.plan.frags = {}; p.dstream = DeviceStream{};
                              p.batch_plan.groups = {}; p.batch_plan.frags = {}; p.batch_plan.slice_spills = {}; p.batch_dstream = DeviceStream{}; p.batch_words = WordVec(); }
    m.dense_host = {};
    m.dense_host16 = {};
    if (m.dense) {          // transposed product of a dense handle: the row blocks add their column sums to y (plain stores when there is one)
        const int nb = gemv_t_row_blocks(m.rows, m.cols);
        m.t_launches = nb > 0 ? 1 : 0;
        m.t_atomic_bytes = nb > 1 ? (int64_t)nb * m.cols * 4 : 0;
    }
    m.t_launches += 1;      // the prologue y = beta * bias (a tile stream reports its figures only when the entries accept it)
    m.loaded = true;
    return HISPMV_OK;
}

HISPMV_API int hispmv_load_matrices(hispmv_ctx* c) {
    if (!c) return HISPMV_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    HIP_TRY(c, hipSetDevice(c->device));
    for (auto& mp : c->mats) {
        int rc;
        // the stored transpose first: its owner counts as loaded only with it
        if (mp->companion && (rc = load_matrix(c, *mp->companion)) != HISPMV_OK) return rc;
        if ((rc = load_matrix(c, *mp)) != HISPMV_OK) return rc;
    }
    return HISPMV_OK;
}

HISPMV_API int hispmv_select_matrix(hispmv_ctx* c, uint32_t idx) {
    if (!c) return HISPMV_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    if (idx >= c->mats.size()) return idx_out_of_range(c);
    c->selected = (int)idx;
    return HISPMV_OK;
}

static int run_host_vectors(hispmv_ctx* c, Matrix& m, const float* x, int64_t num_vecs, const float* bias,
                            float* y, float alpha, float beta, bool is_linear) {
    HIP_TRY(c, hipSetDevice(c->device));
    int rc;
    // device side: [x (num_vecs * cols) | bias (rows)] in one block, y in another
    const int64_t nx = (((int64_t)m.cols * num_vecs + 63) / 64) * 64, nb = m.rows, ny = (int64_t)m.rows * num_vecs;
    if ((rc = ensure_vec(c, &c->d_x, &c->cap_x, nx + nb)) != HISPMV_OK) return rc;
    if ((rc = ensure_vec(c, &c->d_y, &c->cap_y, ny)) != HISPMV_OK) return rc;
    float* const d_x = c->d_x;
    float* const d_bias = c->d_x + nx;
    const size_t bx = (size_t)m.cols * num_vecs * sizeof(float), bb = (size_t)nb * sizeof(float), by = (size_t)ny * sizeof(float);
    const bool staged = (nx + nb + ny) * (int64_t)sizeof(float) <= (8 << 20);     // small vectors: through pinned memory
    if (staged) {
        if (nx + nb + ny > c->cap_stage) {
            host_free(c->h_stage);      // (the staging block only; the batch tables are not touched by this path)
            c->cap_stage = 0;
            const int64_t want = std::max<int64_t>(nx + nb + ny, 1 << 16);
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
        } else
            HIP_TRY(c, hipMemcpyAsync(d_x, c->h_stage, beta != 0.0f ? (size_t)nx * sizeof(float) + bb : bx, hipMemcpyHostToDevice, c->stream));
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

// ---- transposed product (include/hispmv.h: hispmv_spmv_device_t; kernels: hispmv_transpose.hip) ---------------------------------
HISPMV_API int hispmv_set_transposable(hispmv_ctx* c, int enable) {
    if (!c) return HISPMV_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    if (enable != HISPMV_TRANSPOSABLE_OFF && enable != HISPMV_TRANSPOSABLE_SLICES && enable != HISPMV_TRANSPOSABLE_KEEP_FORMAT && enable != HISPMV_TRANSPOSABLE_COMPANION)
        return fail(c, HISPMV_EINVAL, "set_transposable: unknown state (HISPMV_TRANSPOSABLE_OFF, _SLICES, _KEEP_FORMAT or _COMPANION)");
    c->transposable = enable;
    return HISPMV_OK;
}

namespace hispmv {          // (declared in hispmv_ctx.h: hispmv_krylov_abi.cpp refuses what hispmv_spmv_device_t refuses)

// A tile-stream handle the transposed and gradient entries accept (hispmv_tts_transpose.h): created in state _KEEP_FORMAT, one part,
// stream words for every row -- the standard and the small geometry.
bool tts_transposable(const Matrix& m) {
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

}  // namespace

HISPMV_API int hispmv_companion_info(const hispmv_ctx* c, int idx, int64_t out[6]) {
    if (!c || !out || idx < 0 || idx >= (int)c->mats.size()) return HISPMV_EINVAL;
    for (int i = 0; i < 6; ++i) out[i] = 0;
    const Matrix* t = c->mats[(size_t)idx]->companion.get();
    if (!t) return HISPMV_OK;
    out[0] = 1; out[1] = t->format; out[2] = (int64_t)t->parts.size(); out[3] = t->device_bytes; out[4] = t->map_slots;
    out[5] = t->parts.size() > 1 ? (t->tile_kind ? t->tile_kind : 1) : 0;
    return HISPMV_OK;
}

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
    if (m.companion) return launch_companion(c, m, 1, d_x, d_bias, 0, d_y, alpha, beta, s);
    // y = beta * bias first, then every part of the matrix adds alpha * A_t^T * x into it: no partial vectors, no merge
    LAUNCH_TRY(c, launch_transpose_prologue, d_bias, d_y, m.cols, beta, s);
    if (alpha == 0.0f) return HISPMV_OK;          // y is exactly beta * bias
    if (m.dense) LAUNCH_TRY(c, launch_gemv_t, m.d_dense, m.rows, m.cols, m.value_storage == HISPMV_VALUES_BF16, d_x, d_y, alpha, s);
    else if (m.format == 1) LAUNCH_TRY(c, launch_tts_t, m.parts[0].tdev, 1, d_x, d_y, alpha, s);      // an accepted tile stream: one launch, no carries, no fix-up
    else for (auto& p : m.parts) LAUNCH_TRY(c, launch_spmv_t, p.dev, d_x, d_y, alpha, s);
    return HISPMV_OK;
}

// ---- several vectors on device pointers (include/hispmv.h: hispmv_linear_device, hispmv_linear_device_t) ---------------------------
namespace {

// The checks both entries share, all before any device call; on success *out is the handle.  in_len / out_len: floats per vector.
int linear_device_target(hispmv_ctx* c, int idx, const float* d_x, int64_t num_vecs, const float* d_bias, const float* d_y, float beta,
                         const char* who, Matrix** out) {
    if (const int rc = find_handle(c, idx, who, out)) return rc;
    const Matrix& m = **out;
    if (num_vecs < 1) return fail(c, HISPMV_EINVAL, std::string(who) + ": num_vecs must be at least 1");
    if (!d_x || !d_y || (beta != 0.0f && !d_bias)) return fail(c, HISPMV_EINVAL, "NULL device vector");
    if (d_x == d_y) return fail(c, HISPMV_EINVAL, std::string(who) + ": x and y must not be the same vectors");
    if ((int64_t)m.rows * num_vecs >= (1LL << 30) || (int64_t)m.cols * num_vecs >= (1LL << 30))
        return fail(c, HISPMV_EINVAL, std::string(who) + ": rows * num_vecs and cols * num_vecs must stay below 2^30 floats; split the batch");
    return HISPMV_OK;
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

}  // namespace

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
    if (m.companion) return launch_companion(c, m, num_vecs, d_x, d_bias, bias_stride, d_y, alpha, beta, s);
    // ONE prologue for all vectors, then passes of the widest width that fits (4, 2, 1; dense 8, 4, 2, 1)
    LAUNCH_TRY(c, launch_transpose_prologue, d_bias, d_y, m.cols, beta, s, num_vecs, bias_stride);
    if (alpha == 0.0f) return HISPMV_OK;          // y is exactly beta * bias, per vector
    for (int64_t k = 0; k < num_vecs;) {
        const int nv = transposed_width(m, num_vecs - k);
        const float* xk = d_x + k * m.rows;
        float* yk = d_y + k * m.cols;
        // (a pass of several vectors reports under the one-vector launcher's name)
        if (m.dense) {
            LAUNCH_TRY_AS(c, "launch_gemv_t", nv == 1 ? launch_gemv_t(m.d_dense, m.rows, m.cols, m.value_storage == HISPMV_VALUES_BF16, xk, yk, alpha, s)
                                                   : launch_gemv_t_nv(m.d_dense, m.rows, m.cols, m.value_storage == HISPMV_VALUES_BF16, nv, xk, yk, alpha, s));
        } else if (m.format == 1) {
            LAUNCH_TRY(c, launch_tts_t, m.parts[0].tdev, nv, xk, yk, alpha, s);
        } else {
            for (auto& p : m.parts) LAUNCH_TRY_AS(c, "launch_spmv_t", nv == 1 ? launch_spmv_t(p.dev, xk, yk, alpha, s) : launch_spmv_t_nv(p.dev, nv, xk, yk, alpha, s));
        }
        k += nv;
    }
    return HISPMV_OK;
}

// ---- value gradient (include/hispmv.h: hispmv_value_grad_device; kernels: hispmv_value_grad.hip) ---------------------------------
namespace {

// the entry accepts the handle: loaded, updatable (so it has a map, or is dense), and a slice stream or an accepted tile stream
bool value_grad_accepts(const Matrix& m) {
    if (!m.loaded || !m.updatable) return false;
    if (m.dense) return true;
    if (m.format != 0) return tts_transposable(m);
    for (auto& p : m.parts)
        if (p.is_tts) return false;
    return true;
}

}  // namespace

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
    if ((int64_t)m.rows * num_vecs >= (1LL << 30) || (int64_t)m.cols * num_vecs >= (1LL << 30))
        return fail(c, HISPMV_EINVAL, "value_grad_device: rows * num_vecs and cols * num_vecs must stay below 2^30 floats; split the batch");
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

// ---- bf16 value storage (include/hispmv.h: hispmv_set_value_storage) ----------------------------------------------------------
HISPMV_API int hispmv_set_value_storage(hispmv_ctx* c, int storage) {
    if (!c) return HISPMV_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    if (storage != HISPMV_VALUES_FP32 && storage != HISPMV_VALUES_BF16) return fail(c, HISPMV_EINVAL, "unknown value storage (HISPMV_VALUES_FP32 or HISPMV_VALUES_BF16)");
    c->value_storage = storage;
    return HISPMV_OK;
}
HISPMV_API int hispmv_value_storage_info(const hispmv_ctx* c, int idx, int64_t out[4]) {
    if (!c || !out || idx < 0 || idx >= (int)c->mats.size()) return HISPMV_EINVAL;
    const Matrix& m = *c->mats[(size_t)idx];
    out[0] = m.value_storage; out[1] = m.slots_2byte; out[2] = m.slots_4byte; out[3] = m.saved_bytes;
    return HISPMV_OK;
}

// ---- in-place value updates (include/hispmv.h: hispmv_set_value_updates) ----------------------------------------------------
HISPMV_API int hispmv_set_value_updates(hispmv_ctx* c, int enable) {
    if (!c) return HISPMV_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    c->value_updates = enable != 0;          // (any value but 0 and _ANY_STORAGE is _ON, as before the third state existed)
    c->updates_any_storage = enable == HISPMV_VALUE_UPDATES_ANY_STORAGE;
    return HISPMV_OK;
}

HISPMV_API int hispmv_value_update_info(const hispmv_ctx* c, int idx, int64_t out[4]) {
    if (!c || !out || idx < 0 || idx >= (int)c->mats.size()) return HISPMV_EINVAL;
    const Matrix& m = *c->mats[idx];
    out[0] = m.updatable ? 1 : 0; out[1] = m.upd_n; out[2] = m.map_slots; out[3] = m.upd_written + (m.companion ? m.companion->upd_written : 0);
    return HISPMV_OK;
}

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
