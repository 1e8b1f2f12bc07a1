// hispmv_load.cpp -- hispmv_load_matrices of the C ABI (include/hispmv.h): every prepared handle (hispmv_create.cpp) into device
// memory -- a dense W, the parts of a tile or a slice stream, the merge tables of column parts, the value map -- and the release of
// the host tables.  Every allocation of a load goes through dev_alloc.
#include "hispmv_ctx.h"

using namespace hispmv;

namespace {

// Every device allocation of a load: `count` T's, listed in m.allocs at once -- free_matrix_device releases them, those of a load
// that failed half way too -- and, fill >= 0, set to that byte on c->stream.  count == 0: *out = nullptr, nothing allocated.
template <class T>
int dev_alloc(hispmv_ctx* c, Matrix& m, size_t count, T** out, int fill = -1) {
    *out = nullptr;
    if (count == 0) return HISPMV_OK;
    void* d = nullptr;
    HIP_TRY(c, hipMalloc(&d, count * sizeof(T)));
    m.allocs.push_back(d);
    if (fill >= 0) HIP_TRY(c, hipMemsetAsync(d, fill, count * sizeof(T), c->stream));
    *out = (T*)d;
    return HISPMV_OK;
}
// ... with `host` copied in, asynchronously: `host` lives until the load's synchronise
template <class T>
int upload(hispmv_ctx* c, Matrix& m, const T* host, size_t count, const T** dev_out) {
    T* d = nullptr;
    *dev_out = nullptr;
    if (const int rc = dev_alloc(c, m, count, &d)) return rc;
    if (d) HIP_TRY(c, hipMemcpyAsync(d, host, count * sizeof(T), hipMemcpyHostToDevice, c->stream));
    *dev_out = d;
    return HISPMV_OK;
}

// What a load holds until its stream has drained, released on an error return too: the uploaded host words the device layout reads
// (never in m.allocs) and the headers of the batch layouts (asynchronous copies read them).
struct LoadScratch {
    std::vector<void*> dev;
    std::vector<std::vector<SliceHdr>> hdrs;
    ~LoadScratch() { for (void* p : dev) (void)hipFree(p); }
};

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
        int rc;
        const ValueChunkDev* dt = nullptr;
        if ((rc = dev_alloc(c, m, (size_t)m.map_slots, &m.d_map)) != HISPMV_OK) return rc;
        if ((rc = upload(c, m, tab.data(), tab.size(), &dt)) != HISPMV_OK) return rc;
        m.d_upd_table = const_cast<ValueChunkDev*>(dt);
        if (bf16) {               // the map was read on the host (HostPart::value_map): a half slice holds no payloads
            for (const Matrix::Part& p : m.parts) {
                if (p.value_map.size() != chunks[(size_t)(&p - m.parts.data())].size() * (size_t)kValueChunk) return fail(c, HISPMV_EINVAL, "internal: a part's host value map does not match its chunks");
                if (!p.value_map.empty()) HIP_TRY(c, hipMemcpyAsync(m.d_map + p.map_chunk_base * kValueChunk, p.value_map.data(), p.value_map.size() * 4, hipMemcpyHostToDevice, c->stream));
            }
        } else {
            LAUNCH_TRY(c, launch_build_value_map, m.d_upd_table, (int64_t)tab.size(), m.d_map, c->stream);
        }
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

// A dense W: fp32 or bf16 as created, or -- bf16 with updates -- written by the update kernel from the fp32 creation values
int load_dense(hispmv_ctx* c, Matrix& m) {
    int rc;
    if (m.value_storage == HISPMV_VALUES_BF16 && m.updatable) {
        // W is written by the update kernel from the fp32 creation values, staged in the context's update buffer
        uint16_t* d = nullptr;
        if ((rc = dev_alloc(c, m, (size_t)m.nnz, &d)) != HISPMV_OK) return rc;
        m.d_dense = (float*)d;
        if ((rc = ensure_vec(c, &c->d_upd, &c->cap_d_upd, m.nnz)) != HISPMV_OK) return rc;
        HIP_TRY(c, hipMemcpyAsync(c->d_upd, m.dense_host.data(), (size_t)m.nnz * 4, hipMemcpyHostToDevice, c->stream));
        const hipError_t e = launch_update_dense_bf16(d, c->d_upd, m.nnz, c->stream);
        if (e != hipSuccess) return hip_fail(c, e, "launch_update_dense_bf16");
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    } else if (m.value_storage == HISPMV_VALUES_BF16) {
        const uint16_t* d = nullptr;
        if ((rc = upload(c, m, m.dense_host16.data(), m.dense_host16.size(), &d)) != HISPMV_OK) return rc;
        m.d_dense = (float*)const_cast<uint16_t*>(d);      // (rows x cols bf16: every launch of this handle passes its storage along)
    } else {
        const float* d = nullptr;
        if ((rc = upload(c, m, m.dense_host.data(), m.dense_host.size(), &d)) != HISPMV_OK) return rc;
        m.d_dense = const_cast<float*>(d);
    }
    return HISPMV_OK;
}

// One part of a tile stream; fix_rows: the rows it cut into pieces, in fix list order (load_part_merge)
int load_tile_part(hispmv_ctx* c, Matrix& m, Matrix::Part& p, std::vector<int32_t>& fix_rows) {
    int rc;
    TtsStream& ts = p.tts;
    for (size_t k = 0; k + 3 < ts.fix.size(); k += 4) fix_rows.push_back(ts.fix[k]);
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
        // one set per vector of a batched launch
        if ((rc = dev_alloc(c, m, (size_t)std::max(ts.n_carry, 1) * kTtsMaxVectors, &d.carry, 0)) != HISPMV_OK) return rc;
        d.n_carry = ts.n_carry;
        d.fix = (const int4*)dfix; d.n_fix = (int32_t)(ts.fix.size() / 4);
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
    return HISPMV_OK;
}

}  // namespace
// Device bytes of one layout of a slice part as make_sparse charges them: what upload_slice_layout allocates for {plan, ds} -- the
// slice bytes, the headers, the group table, the fragments and, with stray slots, kStraySlots columns per slice behind the headers.
int64_t hispmv::slice_layout_device_bytes(const SliceStream& st, const LaunchPlan& plan, const DeviceStream& ds) {
    return ds.n_bytes + (int64_t)st.hdr.size() * 16 + (int64_t)ds.groups.size() * 4 + (int64_t)plan.frags.size() * 16 +
           (ds.any_stray ? st.n_slices * (int64_t)kStraySlots * 4 : 0);
}
namespace {
// One layout of a slice part -- its first one, or its batch layout (hispmv_choose.h) -- into d, whose n_slices is set: the group
// table, the fragments, the slices, and the headers in `hdr` with this plan's spill flags.  `hdr` (the part's own, or a copy in
// `scratch`) is copied asynchronously and lives until the load's synchronise.  Counted by slice_layout_device_bytes.
struct SliceLayout { const LaunchPlan& plan; const DeviceStream& ds; const WordVec& words; };
int upload_slice_layout(hispmv_ctx* c, Matrix& m, LoadScratch& scratch, const SliceLayout& l, std::vector<SliceHdr>& hdr, SpmvDeviceMatrix& d) {
    int rc;
    const int64_t ns = d.n_slices;
    const int32_t* dg = nullptr; const Frag* dfr = nullptr; const uint8_t* dw = nullptr;
    if ((rc = upload(c, m, l.ds.groups.data(), l.ds.groups.size(), &dg)) != HISPMV_OK) return rc;
    if ((rc = upload(c, m, l.plan.frags.data(), l.plan.frags.size(), &dfr)) != HISPMV_OK) return rc;
    // the slices in their device layout: packed on the host (HISPMV_LAYOUT=host) or laid out HERE from the uploaded host words
    const bool lay_out = l.ds.bytes.empty() && l.ds.n_bytes > 0;
    uint64_t* d_host_words = nullptr;
    if (!lay_out) {
        if ((rc = upload(c, m, l.ds.bytes.data(), l.ds.bytes.size(), &dw)) != HISPMV_OK) return rc;
    } else {
        if ((int64_t)l.words.size() != ns * kSliceElems) return fail(c, HISPMV_EINVAL, "internal: host words missing for the device layout");
        uint8_t* blk = nullptr;
        if ((rc = dev_alloc(c, m, (size_t)l.ds.n_bytes, &blk)) != HISPMV_OK) return rc;
        dw = blk;
        HIP_TRY(c, hipMalloc((void**)&d_host_words, l.words.size() * sizeof(uint64_t)));
        scratch.dev.push_back(d_host_words);
        HIP_TRY(c, hipMemcpyAsync(d_host_words, l.words.data(), l.words.size() * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    }
    // device header: {row_base, chain_len, rows ending in the slice (load_slice_part), 1 if some of its elements lie outside
    // the group's x window} (the column window of a slice is only needed by the planner)
    for (int64_t sl = 0; sl < ns; ++sl) hdr[(size_t)sl].x_span = (!l.plan.slice_spills.empty() && l.plan.slice_spills[(size_t)sl]) ? 1 : 0;
    // stray slots: the columns of every slice's strays (64 x u32 per slice) live BEHIND the headers in one allocation -- the kernels
    // reach them as hdr + n_slices --, copied when packed on the host, else written by the device layout over 0xffffffff = no stray
    const size_t hb = hdr.size() * sizeof(SliceHdr), sb = l.ds.any_stray ? (size_t)ns * kStraySlots * sizeof(uint32_t) : 0;
    if (sb && !lay_out && l.ds.stray_cols.size() * sizeof(uint32_t) != sb) return fail(c, HISPMV_EINVAL, "internal: stray columns of a host-packed layout do not cover its slices");
    char* blk = nullptr;
    if ((rc = dev_alloc(c, m, hb + sb, &blk)) != HISPMV_OK) return rc;
    if (hb) HIP_TRY(c, hipMemcpyAsync(blk, hdr.data(), hb, hipMemcpyHostToDevice, c->stream));
    if (sb && lay_out) HIP_TRY(c, hipMemsetAsync(blk + hb, 0xff, sb, c->stream));
    else if (sb) HIP_TRY(c, hipMemcpyAsync(blk + hb, l.ds.stray_cols.data(), sb, hipMemcpyHostToDevice, c->stream));
    if (lay_out) {
        const int e = layout_on_device(d_host_words, ns, l.plan.group_slices, dg, l.plan.lds_floats, l.plan.block_threads / 64,
                                       (uint8_t*)dw, sb ? (uint32_t*)(blk + hb) : nullptr, c->stream);
        if (e != 0) return hip_fail(c, (hipError_t)e, "layout_on_device");
    }
    d.words = dw; d.hdr = (const int4*)blk; d.groups = (const int4*)dg; d.frags = (const int4*)dfr;
    d.group_slices = l.plan.group_slices; d.n_groups = (ns + l.plan.group_slices - 1) / l.plan.group_slices;
    d.lds_floats = l.plan.lds_floats + l.ds.stray_floats;        // the x window + the wavefronts' stray areas behind it
    d.has_strays = l.ds.stray_floats > 0;
    d.has_half = l.ds.half_values && l.ds.compact_slices > 0;
    return HISPMV_OK;
}

// carry per slice; {carry, launch tag} granules and the group ticket of the look-back variant
int alloc_carries(hispmv_ctx* c, Matrix& m, SpmvDeviceMatrix& d) {
    int rc;
    const size_t n1 = (size_t)std::max<int64_t>(d.n_slices, 1);
    if ((rc = dev_alloc(c, m, n1 * kMaxBatch, &d.carry, 0)) != HISPMV_OK) return rc;      // one set per vector of a batched pass
    if ((rc = dev_alloc(c, m, n1, &d.gran, 0)) != HISPMV_OK) return rc;
    return dev_alloc(c, m, 1, &d.ticket, 0);
}

// The carry variant of a slice part whose first layout is in d (lds_plain: its slice_lds_bytes): d.lookback, d.use_ticket
void choose_carry_variant(const hispmv_ctx* c, const Matrix& m, SpmvDeviceMatrix& d, size_t lds_plain) {
    const bool mailbox_fits = slice_lds_bytes(d, 1, true) <= kDynLdsMax;
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
    if (d.has_strays) { d.lookback = false; d.use_ticket = false; }
}

// One part of a slice stream: its first layout, fix lists and carries, then its batch layout when it has one
int load_slice_part(hispmv_ctx* c, Matrix& m, Matrix::Part& p, LoadScratch& scratch) {
    int rc;
    const int64_t ns = p.st.n_slices;
    std::vector<SliceHdr>& hh = p.st.hdr;
    int max_rows = 1;
    for (int64_t sl = 0; sl < ns; ++sl) {          // the header's x_base field: rows ending in the slice
        const int nr = (sl + 1 < ns ? hh[sl + 1].row_base : m.rows) - hh[sl].row_base;
        hh[sl].x_base = nr;
        max_rows = std::max(max_rows, nr);
    }
    SpmvDeviceMatrix& d = p.dev;
    d.n_slices = ns; d.rows = m.rows; d.cols = m.cols; d.block_threads = p.plan.block_threads;
    d.err = c->d_err; d.launches = 0; d.ticket_launches = 0;
    if ((rc = upload_slice_layout(c, m, scratch, {p.plan, p.dstream, p.st.words}, hh, d)) != HISPMV_OK) return rc;
    const FixEntry *fs = nullptr, *fl = nullptr;
    if ((rc = upload(c, m, p.fix_short.data(), p.fix_short.size(), &fs)) != HISPMV_OK) return rc;
    if ((rc = upload(c, m, p.fix_long.data(), p.fix_long.size(), &fl)) != HISPMV_OK) return rc;
    d.fix_short = (const int4*)fs; d.fix_long = (const int4*)fl;
    d.n_fix_short = (int32_t)p.fix_short.size(); d.n_fix_long = (int32_t)p.fix_long.size();
    if ((rc = alloc_carries(c, m, d)) != HISPMV_OK) return rc;
    d.ytile_floats = std::min(kSliceElems, (max_rows + 63) & ~63);
    const size_t lds_plain = slice_lds_bytes(d);
    if (lds_plain > kDynLdsMax) return fail(c, HISPMV_EINVAL, "internal: launch plan exceeds the LDS of a CU");
    choose_carry_variant(c, m, d, lds_plain);
    transpose_costs(m, p, d);
    // the batch layout (hispmv_choose.h): its own group table, fragments, slice bytes and headers (the spill flags differ);
    // rows, carries, fix lists and the error word are the part's
    if (p.has_batch_layout) {
        SpmvDeviceMatrix b = d;
        scratch.hdrs.push_back(hh);
        if ((rc = upload_slice_layout(c, m, scratch, {p.batch_plan, p.batch_dstream, p.batch_words}, scratch.hdrs.back(), b)) != HISPMV_OK) return rc;
        b.lookback = false; b.use_ticket = false;
        if (slice_lds_bytes(b) <= kDynLdsMax) { p.batch_dev = b; p.has_batch_dev = true; }
    }
    return HISPMV_OK;
}

// Column parts: the partial vectors of parts t > 0 and, where the merge can apply the fix-ups itself, row -> fix entry of every part
int load_part_merge(hispmv_ctx* c, Matrix& m, const std::vector<std::vector<int32_t>>& tts_fix_rows) {
    int rc;
    if ((rc = dev_alloc(c, m, (m.parts.size() - 1) * (size_t)kMaxBatch * m.rows, &m.d_ypart)) != HISPMV_OK) return rc;
    // (short chains only: a part with a long chain keeps the two-launch tail)
    bool fusable = m.parts.size() <= (size_t)kTailMaxParts;
    for (auto& p : m.parts) fusable = fusable && (p.is_tts || p.fix_long.empty());
    if (!fusable) return HISPMV_OK;
    std::vector<int32_t> of((size_t)m.parts.size() * m.rows, -1);
    for (size_t t = 0; t < m.parts.size(); ++t) {
        int32_t* o = of.data() + t * (size_t)m.rows;
        if (m.parts[t].is_tts) { const std::vector<int32_t>& f = tts_fix_rows[t]; for (size_t k = 0; k < f.size(); ++k) o[f[k]] = (int32_t)k; }
        else for (size_t k = 0; k < m.parts[t].fix_short.size(); ++k) o[m.parts[t].fix_short[k].row] = (int32_t)k;
    }
    const int32_t* d_of = nullptr;
    if ((rc = upload(c, m, of.data(), of.size(), &d_of)) != HISPMV_OK) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));      // (`of` is a local)
    m.d_fix_of_row = const_cast<int32_t*>(d_of);
    return HISPMV_OK;
}

// Uploads one prepared matrix (a handle, or the stored transpose of one) and releases its host tables.
int load_matrix(hispmv_ctx* c, Matrix& m) {
    if (m.loaded) return HISPMV_OK;
    int rc;
    LoadScratch scratch;
    std::vector<std::vector<int32_t>> tts_fix_rows;       // tile streams: the rows cut into pieces, per part (fix list order)
    // value updates: the value regions of every part and the sizes of its layouts, while the host tables exist
    std::vector<std::vector<ValueChunk>> value_regions;
    std::vector<std::pair<int64_t, int64_t>> layout_bytes;
    if (m.updatable && !m.dense)
        for (const Matrix::Part& p : m.parts) {
            value_regions.push_back(value_chunks(p));
            layout_bytes.emplace_back(p.is_tts ? (int64_t)p.tts.words.size() : p.dstream.n_bytes, p.has_batch_layout ? p.batch_dstream.n_bytes : 0);
        }
    if (m.dense) {
        if ((rc = load_dense(c, m)) != HISPMV_OK) return rc;
    } else {
        for (Matrix::Part& p : m.parts) {
            if (m.format == 1) { tts_fix_rows.emplace_back(); rc = load_tile_part(c, m, p, tts_fix_rows.back()); }
            else rc = load_slice_part(c, m, p, scratch);
            if (rc != HISPMV_OK) return rc;
        }
        if (m.parts.size() > 1 && (rc = load_part_merge(c, m, tts_fix_rows)) != HISPMV_OK) return rc;
        if (m.updatable && (rc = load_value_map(c, m, value_regions, layout_bytes)) != HISPMV_OK) return rc;
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    // host copies are no longer needed
    for (auto& p : m.parts) { p.st = SliceStream{}; p.fix_short = {}; p.fix_long = {}; p.plan.groups = {}; p.plan.frags = {}; p.dstream = DeviceStream{};
                              p.batch_plan.groups = {}; p.batch_plan.frags = {}; p.batch_plan.slice_spills = {}; p.batch_dstream = DeviceStream{}; p.batch_words = WordVec(); }
    m.dense_host = {}; m.dense_host16 = {};
    if (m.dense) {          // transposed product of a dense handle: the row blocks add their column sums to y (plain stores when there is one)
        const int nb = gemv_t_row_blocks(m.rows, m.cols);
        m.t_launches = nb > 0 ? 1 : 0;
        m.t_atomic_bytes = nb > 1 ? (int64_t)nb * m.cols * 4 : 0;
    }
    m.t_launches += 1;      // the prologue y = beta * bias (a tile stream reports its figures only when the entries accept it)
    m.loaded = true;
    return HISPMV_OK;
}

}  // namespace

void hispmv::free_matrix_device(Matrix& m) {
    for (void*& p : m.allocs) dev_free(p);
    m.allocs.clear();
    for (auto& p : m.parts) p.dev = SpmvDeviceMatrix{};
    m.d_dense = nullptr; m.d_ypart = nullptr; m.d_fix_of_row = nullptr; m.d_map = nullptr; m.d_upd_table = nullptr;
    m.loaded = false;
    if (m.companion) free_matrix_device(*m.companion);
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
