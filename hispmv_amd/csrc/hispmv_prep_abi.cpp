// hispmv_prep_abi.cpp -- the host-only hispmv_prep_* entry points of include/hispmv.h: the preprocessor, the launch planner, the
// format / tiling choice and the tile-stream packer without a device, for tests on a CPU-only box.  Mirrors
// HiSpmvHandle::getPreparedMtx (common/src/spmv-helper.cpp:800-802).  (hispmv_prep_from_coo_device is the one entry here that
// touches the GPU.)
#include "hispmv_block_jacobi.h"
#include "hispmv_ctx.h"
#include "hispmv_gmres.h"

using namespace hispmv;

#define g_prep_err (::hispmv::prep_error())

// ---- host-only preprocessor access ---------------------------------------------------------------
HISPMV_API const char* hispmv_prep_last_error(void) { return g_prep_err.c_str(); }

HISPMV_API int hispmv_host_threads(void) { return host_threads(); }

HISPMV_API int hispmv_prep_from_coo(hispmv_prep** out, const int32_t* r, const int32_t* cl, const float* v,
                                    int64_t nnz, int32_t rows, int32_t cols) {
    if (!out) return HISPMV_EINVAL;
    host_threads();
    *out = nullptr;
    if (rows <= 0 || cols <= 0 || nnz < 0) { g_prep_err = "bad sparse matrix arguments"; return HISPMV_EINVAL; }
    try {
        auto p = std::make_unique<hispmv_prep>();
        p->csr = coo_to_csr(rows, cols, nnz, r, cl, v);
        p->st = build_stream(p->csr);
        *out = p.release();
        return HISPMV_OK;
    } catch (const std::exception& ex) { g_prep_err = ex.what(); return HISPMV_EINVAL; }
}

HISPMV_API int hispmv_prep_from_coo_device(hispmv_prep** out, int device_id, const int32_t* r, const int32_t* cl, const float* v,
                                           int64_t nnz, int32_t rows, int32_t cols, double seconds[5]) {
    if (!out) return HISPMV_EINVAL;
    *out = nullptr;
    if (rows <= 0 || cols <= 0 || nnz < 0 || (nnz > 0 && (!r || !cl || !v))) { g_prep_err = "bad sparse matrix arguments"; return HISPMV_EINVAL; }
    if (hipSetDevice(device_id) != hipSuccess) { g_prep_err = "no such HIP device"; return HISPMV_EDEVICE; }
    try {
        auto p = std::make_unique<hispmv_prep>();
        DevicePrepTimes t;
        std::string err;
        if (!prep_on_device(rows, cols, nnz, r, cl, v, p->csr, p->st, t, err)) {
            g_prep_err = err;
            return err.find("outside") != std::string::npos || err.find("dimension") != std::string::npos ? HISPMV_EINVAL : HISPMV_EDEVICE;
        }
        if (seconds) { seconds[0] = t.upload; seconds[1] = t.csr_device; seconds[2] = t.offsets_host; seconds[3] = t.stream_device; seconds[4] = t.download; }
        *out = p.release();
        return HISPMV_OK;
    } catch (const std::exception& ex) { g_prep_err = ex.what(); return HISPMV_EINVAL; }
}

HISPMV_API int hispmv_prep_from_mtx(hispmv_prep** out, const char* path, int flavor) {
    host_threads();
    if (!out) return HISPMV_EINVAL;
    *out = nullptr;
    if (!path || (flavor != 0 && flavor != 1)) { g_prep_err = "bad arguments"; return HISPMV_EINVAL; }
    try {
        Coo coo = read_mtx(path, (MtxFlavor)flavor);
        auto p = std::make_unique<hispmv_prep>();
        p->csr = coo_to_csr(coo.rows, coo.cols, (int64_t)coo.r.size(), coo.r.data(), coo.c.data(), coo.v.data());
        p->st = build_stream(p->csr);
        *out = p.release();
        return HISPMV_OK;
    } catch (const std::runtime_error& ex) { g_prep_err = ex.what(); return HISPMV_EIO;
    } catch (const std::exception& ex) { g_prep_err = ex.what(); return HISPMV_EINVAL; }
}

HISPMV_API void hispmv_prep_free(hispmv_prep* p) { delete p; }

// The format / tiling decision of the loader for this matrix on a device with n_cus compute units, host-only
// (hispmv_choose.cpp: the same function hispmv_create_sparse_handle* calls).  Works on a copy of the prepared CSR.
HISPMV_API int hispmv_prep_choose_format(const hispmv_prep* p, int n_cus, int64_t out[16]) {
    if (!p || !out || n_cus <= 0) return HISPMV_EINVAL;
    try {
        Csr copy = p->csr;
        FormatOptions opt = FormatOptions::from_env();
        opt.decide_only = true;
        const FormatChoice ch = choose_format(std::move(copy), nullptr, n_cus, opt);
        int64_t n_slices = 0, n_elems = 0, n_split = 0, global_elems = 0;
        for (const HostPart& q : ch.parts) {
            if (q.is_tts) { n_slices += (int64_t)q.tts.col_base.size(); n_elems += q.tts.nnz + q.tts.n_fillers; n_split += (int64_t)q.tts.fix.size() / 4; }
            else { n_slices += q.st.n_slices; n_elems += q.st.n_elems; n_split += (int64_t)q.st.fix.size(); global_elems += q.plan.lds_floats > 0 ? q.plan.global_elems : q.st.n_slices * (int64_t)kSliceElems; }
        }
        const HostPart& p0 = ch.parts[0];
        out[0] = ch.format; out[1] = ch.parts.size() > 1 ? (ch.tile_kind ? ch.tile_kind : 1) : 0; out[2] = (int64_t)ch.parts.size();
        out[3] = ch.col_tile_width; out[4] = ch.col_tile_base; out[5] = ch.l2_tiles ? 1 : 0;
        out[6] = ch.format == 1 ? p0.tts.geometry.threads : p0.plan.block_threads;
        out[7] = ch.format == 1 ? p0.tts.geometry.max_slots / kTtsChunk : p0.plan.group_slices;
        out[8] = ch.format == 1 ? 0 : p0.plan.lds_floats;
        out[9] = n_slices; out[10] = n_elems; out[11] = n_split;
        out[12] = (int64_t)(ch.tts_lines_per_gather * 1000.0 + 0.5);
        out[13] = global_elems;        // elements that gather x through L2 (slice streams: outside their window, or no window at all)
        out[14] = 0; out[15] = 0;
        return HISPMV_OK;
    } catch (const std::exception& ex) { g_prep_err = ex.what(); return HISPMV_EINVAL; }
}

HISPMV_API int hispmv_prep_swapped_coo_from_csr(const int32_t* row_ptr, const int32_t* col_idx, int32_t rows, int32_t* out_rows, int32_t* out_cols) {
    if (!row_ptr || rows <= 0 || row_ptr[0] != 0) { g_prep_err = "bad CSR arguments"; return HISPMV_EINVAL; }
    for (int32_t i = 0; i < rows; ++i) if (row_ptr[i + 1] < row_ptr[i]) { g_prep_err = "row_ptr must be non-decreasing"; return HISPMV_EINVAL; }
    const int64_t nnz = row_ptr[rows];
    if (nnz > 0 && (!col_idx || !out_rows || !out_cols)) { g_prep_err = "bad CSR arguments"; return HISPMV_EINVAL; }
    host_threads();
    if (nnz > 0) std::memcpy(out_rows, col_idx, (size_t)nnz * sizeof(int32_t));
    csr_entry_rows(rows, row_ptr, out_cols);
    return HISPMV_OK;
}

HISPMV_API int hispmv_prep_step_queue(const double* slice_costs, int32_t n_slice, const double* tile_costs, int32_t n_tile, int32_t n_wg, int32_t mode,
                                      int32_t* out_class, int32_t* out_index) {
    if (n_slice < 0 || n_tile < 0 || n_wg <= 0 || mode < 0 || (mode > 4 && mode < 16) || mode > 255 || (n_slice > 0 && !slice_costs) || (n_tile > 0 && !tile_costs) ||
        (n_slice + n_tile > 0 && (!out_class || !out_index))) return HISPMV_EINVAL;
    try {
        const std::vector<double> a(slice_costs, slice_costs + n_slice), b(tile_costs, tile_costs + n_tile);
        const auto order = order_step_queue(a, b, n_wg, mode);
        for (size_t i = 0; i < order.size(); ++i) { out_class[i] = order[i].first; out_index[i] = order[i].second; }
        return HISPMV_OK;
    } catch (const std::exception& ex) { g_prep_err = ex.what(); return HISPMV_EINVAL; }
}

// inside[nnz]: 1 for the CSR entries whose block of x lies in the window of their workgroup under the launch plan for n_cus CUs
// (the criterion of the stray split, hispmv_matrix_info.tile_kind 3).  For tests: lets the wavefront model pack the two parts.
HISPMV_API int hispmv_prep_window_membership(const hispmv_prep* p, int n_cus, uint8_t* inside) {
    if (!p || !inside || n_cus <= 0) return HISPMV_EINVAL;
    try {
        SliceStream copy = build_stream(p->csr);
        const LaunchPlan plan = make_plan(copy, n_cus);
        const std::vector<uint8_t> m = window_membership(p->csr, plan);
        std::copy(m.begin(), m.end(), inside);
        return HISPMV_OK;
    } catch (const std::exception& ex) { g_prep_err = ex.what(); return HISPMV_EINVAL; }
}

HISPMV_API int hispmv_prep_dims(const hispmv_prep* p, int64_t d[8]) {
    if (!p || !d) return HISPMV_EINVAL;
    d[0] = p->st.rows; d[1] = p->st.cols; d[2] = p->st.nnz; d[3] = p->st.n_elems; d[4] = p->st.n_slices;
    d[5] = kSliceElems; d[6] = (int64_t)p->st.fix.size(); d[7] = p->st.bytes();
    return HISPMV_OK;
}
HISPMV_API int hispmv_prep_plan(const hispmv_prep* p, int n_cus, int64_t plan[6]) {
    if (!p || !plan || n_cus <= 0) return HISPMV_EINVAL;
    SliceStream copy = p->st;                      // make_plan rewrites the words of staged groups
    const LaunchPlan g = make_plan(copy, n_cus);
    plan[0] = g.block_threads; plan[1] = g.group_slices; plan[2] = g.lds_floats; plan[3] = g.ytile_floats;
    plan[4] = (int64_t)g.groups.size();
    plan[5] = ((int64_t)g.lds_floats + (int64_t)g.ytile_floats * (g.block_threads / 64)) * 4;
    return HISPMV_OK;
}

// The widths hispmv_linear_device / hispmv_linear_device_t take for this stream as a single-part handle: the plan's workgroup, its
// window with the stray areas the packer puts behind it, its row tiles -- the figures the loader hands the launchers.
HISPMV_API int hispmv_prep_vector_widths(const hispmv_prep* p, int n_cus, int64_t num_vecs, int64_t out[2]) {
    if (!p || !out || n_cus <= 0 || num_vecs < 1) return HISPMV_EINVAL;
    SliceStream copy = p->st;
    const LaunchPlan g = make_plan(copy, n_cus);
    const DeviceStream ds = pack_device_stream(copy, g, false, p->half_values);
    SpmvDeviceMatrix d;
    d.block_threads = g.block_threads; d.group_slices = g.group_slices;
    d.lds_floats = g.lds_floats + ds.stray_floats; d.ytile_floats = g.ytile_floats;
    d.rows = p->st.rows; d.cols = p->st.cols;
    out[0] = spmv_batch_width(d, num_vecs);
    out[1] = spmv_t_width(d, num_vecs);
    return HISPMV_OK;
}

HISPMV_API int hispmv_prep_apply_plan(hispmv_prep* p, int n_cus, int64_t counts[2]) {
    if (!p || !counts || n_cus <= 0) return HISPMV_EINVAL;
    p->plan = make_plan(p->st, n_cus);
    counts[0] = (int64_t)p->plan.groups.size(); counts[1] = (int64_t)p->plan.frags.size();
    return HISPMV_OK;
}
// Host-only counterpart of hispmv_set_value_storage: bf16 rounds the prepared values once, in place -- the CSR and the value halves of
// the stream words (fillers and padding are zeros: unchanged) -- and selects the half slice for hispmv_prep_device_stream.
HISPMV_API int hispmv_prep_set_value_storage(hispmv_prep* p, int storage) {
    if (!p || (storage != HISPMV_VALUES_FP32 && storage != HISPMV_VALUES_BF16)) { g_prep_err = "bad value storage arguments"; return HISPMV_EINVAL; }
    p->half_values = storage == HISPMV_VALUES_BF16;
    if (!p->half_values) return HISPMV_OK;
    for (float& v : p->csr.val) { uint32_t u; std::memcpy(&u, &v, 4); u = round_bits_to_bf16(u); std::memcpy(&v, &u, 4); }
    for (uint64_t& w : p->st.words) w = (w & 0xffffffff00000000ull) | round_bits_to_bf16((uint32_t)w);
    return HISPMV_OK;
}
// The device layout of the stream under the plan hispmv_prep_apply_plan computed (call that first): counts = {bytes, groups,
// compact slices, slices with stray slots, stray-area floats, window floats of the plan}; arrays through hispmv_prep_device_array.
HISPMV_API int hispmv_prep_device_stream(hispmv_prep* p, int64_t counts[6]) {
    if (!p || !counts) return HISPMV_EINVAL;
    try {
        p->dstream = pack_device_stream(p->st, p->plan, true, p->half_values);
        counts[0] = (int64_t)p->dstream.bytes.size(); counts[1] = (int64_t)p->dstream.groups.size() / 4; counts[2] = p->dstream.compact_slices;
        counts[3] = p->dstream.stray_slices; counts[4] = p->dstream.stray_floats; counts[5] = p->plan.lds_floats;
        return HISPMV_OK;
    } catch (const std::exception& ex) { g_prep_err = ex.what(); return HISPMV_EINVAL; }
}
// The same layout written by the DEVICE (layout_on_device, what hispmv_load_matrices runs with HISPMV_LAYOUT=device) from the planned host words:
// call hispmv_prep_apply_plan and hispmv_prep_device_stream first; bytes_out takes counts[0] bytes, stray_cols_out n_slices x 64 u32
// (may be null when counts[4] == 0).  For tests: device == host, byte for byte.
HISPMV_API int hispmv_prep_device_stream_on_device(hispmv_prep* p, int device_id, uint8_t* bytes_out, uint32_t* stray_cols_out) {
    if (!p || !bytes_out) return HISPMV_EINVAL;
    if (p->dstream.groups.empty() || (int64_t)p->st.words.size() != p->st.n_slices * kSliceElems) { g_prep_err = "call hispmv_prep_apply_plan and hispmv_prep_device_stream first"; return HISPMV_ESTATE; }
    if (hipSetDevice(device_id) != hipSuccess) { g_prep_err = "no such HIP device"; return HISPMV_EDEVICE; }
    const int64_t ns = p->st.n_slices;
    const size_t wb = p->st.words.size() * sizeof(uint64_t), gb = p->dstream.groups.size() * sizeof(int32_t), sb = (size_t)ns * kStraySlots * sizeof(uint32_t);
    void *dw = nullptr, *dg = nullptr, *db = nullptr, *ds = nullptr;
    auto done = [&](int rc, const char* what) { if (rc != HISPMV_OK) g_prep_err = what; (void)hipFree(dw); (void)hipFree(dg); (void)hipFree(db); (void)hipFree(ds); return rc; };
    if (hipMalloc(&dw, std::max<size_t>(wb, 8)) != hipSuccess || hipMalloc(&dg, gb) != hipSuccess || hipMalloc(&db, std::max<int64_t>(p->dstream.n_bytes, 8)) != hipSuccess)
        return done(HISPMV_EDEVICE, "hipMalloc failed");
    const bool strays = p->dstream.any_stray && stray_cols_out;
    if (strays && (hipMalloc(&ds, sb) != hipSuccess || hipMemset(ds, 0xff, sb) != hipSuccess)) return done(HISPMV_EDEVICE, "hipMalloc failed");
    if (hipMemcpy(dw, p->st.words.data(), wb, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(dg, p->dstream.groups.data(), gb, hipMemcpyHostToDevice) != hipSuccess)
        return done(HISPMV_EDEVICE, "hipMemcpy failed");
    if (layout_on_device((const uint64_t*)dw, ns, p->plan.group_slices, (const int32_t*)dg, p->plan.lds_floats, p->plan.block_threads / 64, (uint8_t*)db, (uint32_t*)ds, nullptr) != 0)
        return done(HISPMV_EDEVICE, "layout kernel launch failed");
    if (hipDeviceSynchronize() != hipSuccess) return done(HISPMV_EDEVICE, "layout kernel failed");
    if (hipMemcpy(bytes_out, db, (size_t)p->dstream.n_bytes, hipMemcpyDeviceToHost) != hipSuccess) return done(HISPMV_EDEVICE, "hipMemcpy failed");
    if (strays && hipMemcpy(stray_cols_out, ds, sb, hipMemcpyDeviceToHost) != hipSuccess) return done(HISPMV_EDEVICE, "hipMemcpy failed");
    return done(HISPMV_OK, "");
}
HISPMV_API const void* hispmv_prep_device_array(const hispmv_prep* p, int which) {
    if (!p) return nullptr;
    switch (which) {
        case 0: return p->dstream.bytes.data();
        case 1: return p->dstream.groups.data();
        case 2: return p->dstream.stray_cols.data();
        default: return nullptr;
    }
}
HISPMV_API const int32_t* hispmv_prep_groups(const hispmv_prep* p) { return (const int32_t*)p->plan.groups.data(); }
HISPMV_API const int32_t* hispmv_prep_frags(const hispmv_prep* p) { return (const int32_t*)p->plan.frags.data(); }

HISPMV_API int hispmv_prep_build_tts(hispmv_prep* p, int64_t target_tile_elems, int small_geometry, int64_t counts[8], double* lines_per_gather) {
    if (!p || !counts) return HISPMV_EINVAL;
    try {
        TtsGeometry geo;
        if (small_geometry == 1) { geo.max_slots = kTtsSmallSlots; geo.max_rows = kTtsSmallRows; geo.tiles_wanted = 512; }
        if (small_geometry == 6) geo.zero_fill = true;      // the standard sizes without filler words (HISPMV_TTS_GEOMETRY=zerofill)
        if ((small_geometry >= 2 && small_geometry < 6) || small_geometry == 8 || small_geometry == 9) {         // 2 + q / 4 + q / 8 + q: column part q of the tall / paired / tall gap-coded geometry, as the loader builds it for a 256-CU device
            const bool paired = small_geometry >= 4 && small_geometry < 6, gap = small_geometry >= 8;
            const int q = small_geometry - (gap ? 8 : paired ? 4 : 2);
            if (q >= kTtsTallParts) { g_prep_err = "no such column part"; return HISPMV_EINVAL; }
            const std::vector<int32_t> cuts = tts_column_cuts(p->csr, kTtsTallParts);
            const Csr part = csr_column_range(p->csr, q == 0 ? 0 : cuts[(size_t)q - 1], q + 1 == kTtsTallParts ? p->csr.cols : cuts[(size_t)q]);
            p->tts = build_tts(part, target_tile_elems, gap ? tts_tallgap_geometry(256, kTtsTallParts) : paired ? tts_paired_geometry(256) : tts_tall_geometry(256, kTtsTallParts));
        } else
        p->tts = build_tts(p->csr, target_tile_elems, geo);
    } catch (const std::exception& ex) { g_prep_err = ex.what(); return HISPMV_EINVAL; }
    const TtsStream& t = p->tts;
    counts[0] = (int64_t)t.tiles.size(); counts[1] = (int64_t)t.blocks.size(); counts[2] = (int64_t)t.col_base.size();
    counts[3] = (int64_t)t.chunk_info.size() / 2; counts[4] = t.n_fillers; counts[5] = t.n_pad_words; counts[6] = t.max_rows; counts[7] = t.max_slots;
    if (lines_per_gather) *lines_per_gather = t.lines_per_gather;
    return HISPMV_OK;
}
HISPMV_API int hispmv_prep_tts_pieces(const hispmv_prep* p, int64_t counts[2]) {
    if (!p || !counts) return HISPMV_EINVAL;
    counts[0] = (int64_t)p->tts.fix.size() / 4; counts[1] = p->tts.n_carry;
    return HISPMV_OK;
}
HISPMV_API const void* hispmv_prep_tts_array(const hispmv_prep* p, int which) {
    if (!p) return nullptr;
    switch (which) {
        case 6: return p->tts.fix.data();
        case 7: return p->tts.flags_hi.data();
        case 0: return p->tts.words.data();
        case 1: return p->tts.col_base.data();
        case 2: return p->tts.flags.data();
        case 3: return p->tts.chunk_info.data();
        case 4: return p->tts.tiles.data();
        case 5: return p->tts.blocks.data();
        default: return nullptr;
    }
}

HISPMV_API const int64_t* hispmv_prep_csr_row_ptr(const hispmv_prep* p) { return p->csr.row_ptr.data(); }
HISPMV_API const int32_t* hispmv_prep_csr_col(const hispmv_prep* p) { return p->csr.col.data(); }
HISPMV_API const float* hispmv_prep_csr_val(const hispmv_prep* p) { return p->csr.val.data(); }
HISPMV_API const uint64_t* hispmv_prep_words(const hispmv_prep* p) { return p->st.words.data(); }
HISPMV_API const int32_t* hispmv_prep_slice_hdr(const hispmv_prep* p) { return (const int32_t*)p->st.hdr.data(); }
HISPMV_API const int32_t* hispmv_prep_fix(const hispmv_prep* p) { return (const int32_t*)p->st.fix.data(); }

// Every device layout of the handle hispmv_create_sparse_handle would make from this COO input on a device with n_cus CUs, packed
// twice by the same host path: with the real values, and -- as for a handle created with value updates on -- with the index
// payloads bits(k + 1).  The map is read out of the payload layouts' value regions (value_chunks) exactly as the loader reads it on
// the device.  For tests: gathering the values through the map must give the real layouts byte for byte.
// `storage` = HISPMV_VALUES_BF16: what a handle created under HISPMV_VALUE_UPDATES_ANY_STORAGE with bf16 storage gets.  The real
// layouts are packed from R(values), half groups included; the payload layouts have the same group tables and metas, their half
// slices hold no payloads (a 16-bit slot cannot), and the map is the one the loader uploads: the parts' HostPart::value_map, read
// from the host words (host_value_map).  Array 4 names the kind of every chunk destination.
HISPMV_API int hispmv_prep_value_layouts_storage(hispmv_prep** out, const int32_t* r, const int32_t* cl, const float* v, int64_t nnz, int32_t rows,
                                                 int32_t cols, int n_cus, int storage, int64_t counts[8]) {
    if (!out) return HISPMV_EINVAL;
    if (storage != HISPMV_VALUES_FP32 && storage != HISPMV_VALUES_BF16) { g_prep_err = "unknown value storage"; return HISPMV_EINVAL; }
    const bool bf16 = storage == HISPMV_VALUES_BF16;
    host_threads();
    *out = nullptr;
    if (rows <= 0 || cols <= 0 || nnz < 0 || n_cus <= 0 || !counts || (nnz > 0 && (!r || !cl || !v))) { g_prep_err = "bad sparse matrix arguments"; return HISPMV_EINVAL; }
    if (nnz > 0x7F7FFFFFll) { g_prep_err = "more entries than an index payload can name"; return HISPMV_EINVAL; }
    try {
        FormatOptions opt = FormatOptions::from_env();
        if (opt.tts_geometry != 0 || opt.tts_small) { g_prep_err = "value updates: experiment geometries are refused"; return HISPMV_EINVAL; }
        opt.device_layout = false;             // (the bytes on the host; HISPMV_LAYOUT=device writes the same ones on the device)
        auto p = std::make_unique<hispmv_prep>();
        std::vector<float> payloads((size_t)nnz);
        for (int64_t k = 0; k < nnz; ++k) { const uint32_t b = (uint32_t)(k + 1); std::memcpy(&payloads[(size_t)k], &b, 4); }
        int64_t info[4] = {0, 0, 0, 0};
        opt.half_values = bf16;
        std::vector<float> rounded;
        if (bf16) {
            rounded.resize((size_t)nnz);
            for (int64_t k = 0; k < nnz; ++k) { uint32_t u; std::memcpy(&u, v + k, 4); u = round_bits_to_bf16(u); std::memcpy(&rounded[(size_t)k], &u, 4); }
            v = rounded.data();
        }
        auto pack = [&](const float* vals, std::vector<uint8_t>& bytes, bool record) {
            opt.index_payloads = bf16 && record;
            FormatChoice ch = choose_format(coo_to_csr(rows, cols, nnz, r, cl, vals), nullptr, n_cus, opt);
            if (record) { info[0] = ch.format; info[1] = ch.parts.size() > 1 ? (ch.tile_kind ? ch.tile_kind : 1) : 0; info[2] = (int64_t)ch.parts.size(); }
            for (const HostPart& q : ch.parts) {
                const std::vector<ValueChunk> chunks = value_chunks(q);
                const int64_t base0 = (int64_t)bytes.size();
                if (q.is_tts) bytes.insert(bytes.end(), q.tts.words.begin(), q.tts.words.end());
                else bytes.insert(bytes.end(), q.dstream.bytes.begin(), q.dstream.bytes.end());
                const int64_t base1 = (int64_t)bytes.size();
                if (!q.is_tts && q.has_batch_layout) { bytes.insert(bytes.end(), q.batch_dstream.bytes.begin(), q.batch_dstream.bytes.end()); info[3]++; }
                if (!record) continue;
                for (const ValueChunk& c : chunks) {
                    p->vl_chunks.push_back(base0 + c.off0);
                    p->vl_chunks.push_back(c.off1 >= 0 ? base1 + c.off1 : -1);
                    p->vl_kinds.push_back(c.kind0);
                    p->vl_kinds.push_back(c.off1 >= 0 ? c.kind1 : kChunkSlots32);
                }
                if (bf16) {           // the map as the loader gets it (slice parts: kept by pack_part; tile streams: read from their words)
                    const std::vector<int32_t> part_map = q.is_tts ? host_value_map(q) : q.value_map;
                    if (part_map.size() != chunks.size() * (size_t)kValueChunk) throw std::logic_error("internal: a part's host value map does not match its chunks");
                    p->vl_map.insert(p->vl_map.end(), part_map.begin(), part_map.end());
                }
            }
        };
        pack(v, p->vl_real, false);
        pack(payloads.data(), p->vl_index, true);
        const int64_t n_chunks = (int64_t)p->vl_chunks.size() / 2;
        if (bf16 && (int64_t)p->vl_map.size() != n_chunks * kValueChunk) { g_prep_err = "internal: host value map size"; return HISPMV_EINVAL; }
        p->vl_map.resize((size_t)n_chunks * kValueChunk);
        int64_t written = 0;
        for (int64_t k = 0; k < n_chunks; ++k) {
            const int64_t off = p->vl_chunks[(size_t)k * 2];
            if (off < 0 || off + kValueChunk * 4 > (int64_t)p->vl_index.size()) { g_prep_err = "internal: value region outside its layout"; return HISPMV_EINVAL; }
            if (!bf16) std::memcpy(p->vl_map.data() + k * kValueChunk, p->vl_index.data() + off, kValueChunk * 4);
            written += kValueChunk * (p->vl_chunks[(size_t)k * 2 + 1] >= 0 ? 2 : 1);
        }
        counts[0] = (int64_t)p->vl_index.size(); counts[1] = (int64_t)p->vl_map.size(); counts[2] = n_chunks; counts[3] = written;
        counts[4] = info[0]; counts[5] = info[1]; counts[6] = info[2]; counts[7] = info[3];
        if (p->vl_real.size() != p->vl_index.size()) { g_prep_err = "the layouts of the two packings differ in size"; return HISPMV_EINVAL; }
        *out = p.release();
        return HISPMV_OK;
    } catch (const std::exception& ex) { g_prep_err = ex.what(); return HISPMV_EINVAL; }
}

HISPMV_API int hispmv_prep_value_layouts(hispmv_prep** out, const int32_t* r, const int32_t* cl, const float* v, int64_t nnz, int32_t rows,
                                         int32_t cols, int n_cus, int64_t counts[8]) {
    return hispmv_prep_value_layouts_storage(out, r, cl, v, nnz, rows, cols, n_cus, HISPMV_VALUES_FP32, counts);
}

// 0 = the layouts with the real values (counts[0] bytes; bf16 storage: packed from R(values), half groups included), 1 = the same
// with the index payloads, 2 = the map (int32, counts[1]), 3 = the chunks (counts[2] x int64 {byte offset of the first destination,
// of the second or -1}), 4 = the kinds (counts[2] x 2 int32, the shape of 3: 0 = 1024 fp32 slots, 1 = a half slice).
HISPMV_API const void* hispmv_prep_value_array(const hispmv_prep* p, int which) {
    if (!p) return nullptr;
    switch (which) {
        case 0: return p->vl_real.data();
        case 1: return p->vl_index.data();
        case 2: return p->vl_map.data();
        case 3: return p->vl_chunks.data();
        case 4: return p->vl_kinds.data();
        default: return nullptr;
    }
}

// The workspace rule of restarted GMRES (hispmv_gmres.h: gmres_layout), which hispmv_gmres_info and hispmv_gmres_device follow.
HISPMV_API int hispmv_prep_gmres(int64_t n, int64_t restart, int with_minv, int64_t out[8]) {
    if (!out || n < 0 || restart < 1 || restart > kGmresMaxRestart) return HISPMV_EINVAL;
    const GmresLayout l = gmres_layout(n, restart, with_minv != 0);
    out[0] = l.work_bytes; out[1] = l.off_v; out[2] = l.stride; out[3] = l.groups; out[4] = kGmresDotTile;
    out[5] = kGmresLaunchesInner; out[6] = kGmresLaunchesCycle; out[7] = restart + 1;
    return HISPMV_OK;
}

// The layout rule of a block-Jacobi buffer (hispmv_block_jacobi.h: block_jacobi_layout), which every block-Jacobi entry follows.
HISPMV_API int hispmv_prep_block_jacobi(int64_t n, int64_t bs, int64_t out[4]) {
    if (!out || n < 0 || n > 0x7fffffffLL || !block_jacobi_size_ok(bs)) return HISPMV_EINVAL;
    const BlockJacobiLayout l = block_jacobi_layout(n, bs);
    out[0] = l.n_blocks; out[1] = l.pre_bytes; out[2] = l.off_flags; out[3] = l.block_floats;
    return HISPMV_OK;
}
