// hispmv_tts_transpose.hip -- the transposed product and the value gradient on the transposed tile stream (hispmv_tts_transpose.h).
// The bit and load helpers, store_grad and the LDS limit of a launch it shares with the other four satellite files
// (hispmv_slice_walk.h); the few helpers of the tile-stream format (the slice request, the row-end arithmetic of the forward kernel's
// phase B) are its own text, as hispmv_kernels.hip keeps its own: no forward kernel is touched from here.
//
// One workgroup per tile (hispmv_tts.h), LDS [x rows of the tile: acc_floats][staging: one float per row-major slot of the block in
// flight] -- the forward kernel's layout without the chunk tails.  Per block the forward kernel's two phases in the other order:
//   EXPAND   (row-major order, a wavefront per chunk of 1024 slots): row(slot) = chunk_info.x + the row ends at earlier slots of the
//            chunk (the ballots of the forward phase B, applied to every slot), staging[slot] = xrows[row(slot)], one float4 store per
//            lane and step.  Rows cut by chunk boundaries need nothing extra: there are no tails and no chain.
//   barrier
//   SCATTER  (column order, a wavefront per slice of 1024 words): a word {value, col_off:16 | slot:16} adds alpha * value *
//            staging[slot] to y[col_base + col_off].  Sorted element 256 j + 64 k + l sits at word 256 j + 4 l + k, and the atomics are
//            issued per word position k: the 64 lanes of a wave-instruction cover 64 consecutive columns of the sort, a few lines of y
//            (hispmv_matrix_info.tts_lines_per_gather) instead of the 64 of a slice stream without a window.
//            A word whose value is +-0 is skipped: the zero-slot rule of hispmv_spmv_device_t, and required here -- padding words
//            point at slot geometry.max_slots, which the expand never wrote.
//   barrier  (the next block's expand overwrites the staging)
// A carry tile (row0 < 0: one piece of a long row) reads x[row] of the `fix` entry whose carry range holds -row0 - 1; carry[] itself
// is neither read nor written.  The value gradient runs the same expand with gy in place of x and, in the column-order phase, reads
// the metas and the value map only: grad[q - 1] = sum_v staging_v[slot] * x[v, col], one writer per entry.
#include <hip/hip_runtime.h>

#include "hispmv_slice_walk.h"
#include "hispmv_tts_transpose.h"
#include "hispmv_update.h"

namespace hispmv {

namespace {

constexpr int kChunkSlots = 1024;      // hispmv_tts.h: kTtsChunk (slots per row-major chunk, words per column-order slice)

// A column-order slice as it arrives: 4 values and 4 metas per lane and step (the forward kernel's TtsSlice); the gradient requests
// the metas alone (they begin 4096 B behind the values).
struct TtsSlice { uint4 v[kSliceSteps]; uint4 m[kSliceSteps]; };
struct TtsMetas { uint4 m[kSliceSteps]; };
__device__ __forceinline__ void tts_request(TtsSlice& s, const char* words, int slice, int lane) {
    const uint4* pv = (const uint4*)(words + (size_t)slice * (kSliceElems * 8)) + lane;
#pragma unroll
    for (int j = 0; j < kSliceSteps; ++j) s.v[j] = load_words(pv + j * 64);
#pragma unroll
    for (int j = 0; j < kSliceSteps; ++j) s.m[j] = load_words(pv + 256 + j * 64);
}
__device__ __forceinline__ void tts_request(TtsMetas& s, const char* words, int slice, int lane) {
    const uint4* pv = (const uint4*)(words + (size_t)slice * (kSliceElems * 8)) + lane;
#pragma unroll
    for (int j = 0; j < kSliceSteps; ++j) s.m[j] = load_words(pv + 256 + j * 64);
}

// The row whose x a tile reads first: row0, or -- a carry tile, row0 < 0, one piece of a long row -- the row of the fix entry
// {row, first carry, carries, 0} whose carry range holds -row0 - 1 (-1: none does; the tile then reads zeros).  The list is short.
__device__ __forceinline__ int tile_first_row(const TtsDeviceMatrix& M, int row0) {
    if (row0 >= 0) return row0;
    const int ci = -row0 - 1;
    int row = -1;
    for (int f = 0; f < M.n_fix; ++f) {
        const int4 e = load_int4(M.fix + f);
        if (ci >= e.y && ci < e.y + e.z) row = e.x;
    }
    return row;
}

// in[v * M.rows + row + i], i < n_rows, -> rows0[v * M.acc_floats + i], coalesced; each vector through its own descriptor over its
// M.rows floats, so a row past the end reads 0 and not the next vector's first float
template <int NV>
__device__ __forceinline__ void load_tile_rows(const TtsDeviceMatrix& M, const float* in, float* rows0, int row, int n_rows, unsigned tid) {
#pragma unroll 1
    for (int v = 0; v < NV; ++v) {
        const __amdgpu_buffer_rsrc_t r = float_buffer(in + (size_t)v * (size_t)M.rows, M.rows);
        for (int i = (int)tid; i < n_rows; i += (int)blockDim.x)
            rows0[v * M.acc_floats + i] = buffer_float(r, row >= 0 ? (unsigned)(row + i) << 2 : kNoAccess);
    }
}

// The expand of one chunk: staging_v[c * 1024 + slot] = rows_v[row(slot)] for the 1024 slots of chunk c and every vector.  `ends`: the
// lane's 16 flag bits (bit 4 j + k = row end at slot 256 j + 4 lane + k), `first`: the rows ending before the chunk.  Slots behind
// n_slots in the last chunk have no row: the index is clamped to the tile's rows.
template <int NV>
__device__ __forceinline__ void expand_chunk(const float* rows0, int acc_floats, float* staging0, int stage_stride, int c, int first, unsigned ends,
                                             int n_rows, int lane) {
    int row = __builtin_amdgcn_readfirstlane(first);
    const int last = n_rows > 0 ? n_rows - 1 : 0;
#pragma unroll
    for (int j = 0; j < kSliceSteps; ++j) {
        bool e[kLaneElems];
        int below = 0, total = 0;
#pragma unroll
        for (int k = 0; k < kLaneElems; ++k) {
            e[k] = ((ends >> (4 * j + k)) & 1u) != 0;
            const unsigned long long mk = __builtin_amdgcn_ballot_w64(e[k]);
            below += lanes_below(mk);
            total += __builtin_popcountll(mk);
        }
        int r[kLaneElems];
        r[0] = row + below;
#pragma unroll
        for (int k = 1; k < kLaneElems; ++k) r[k] = r[k - 1] + (e[k - 1] ? 1 : 0);
#pragma unroll
        for (int k = 0; k < kLaneElems; ++k) r[k] = min(max(r[k], 0), last);
#pragma unroll 1
        for (int v = 0; v < NV; ++v) {
            const float* const rows = rows0 + v * acc_floats;
            float4* const st4 = (float4*)(staging0 + v * stage_stride + c * kChunkSlots) + lane;
            st4[j * 64] = float4{rows[r[0]], rows[r[1]], rows[r[2]], rows[r[3]]};
        }
        row += total;
    }
}

// The scatter of one slice for NV vectors: the words are decoded once, vector v reads staging area v and adds into y + v * cols.
template <int NV>
__device__ __forceinline__ void scatter_slice(const TtsSlice& w, int col_base, const float* staging0, int stage_stride, float* y, int cols, float alpha) {
    constexpr int kE = kSliceSteps * kLaneElems;
    const int cb = __builtin_amdgcn_readfirstlane(col_base);
    const unsigned top = (unsigned)stage_stride - 1u;
    unsigned val[kE], meta[kE];
#pragma unroll
    for (int j = 0; j < kSliceSteps; ++j) {
        val[4 * j + 0] = w.v[j].x; val[4 * j + 1] = w.v[j].y; val[4 * j + 2] = w.v[j].z; val[4 * j + 3] = w.v[j].w;
        meta[4 * j + 0] = w.m[j].x; meta[4 * j + 1] = w.m[j].y; meta[4 * j + 2] = w.m[j].z; meta[4 * j + 3] = w.m[j].w;
    }
    // i = 4 j + k: one wave-instruction per word position, 64 consecutive columns of the sort.  In two halves of 8 words, each half
    // through all vectors: slots and columns of 8 words are what stays in registers across the vectors (with all 16 the NV = 4 body,
    // next to its two slice buffers, went to scratch)
#pragma unroll
    for (int i0 = 0; i0 < kE; i0 += kE / 2) {
        unsigned slot[kE / 2], col[kE / 2];
#pragma unroll
        for (int i = 0; i < kE / 2; ++i) {
            slot[i] = min(meta[i0 + i] & 0xffffu, top);
            // a +-0 word adds nothing, whatever x holds (its slot may never have been written): its column becomes one past the end
            col[i] = (val[i0 + i] & 0x7fffffffu) != 0u ? (unsigned)cb + (meta[i0 + i] >> 16) : kNoAccess;
        }
#pragma unroll 1
        for (int v = 0; v < NV; ++v) {
            const float* const staging = staging0 + v * stage_stride;
            float* const yv = y + (size_t)v * (size_t)cols;
            float xr[kE / 2];
#pragma unroll
            for (int i = 0; i < kE / 2; ++i) xr[i] = staging[slot[i]];
#pragma unroll
            for (int i = 0; i < kE / 2; ++i)
                if (col[i] < (unsigned)cols) y_add(yv, col[i], alpha * (i2f((int)val[i0 + i]) * xr[i]));
        }
    }
}

// The gradient's column-order phase for one slice: per word the sum over the vectors of staging_v[slot] (= gy[v, row]) * x[v, col], x
// gathered through a descriptor of the vector's `cols` floats, 8 gathers in flight per lane; stored through the slice's map chunk.
template <int NV>
__device__ __forceinline__ void grad_slice(const TtsMetas& w, int col_base, const float* staging0, int stage_stride, const int32_t* map_chunk,
                                           const float* x, float* grad, long long n, int cols, float alpha, float beta, int lane) {
    constexpr int kE = kSliceSteps * kLaneElems;
    const int cb = __builtin_amdgcn_readfirstlane(col_base);
    const unsigned top = (unsigned)stage_stride - 1u;
    unsigned meta[kE];
#pragma unroll
    for (int j = 0; j < kSliceSteps; ++j) { meta[4 * j + 0] = w.m[j].x; meta[4 * j + 1] = w.m[j].y; meta[4 * j + 2] = w.m[j].z; meta[4 * j + 3] = w.m[j].w; }
    float acc[kE];
#pragma unroll
    for (int i = 0; i < kE; ++i) acc[i] = 0.0f;
#pragma unroll 1
    for (int v = 0; v < NV; ++v) {
        const __amdgpu_buffer_rsrc_t rxv = float_buffer(x + (size_t)v * (size_t)cols, cols);
        const float* const staging = staging0 + v * stage_stride;
#pragma unroll
        for (int i0 = 0; i0 < kE; i0 += kE / 2) {
            float xg[kE / 2];
#pragma unroll
            for (int i = 0; i < kE / 2; ++i) {
                const unsigned col = (unsigned)cb + (meta[i0 + i] >> 16);
                xg[i] = buffer_float(rxv, col < (unsigned)cols ? col << 2 : kNoAccess);
            }
#pragma unroll
            for (int i = 0; i < kE / 2; ++i) {
                const float gr = staging[min(meta[i0 + i] & 0xffffu, top)];
                acc[i0 + i] = acc[i0 + i] + gr * xg[i];
            }
        }
    }
    // the map words of the slice, addressed as its values are: word 256 j + 4 lane + k
    const int4* const mp = (const int4*)map_chunk + lane;
#pragma unroll
    for (int j = 0; j < kSliceSteps; ++j) {
        const int4 q = load_int4(mp + j * 64);
        store_grad(grad, n, q.x, acc[4 * j + 0], alpha, beta);
        store_grad(grad, n, q.y, acc[4 * j + 1], alpha, beta);
        store_grad(grad, n, q.z, acc[4 * j + 2], alpha, beta);
        store_grad(grad, n, q.w, acc[4 * j + 3], alpha, beta);
    }
}

// The work of one workgroup on tile `tile_index`.  GRAD = false: y += alpha * A^T x (in = x, out = y); GRAD = true: the value gradient
// (in = gy, out = grad, x2 = x), which keeps only the metas of a slice.
// A wavefront takes slices `wave`, `wave + n_waves`, ... of a block through two buffers: its first slice of a block is requested a
// block ahead -- the first block's before the tile's rows are loaded, the next block's before the barrier that ends the block -- so its
// latency hides behind the load, or the barrier and the next expand; every later slice is requested before the slice in front of it
// is scattered.  (Both buffers requested a block ahead, as the forward kernel does, cost the NV = 4 body 72 B of scratch per lane.)
template <int NV, bool GRAD>
__device__ __forceinline__ void tts_t_tile(const TtsDeviceMatrix& M, const float* __restrict__ in, float* out, const float* __restrict__ x2,
                                           const int32_t* __restrict__ map, long long n, float alpha, float beta, int tile_index) {
    extern __shared__ float xs[];
    using Slice = typename std::conditional<GRAD, TtsMetas, TtsSlice>::type;
    const unsigned tid = threadIdx.x;
    const int lane = (int)(tid & 63), wave = (int)(tid >> 6), n_waves = (int)(blockDim.x >> 6);
    const int stage_stride = NV > 1 ? M.batch_stage_floats : M.staging_floats;
    float* const rows0 = xs;
    float* const staging0 = xs + M.acc_floats * NV;
    const int max_chunks = stage_stride / kChunkSlots;       // (whole chunks the staging holds: the expand writes whole chunks)
    const char* const words = (const char*)M.words;
    const int4 tile = load_int4(M.tiles + tile_index);
    const int row0 = __builtin_amdgcn_readfirstlane(tile.x), block_begin = __builtin_amdgcn_readfirstlane(tile.z);
    const int n_rows = min(__builtin_amdgcn_readfirstlane(tile.y), M.acc_floats), n_blocks = __builtin_amdgcn_readfirstlane(tile.w);
    if (n_blocks <= 0) return;

    int4 blk = load_int4(M.blocks + 2 * (size_t)block_begin);
    Slice wA, wB;
    int cbA = 0, cbB = 0;
    auto request = [&](Slice& w, int& cb, int slice) {
        tts_request(w, words, slice, lane);
        cb = *(const HISPMV_GLOBAL int*)(M.col_base + slice);
    };
    if (wave < blk.y) request(wA, cbA, blk.x + wave);
    load_tile_rows<NV>(M, in, rows0, tile_first_row(M, row0), n_rows, tid);
    __syncthreads();

    auto column_phase = [&](const Slice& w, int cb, int slice) {
        if constexpr (GRAD) grad_slice<NV>(w, cb, staging0, stage_stride, map + (size_t)slice * kValueChunk, x2, out, n, M.cols, alpha, beta, lane);
        else scatter_slice<NV>(w, cb, staging0, stage_stride, out, M.cols, alpha);
    };
    for (int b = 0; b < n_blocks; ++b) {
        const int slice_begin = __builtin_amdgcn_readfirstlane(blk.x), n_slices = __builtin_amdgcn_readfirstlane(blk.y);
        const int chunk_begin = __builtin_amdgcn_readfirstlane(blk.z), n_chunks = min(__builtin_amdgcn_readfirstlane(blk.w), max_chunks);
        int4 nxt = int4{0, 0, 0, 0};
        if (b + 1 < n_blocks) nxt = load_int4(M.blocks + 2 * (size_t)(block_begin + b + 1));
        // ---- expand: row-major order ----------------------------------------------------------------------------------------
        for (int c = wave; c < n_chunks; c += n_waves) {
            const int first = *(const HISPMV_GLOBAL int*)((const int*)M.chunk_info + 2 * (size_t)(chunk_begin + c));
            const unsigned ends = *(const HISPMV_GLOBAL unsigned short*)(M.flags + (size_t)(chunk_begin + c) * 64 + lane);
            expand_chunk<NV>(rows0, M.acc_floats, staging0, stage_stride, c, first, ends, n_rows, lane);
        }
        __syncthreads();
        // ---- scatter / gradient: column order; wA holds slice `wave` of the block, the two buffers then alternate -----------------
        if (wave < n_slices) {
            int s = wave + n_waves;
            if (s < n_slices) request(wB, cbB, slice_begin + s);
            column_phase(wA, cbA, slice_begin + wave);
            while (s < n_slices) {            // wB holds slice s
                const int s2 = s + n_waves;
                if (s2 < n_slices) request(wA, cbA, slice_begin + s2);
                column_phase(wB, cbB, slice_begin + s);
                if (s2 >= n_slices) break;
                s = s2 + n_waves;             // wA holds slice s2
                if (s < n_slices) request(wB, cbB, slice_begin + s);
                column_phase(wA, cbA, slice_begin + s2);
            }
        }
        if (b + 1 < n_blocks) {
            if (wave < nxt.y) request(wA, cbA, nxt.x + wave);
            __syncthreads();       // the staging is read: the next block's expand may overwrite it
        }
        blk = nxt;
    }
}

template <int NV>
__global__ __launch_bounds__(1024) void spmv_tts_t_kernel(TtsDeviceMatrix M, const float* __restrict__ x, float* y, float alpha) {
    tts_t_tile<NV, false>(M, x, y, nullptr, nullptr, 0, alpha, 0.0f, (int)blockIdx.x);
}

template <int NV>
__global__ __launch_bounds__(1024) void value_grad_tts_kernel(TtsDeviceMatrix M, const int32_t* __restrict__ map, const float* __restrict__ gy,
                                                              const float* __restrict__ x, float* grad, long long n, float alpha, float beta) {
    tts_t_tile<NV, true>(M, gy, grad, x, map, n, alpha, beta, (int)blockIdx.x);
}

// tts_nv_lds_bytes(m, nv, false) of hispmv_kernels.hip: per vector the accumulators, one staging area (the largest block of the matrix in
// whole chunks + 64) and the forward kernel's 64 tails, which these kernels leave unused -- the bound is the forward one on purpose
size_t nv_lds_bytes(const TtsDeviceMatrix& m, int nv) { return ((size_t)m.acc_floats + (size_t)m.batch_stage_floats + 64) * nv * sizeof(float); }
size_t pass_lds_bytes(const TtsDeviceMatrix& m, int nv) { return nv > 1 ? nv_lds_bytes(m, nv) : tts_tile_lds_bytes(m); }

// what every launch of this file checks before it starts a grid: the stream is accepted and the pass fits
bool pass_ok(const TtsDeviceMatrix& m, int nv) {
    if (nv != 1 && nv != 2 && nv != 4) return false;
    if (!tts_t_accepts(m) || m.n_tiles <= 0) return false;
    if (nv > 1 && tts_t_width(m, nv) != nv) return false;
    return (int64_t)m.cols * nv < (1 << 30) && (int64_t)m.rows * nv < (1 << 30);
}

}  // namespace

bool tts_t_accepts(const TtsDeviceMatrix& m) {
    return m.zero_fill == 0 && m.threads >= 64 && m.threads <= 1024 && (m.threads & 63) == 0 && m.acc_floats > 0 && m.staging_floats >= kChunkSlots &&
           tts_tile_lds_bytes(m) <= (size_t)kDynLdsMax && m.words && m.col_base && m.flags && m.chunk_info && m.tiles && m.blocks &&
           (m.n_fix == 0 || m.fix);
}

int tts_t_width(const TtsDeviceMatrix& m, int64_t vecs) {
    if (vecs < 2 || m.zero_fill || m.batch_stage_floats < kChunkSlots) return 1;
    for (int nv = 4; nv >= 2; nv >>= 1) {
        if (nv > vecs) continue;
        if ((int64_t)m.cols * nv >= (1 << 30) || (int64_t)m.rows * nv >= (1 << 30)) continue;
        if (nv_lds_bytes(m, nv) <= (size_t)kDynLdsMax) return nv;
    }
    return 1;
}

hipError_t launch_tts_t(const TtsDeviceMatrix& m, int nv, const float* x, float* y, float alpha, hipStream_t stream) {
    (void)hipGetLastError();
    if (m.n_tiles <= 0 && tts_t_accepts(m)) return hipSuccess;
    if (!pass_ok(m, nv)) return hipErrorInvalidValue;
    const auto go = [&](auto kernel) {
        const hipError_t e = raise_lds_limit<kernel()>();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kernel(), dim3((unsigned)m.n_tiles), dim3((unsigned)m.threads), pass_lds_bytes(m, nv), stream, m, x, y, alpha);
        return hipGetLastError();
    };
    switch (nv) {
        case 4: return go([] { return spmv_tts_t_kernel<4>; });
        case 2: return go([] { return spmv_tts_t_kernel<2>; });
        default: return go([] { return spmv_tts_t_kernel<1>; });
    }
}

hipError_t launch_tts_value_grad(const TtsDeviceMatrix& m, int nv, const int32_t* map, const float* gy, const float* x, float* grad, int64_t n,
                                 float alpha, float beta, hipStream_t stream) {
    (void)hipGetLastError();
    if ((m.n_tiles <= 0 && tts_t_accepts(m)) || n <= 0) return hipSuccess;
    if (!map || !pass_ok(m, nv)) return hipErrorInvalidValue;
    const auto go = [&](auto kernel) {
        const hipError_t e = raise_lds_limit<kernel()>();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kernel(), dim3((unsigned)m.n_tiles), dim3((unsigned)m.threads), pass_lds_bytes(m, nv), stream, m, map, gy, x, grad, (long long)n,
                           alpha, beta);
        return hipGetLastError();
    };
    switch (nv) {
        case 4: return go([] { return value_grad_tts_kernel<4>; });
        case 2: return go([] { return value_grad_tts_kernel<2>; });
        default: return go([] { return value_grad_tts_kernel<1>; });
    }
}

}  // namespace hispmv
