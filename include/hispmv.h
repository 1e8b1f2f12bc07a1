/* hispmv.h -- C ABI of libhispmv.so, the MI355X (gfx950) drop-in for the SpMV hot path of
 * mfkiwl/HiSpMV:  y = alpha * A * x + beta * bias,  A sparse (slice stream) or dense (GeMV overlay).
 *
 * Every entry point replaces one piece of the reference's pybind11 class FpgaHandle
 * (pyhispmv/include/fpga_handle.h:9-74, pyhispmv/src/fpga_handle.cpp, bound in
 * pyhispmv/src/pyhispmv_bindings.cpp:3-39).  The reference-side binding a maintainer
 * would write against this header is shown in INTEGRATION.md.
 *
 * Conventions: plain pointers and sizes only; all functions return 0 (or a handle index
 * >= 0) on success, HISPMV_FULL (-1) where the reference returns -1, and another negative
 * HISPMV_E* code otherwise -- never exit(), never a C++ exception across the boundary
 * (the reference calls std::exit on device errors, fpga_handle.cpp:58-64,82-88,267-270).
 * hispmv_last_error() gives the message.  Calls on one context are serialised internally.
 * Host pointers are borrowed for the duration of the call only.
 */
#ifndef HISPMV_H
#define HISPMV_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HISPMV_OK          0
#define HISPMV_FULL       -1   /* matrix does not fit the arena (fpga_handle.cpp:192-195,235-238) */
#define HISPMV_EINVAL     -2   /* bad argument (negative device id, empty path, bad shape, index out of range) */
#define HISPMV_EDEVICE    -3   /* HIP runtime error / no gfx950 device */
#define HISPMV_ESTATE     -4   /* call out of order (run before load/select) */
#define HISPMV_ENOTDENSE  -5   /* dense handle requested on a context created without dense_overlay (spmv-helper.cpp:718) */
#define HISPMV_EIO        -6   /* MatrixMarket file unreadable / malformed */
#define HISPMV_ENOMEM     -7
#define HISPMV_ENOTSUP    -8   /* the handle's device format has no kernel for the operation (hispmv_spmv_device_t, hispmv_value_grad_device on a tile stream) */

typedef struct hispmv_ctx hispmv_ctx;

/* ---- FpgaHandle::FpgaHandle (fpga_handle.cpp:40-154; bindings :8-12) -------------------------
 * xclbin_path is accepted for signature compatibility; it must be non-empty (fpga_handle.cpp:70-71)
 * but is not opened.  device_id is the HIP device ordinal; negative is an error (:51-52).
 * The hardware tuple (num_ch_A.. row_dist_net) is recorded: dense_overlay gates
 * hispmv_create_dense_handle exactly as in the reference, num_ch_A sizes the default arena
 * (num_ch_A x 256 MiB, fpga_handle.h:12) unless HISPMV_ARENA_BYTES / hispmv_set_arena_bytes overrides it. */
int hispmv_create(hispmv_ctx** out, const char* xclbin_path, int device_id,
                  int num_ch_A, int num_ch_B, int num_ch_C, int urams_per_pe, int fp_acc_latency,
                  int dense_overlay, int pre_accumulator, int row_dist_net);

/* The reference never frees its handles (fpga_handle.cpp:177,220); we do. */
void hispmv_destroy(hispmv_ctx* ctx);

/* Message of the last failing call on ctx (or of the last failing hispmv_create when ctx is NULL). */
const char* hispmv_last_error(const hispmv_ctx* ctx);

/* Arena budget in bytes shared by all handles of the context ("-1 when full" contract). */
int hispmv_set_arena_bytes(hispmv_ctx* ctx, int64_t bytes);
int64_t hispmv_arena_bytes_used(const hispmv_ctx* ctx);

/* ---- FpgaHandle::createSparseMtxHandle (fpga_handle.cpp:156-207; bindings :20-23) --------------
 * COO triplets, unsorted and duplicated entries allowed (duplicates are summed by the
 * multiply, not coalesced -- spmv-helper.cpp:139-227).  Returns the handle index (0,1,2.. in
 * creation order), HISPMV_FULL, or an error. */
int hispmv_create_sparse_handle(hispmv_ctx* ctx, const int32_t* coo_rows, const int32_t* coo_cols,
                                const float* coo_values, int64_t nnz, int32_t rows, int32_t cols);

/* HiSpmvHandle::prepareSparseMtxForFPGA(mtx_file) (spmv-helper.cpp:642-646): MatrixMarket
 * coordinate file.  flavor 0 = common/ loader semantics (spmv-helper.cpp:34-136), 1 = cpu/ loader
 * semantics (cpu/src/helper_functions.cpp:91-146). */
int hispmv_create_sparse_handle_from_mtx(hispmv_ctx* ctx, const char* mtx_path, int flavor);

/* CSR input (what cpu/src/main.cpp:26-33 hands MKL): row_ptr[rows+1] starting at 0 and non-decreasing, columns inside
 * [0, cols).  Rows whose columns are not ascending (scipy: has_sorted_indices == False) are sorted by column on the
 * way in (stably: duplicates keep their order); NULL col_idx / values with nnz > 0 -> HISPMV_EINVAL. */
int hispmv_create_sparse_handle_from_csr(hispmv_ctx* ctx, const int32_t* row_ptr, const int32_t* col_idx,
                                         const float* values, int32_t rows, int32_t cols);

/* ---- FpgaHandle::createDenseMtxHandle (fpga_handle.cpp:209-250; bindings :15-18) ---------------
 * Row-major rows x cols fp32. */
int hispmv_create_dense_handle(hispmv_ctx* ctx, const float* flattened_dense_values, int32_t rows, int32_t cols);

/* ---- FpgaHandle::loadMatrices (fpga_handle.cpp:252-264) -----------------------------------------
 * Uploads every handle created so far to HBM.  Idempotent (the reference corrupts its offsets
 * when called twice, :259-261 -- not replicated). */
int hispmv_load_matrices(hispmv_ctx* ctx);

/* ---- FpgaHandle::selectMatrix (fpga_handle.cpp:266-283) -----------------------------------------
 * Out of range -> HISPMV_EINVAL (reference: exit, :267-270). */
int hispmv_select_matrix(hispmv_ctx* ctx, uint32_t matrix_idx);

/* ---- FpgaHandle::runKernel (fpga_handle.cpp:286-321) --------------------------------------------
 * y = alpha * A * x + beta * bias for the selected matrix; x[cols], bias[rows] read-only,
 * y[rows] written; blocking.  bias is not read when beta == 0 (BLAS/MKL convention, cpu/src/main.cpp:39). */
int hispmv_run_kernel(hispmv_ctx* ctx, const float* x, const float* bias, float* y, float alpha, float beta);

/* ---- FpgaHandle::runLinear (fpga_handle.cpp:323-388) --------------------------------------------
 * alpha = beta = 1; num_vecs = x_len / cols; y_out[num_vecs * rows]; same bias for every vector;
 * independent of the select_matrix state. */
int hispmv_linear(hispmv_ctx* ctx, int matrix_idx, const float* x, int64_t x_len, const float* bias, float* y_out);

/* ---- device-resident entry points (no counterpart in the reference, whose vectors always cross
 * PCIe -- fpga_handle.cpp:306-320).  d_* are device pointers; the launch is asynchronous on
 * `stream` (a hipStream_t).  ONE rule for every entry point that takes a stream (hispmv_spmv_device, hispmv_spmv_device_batch,
 * hispmv_boundary_pack, hispmv_boundary_apply): NULL = the context's own stream (created non-blocking: it does NOT synchronise
 * with HIP's null stream), anything else = the caller's stream.  Work issued with NULL is ordered with other NULL work of the
 * same context; hispmv_synchronize waits for it.  Used by bench.py and the multi-GPU driver. */
int hispmv_spmv_device(hispmv_ctx* ctx, int matrix_idx, const float* d_x, const float* d_bias, float* d_y,
                       float alpha, float beta, void* stream);
/* Waits for the context's stream and for the last caller-supplied stream a launch of this context went to, then reports
 * a device-side error of those launches (HISPMV_EDEVICE: an in-kernel bounded wait expired).  Launches sent to OTHER
 * caller streams before that must be synchronised by the caller first. */
int hispmv_synchronize(hispmv_ctx* ctx);

/* Whole-kernel device time of the last hispmv_spmv_device/run_kernel/linear launch sequence,
 * measured with HIP events on the launch stream (milliseconds); negative if unavailable. */
float hispmv_last_kernel_ms(hispmv_ctx* ctx);

/* Diagnostics of the HIP-graph replay of hispmv_spmv_device_batch (HISPMV_BATCH_GRAPH=1; plain launches by default): out = {graphs instantiated, alpha patches applied to an
 * instantiated graph}.  A call signature (handles, vectors, beta) is captured and instantiated ONCE; calls that differ only
 * in alpha patch the graph's kernel nodes (hipGraphExecKernelNodeSetParams) instead of instantiating again. */
int hispmv_batch_graph_stats(hispmv_ctx* ctx, int64_t out[2]);
/* How the LAST hispmv_spmv_device_batch call of this context was issued (diagnostics; bench.py names the kernels of its step from
 * it): out = {launches of the call, 1 if its slice groups and tiles ran as items of the step kernel's queue (one persistent
 * workgroup per CU, hispmv_kernels.hip: spmv_step_kernel, its HALF = 1 instantiation for a call with half groups under
 * hispmv_set_step_half), items of that queue, HIP streams the main launches were spread over}.
 * HISPMV_ESTATE before the first batch call. */
int hispmv_batch_call_info(hispmv_ctx* ctx, int64_t out[4]);
/* Batch calls with bf16 handles through the step kernel (opt-in, default OFF; HISPMV_STEP_HALF=1 sets the same flag when the context is
 * created).  enable: 0 or 1; anything else, or a NULL context, is HISPMV_EINVAL (checked before any device call).
 * OFF: a batch call that holds a part with half groups (a bf16 handle whose slice layout has compact groups, hispmv_set_value_storage)
 * runs as separate grids on two lanes, whatever else it holds.  ON: such a call qualifies for the step kernel under the same
 * conditions as a call of fp32 handles (HISPMV_STEP_KERNEL not 0, the call shares the chip, 1024- or 256-thread slice plans and
 * standard tile streams, no dense handle); it is planned from the parts' batch layouts and runs hispmv_kernels.hip:
 * spmv_step_kernel<., HALF = 1>, whose slice items read half, compact and wide groups -- hispmv_batch_call_info then reports it like
 * any step call.  A call WITHOUT half groups takes spmv_step_kernel<., HALF = 0> in either state.  HISPMV_STEP_KERNEL=0 still wins.
 * A batch call issued after the setter runs under the new state: the state is part of the key of the cached batch plans, so a
 * plan built under the other state is not reused (and stays valid for work still in flight).
 * The result bits are those of the grids: every item runs the body the grids run, on the same slices in the same order. */
int hispmv_set_step_half(hispmv_ctx* ctx, int enable);

/* n independent SpMVs y_i = alpha*A_i*x_i + beta*bias_i on loaded handles idx[i] in as few launches as possible: the
 * workgroups of all matrices with the same workgroup size share ONE grid (plus one fix-up launch), so small matrices no
 * longer pay 6-20 us of launch latency each (no reference counterpart: the reference runs one matrix at a time,
 * fpga_handle.cpp:286-321).  idx, d_x, d_bias, d_y are HOST arrays of n entries (device pointers inside); the y_i must
 * be distinct and a sparse handle may appear only once (its carry buffers belong to the handle).  Rows cut by slice
 * boundaries always take the fix-up variant here, so a result may differ in the last
 * bit from hispmv_spmv_device on a matrix whose single launch uses the look-back variant.  Asynchronous on `stream`. */
int hispmv_spmv_device_batch(hispmv_ctx* ctx, int32_t n, const int32_t* idx, const float* const* d_x,
                             const float* const* d_bias, float* const* d_y, float alpha, float beta, void* stream);
/* One call of a signature in flight at a time: the step kernel's queue state belongs to the cached plan of a call signature
 * (handles, vectors, beta), so the same signature must not run on two streams at once, nor from a caller-captured graph replayed
 * concurrently.  Value updates (below) follow the same ordering rule: they are ordered on their stream only. */

/* ---- in-place value updates (no reference counterpart; MKL mkl_sparse_?_update_values, hipSPARSE SpMatSetValues) ------------
 * A handle keeps its sparsity pattern, plan and device addresses; only its values change, in place: cached batch plans, step-kernel
 * queues and captured graphs stay valid.  Context-wide switch, default off: sparse and dense handles created while it is on carry
 * a VALUE MAP (4 bytes per value slot of their device layouts, charged to the arena: HISPMV_FULL covers it); handles created
 * while it is off are exactly as before.  Values come in the order of the creation input: the COO arrays of
 * hispmv_create_sparse_handle (duplicates included), col_idx / values of _from_csr BEFORE its per-row sort, W row-major for a
 * dense handle.  hispmv_create_sparse_handle_from_mtx refuses (HISPMV_EINVAL) while the switch is on: its reader drops zeros and
 * mirrors symmetric entries.  So do the tile-stream experiments HISPMV_TTS_GEOMETRY (other than standard) and HISPMV_TTS_SMALL.
 * `enable` has three states.  HISPMV_VALUE_UPDATES_OFF; HISPMV_VALUE_UPDATES_ON: as above, and creating a handle while bf16 value
 * storage is on as well is refused (HISPMV_EINVAL, see hispmv_set_value_storage); HISPMV_VALUE_UPDATES_ANY_STORAGE: fp32 handles
 * exactly as under _ON (same layouts, map, device bytes), and a bf16 handle, sparse or dense, is accepted and becomes updatable.  Any
 * other non-zero value means _ON.  An update of a bf16 handle takes fp32 values and ROUNDS THEM ON THE DEVICE with the R of
 * hispmv_set_value_storage (nearest bfloat16, ties to even; +-Inf stay, a finite value above the largest bf16 becomes Inf, a NaN a
 * quiet NaN with its sign, subnormals as bf16 has them): afterwards every entry returns the bits of a fresh bf16 handle created from
 * those values.  Its map has the words of the fp32 handle of the same input; its device bytes are those of the plain bf16 handle
 * plus the map and its chunk table. */
#define HISPMV_VALUE_UPDATES_OFF 0
#define HISPMV_VALUE_UPDATES_ON 1
#define HISPMV_VALUE_UPDATES_ANY_STORAGE 2
int hispmv_set_value_updates(hispmv_ctx* ctx, int enable);
/* n = the number of values of the creation input.  HISPMV_ESTATE: the handle is not updatable or not loaded; HISPMV_EINVAL: wrong
 * n, NULL values, bad index.  Host values: returns when the device layout holds them (pinned staging, one copy, one launch). */
int hispmv_update_values(hispmv_ctx* ctx, int matrix_idx, const float* values, int64_t n);
/* Device values: asynchronous and ordered on `stream` (NULL = the context's stream, as for hispmv_spmv_device): a later SpMV on the
 * same stream sees the new values.  Ordering against work on OTHER streams (an SpMV still reading the old values, the producer of
 * d_values) is the caller's job. */
int hispmv_update_values_device(hispmv_ctx* ctx, int matrix_idx, const float* d_values, int64_t n, void* stream);
/* out = {1 if the handle is updatable, n an update takes, map slots, slots written per update (more than the map slots where a
 * batch layout holds a second copy of the slices)}; zeros for a handle that is not updatable. */
int hispmv_value_update_info(const hispmv_ctx* ctx, int matrix_idx, int64_t out[4]);

/* ---- bf16 value storage (no reference counterpart; the 16-bit value types of rocSPARSE / hipBLASLt are the analogue) -------------
 * Context-wide switch, default HISPMV_VALUES_FP32, may be flipped between creations: a sparse or dense handle created (COO, CSR or
 * MatrixMarket) while it is HISPMV_VALUES_BF16 computes  y = alpha * R(A) * x + beta * bias,  where R rounds every stored value of A
 * ONCE, at creation, to bfloat16 (nearest, ties to even; +-Inf stay, a finite value above the largest bf16 becomes Inf, NaN stays a
 * quiet NaN; duplicated COO entries are rounded one by one).  x, bias, y, alpha, beta, every product and every sum stay fp32, in the
 * order of an fp32 handle: the result equals, bit for bit, that of an fp32 handle created from the pre-rounded values.  Format choice
 * and launch plan do not depend on the storage.  Where a layout has a kernel that reads 16-bit values its bytes shrink -- compact
 * slice groups (6 -> 4 bytes per element, stray-slot groups included), dense W (4 -> 2) --; wide groups, plans without a window and
 * the tile stream keep 32-bit slots that hold R(v).  Unknown storage or NULL context -> HISPMV_EINVAL.  Creating a handle while
 * value updates (HISPMV_VALUE_UPDATES_ON) AND bf16 storage are both on -> HISPMV_EINVAL (the value map lives in 32-bit slots);
 * HISPMV_VALUE_UPDATES_ANY_STORAGE is the opt-in under which such a handle is created, with its map read on the host. */
#define HISPMV_VALUES_FP32 0
#define HISPMV_VALUES_BF16 1
int hispmv_set_value_storage(hispmv_ctx* ctx, int storage);
/* out = {storage of the handle, value slots held in 2 bytes, value slots held in 4 bytes, device bytes the handle saves against
 * fp32 storage}; the slices of a batch layout count again (as in hispmv_value_update_info). */
int hispmv_value_storage_info(const hispmv_ctx* ctx, int matrix_idx, int64_t out[4]);

/* ---- transposed product (no reference counterpart; MKL SPARSE_OPERATION_TRANSPOSE, hipSPARSE HIPSPARSE_OPERATION_TRANSPOSE) ----------
 *   y[cols] = alpha * A^T * x[rows] + beta * bias[cols]
 * on a loaded handle: hispmv_spmv_device with the roles of the two dimensions exchanged -- d_x holds `rows` floats, d_bias and d_y
 * `cols`.  Device pointers, asynchronous on `stream` (the stream rule above: NULL = the context's stream).  Nothing is stored for it:
 * the kernels read the layout the forward product reads (the row of a slice element is its slice's row base plus the row ends before
 * it, its column is the meta), so a value update is seen by both products and the handle uses no extra arena bytes.
 *  - beta == 0: bias is not read and may be NULL, y is overwritten.  alpha == 0: y is exactly beta * bias.
 *  - d_bias == d_y is allowed.  d_x == d_y, a NULL d_x or d_y, a NULL d_bias with beta != 0 -> HISPMV_EINVAL; before
 *    hispmv_load_matrices -> HISPMV_ESTATE.  The argument checks come before any device call.
 *  - d_y must be ordinary device memory (hipMalloc, a torch tensor: coarse-grained).  The adds into y are hardware float atomics
 *    without a compare-and-swap fall-back; on fine-grained or host-pinned memory they are not guaranteed to land.  The forward
 *    entries store plainly and have no such precondition; d_x and d_bias are only read and may live anywhere the device can read.
 *  - A bf16 handle multiplies with its stored (rounded) values.
 *  - ZERO SLOTS: a stored slot whose value is +-0 contributes nothing, whatever x holds.  That covers the zero-valued fillers of empty
 *    rows, the row extensions of aligned slices, tail padding and explicit zeros of the input: an Inf or NaN in x[empty row] does not
 *    reach any y[col] (0 * Inf would), and neither does one in x[r] through an explicit zero a_rc.
 *  - ORDER: the sums into one y[col] arrive through float atomic adds, in no fixed order.  The result may differ in the last bits
 *    from run to run and from the forward product of a handle created from the swapped COO; this entry does not keep the bit-for-bit
 *    promises of the forward entries.  The handle's own state (carries, tickets, cached batch plans) is not touched.
 *  - ACCEPTED: every slice-stream handle (all its parts: column tiles, band tiles, stray split), every dense handle, and a sparse
 *    handle whose device format is the transposed tile stream (hispmv_matrix_info.format == 1) when it was created under
 *    hispmv_set_transposable(ctx, HISPMV_TRANSPOSABLE_KEEP_FORMAT) and is one part with stream words for every row (the standard
 *    geometry and HISPMV_TTS_SMALL).  Such a handle runs the forward tile kernel backwards: x of a tile's rows in the LDS, expanded to
 *    the block's row-major slots, scattered in column order -- the 64 atomics of a wave-instruction go to 64 consecutive columns of
 *    the block's sort (hispmv_matrix_info.tts_lines_per_gather lines of y).  The carries of its cut rows are neither read nor written.
 *    A tile stream created in state OFF -> HISPMV_ENOTSUP, and the message names both remedies (states SLICES and KEEP_FORMAT of
 *    hispmv_set_transposable); the tall, tallgap and paired geometries (HISPMV_TTS_GEOMETRY) -> HISPMV_ENOTSUP in every state, and
 *    the message names the geometry.
 * Out of scope: transposed calls inside hispmv_spmv_device_batch or the step kernel, host-pointer entries, sharding over devices,
 * the tall, tallgap and paired tile-stream geometries.  Several vectors per pass: hispmv_linear_device_t below. */
int hispmv_spmv_device_t(hispmv_ctx* ctx, int matrix_idx, const float* d_x, const float* d_bias, float* d_y,
                         float alpha, float beta, void* stream);
/* Context-wide switch of four states, default OFF, may be flipped between creations (like hispmv_set_value_storage); the state is
 * taken per handle at its creation.
 *   HISPMV_TRANSPOSABLE_SLICES (1): a sparse handle created in this state keeps the slice stream -- the format choice of that
 *     creation is the one HISPMV_FORMAT=slices makes for a whole process -- and is therefore accepted by hispmv_spmv_device_t.
 *   HISPMV_TRANSPOSABLE_KEEP_FORMAT (2): a sparse handle created in this state keeps the loader's own format choice, and if that is a
 *     tile stream the transposed and gradient entries accept it (see ACCEPTED above).  Nothing is stored for it: device_bytes of the
 *     handle is what it is in state OFF.
 *   HISPMV_TRANSPOSABLE_COMPANION (3): a sparse handle created in this state is what state KEEP_FORMAT makes it, and owns a STORED
 *     TRANSPOSE besides (the "companion", below): the transposed entries then issue no atomic.
 * Nothing else about the handle changes.  A handle created in state OFF that happens to be a slice stream is transposable all the
 * same, and so is every dense handle.  Any other value of `enable` -> HISPMV_EINVAL. */
#define HISPMV_TRANSPOSABLE_OFF 0
#define HISPMV_TRANSPOSABLE_SLICES 1
#define HISPMV_TRANSPOSABLE_KEEP_FORMAT 2
#define HISPMV_TRANSPOSABLE_COMPANION 3
int hispmv_set_transposable(hispmv_ctx* ctx, int enable);
/* ---- the stored transpose (HISPMV_TRANSPOSABLE_COMPANION) ---------------------------------------------------------------------------
 * The companion of a sparse handle is a second, hidden matrix for A^T, made by the ordinary creation path from the SWAPPED INPUT: for
 * the entries (rows[k], cols[k], values[k]) of a rows x cols input it is (cols[k], rows[k], values[k]) with dimensions cols x rows --
 * the same entry order k, duplicates and explicit zeros kept.  hispmv_create_sparse_handle_from_csr expands row_ptr to the row of
 * every entry in input order (before its per-row sort), so entry k is entry k of the documented value order; _from_mtx swaps the
 * entries its reader produced (and stays refused together with value updates).  The companion is created under the context's format
 * options, value storage and value-updates switch as they stand at that creation, and may come out as a slice stream, a cut matrix
 * (column tiles, band tiles, stray split) or a standard-geometry tile stream; it builds no batch layout, since it is never part of a
 * batch call.  It is not a handle: indices, hispmv_num_matrices and creation order are what they are without it.  Dense handles
 * ignore the state.  Creation in this state under HISPMV_TTS_GEOMETRY other than standard or under HISPMV_TTS_SMALL -> HISPMV_EINVAL.
 *  - ARENA: device_bytes (and prep_seconds) of the handle is the sum of both, the companion's value map and chunk table included on an
 *    updatable handle.  The capacity check runs once, on the sum: when it does not fit, creation returns HISPMV_FULL, nothing is
 *    registered or charged and the context is as before the call.  hispmv_value_storage_info and the plan fields of
 *    hispmv_get_matrix_info describe the handle's own layouts, as without a companion.
 *  - LOAD: hispmv_load_matrices uploads the companion with its owner and, on an updatable handle, builds its value map the same way.
 *  - UPDATES: hispmv_update_values(_device) takes the same n values in the same order and writes the handle's layouts, its batch layout
 *    and the companion's layouts on the call's stream.  hispmv_value_update_info out[3] includes the companion's slots, out[1] is n.
 *  - TRANSPOSED ENTRIES: hispmv_spmv_device_t and hispmv_linear_device_t on such a handle run the forward launches over the companion.
 *    Their argument checks are unchanged.  In place of the ORDER, ZERO SLOTS and "ordinary device memory" clauses above:
 *      BITS: for every vector v, y_v has the bits of a one-vector hispmv_linear_device call (the fix-up carry variant) on a handle
 *        created from the swapped input under the same switches, with bias_v, alpha and beta -- whatever the batch around the vector,
 *        and from run to run.
 *      ZERO SLOTS and non-finite inputs behave as in that forward product: the rule "a +-0 slot adds nothing" of the atomics route
 *        does NOT apply (0 * Inf is NaN here, as in every forward call).
 *      alpha == 0 still gives exactly beta * bias per vector through the prologue launch and reads neither x nor the matrix;
 *        beta == 0 does not read the bias.  bias_stride = cols and d_bias == d_y keep working: every y element's bias is read by the
 *        thread that stores it.
 *      WIDTHS: the vectors go in passes of the widths hispmv_linear_device takes on the companion for beta != 0 -- 4, 2, 1 on a slice
 *        stream or cut matrix, the tile-stream rules on a tile stream -- for beta == 0 too.  A per-vector bias on a tile-stream
 *        companion takes one vector per launch (the batched tile kernel takes one shared bias).  A d_x that is not 16-byte aligned,
 *        or rows % 4 != 0 where the companion's plan has a window, falls to width 1, with the same bits.
 *      d_y may be any memory the device can write: the stores are plain.
 *      OWNERSHIP: the companion's carries and partial vectors belong to the handle, so ONE transposed call per handle may be in
 *        flight.  A forward and a transposed call on the same handle may overlap: they use separate matrices, carries and partial
 *        vectors.  hispmv_value_grad_device reads only the handle's own layouts and is unchanged.
 *  - hispmv_transpose_info reports {1, launches of a one-vector call, 0, 0}; hispmv_linear_info reports the companion route's widest
 *    pass, passes and launches (shared bias, aligned d_x) in its three transposed fields.  For a cut companion's one-vector passes the
 *    launch figure is that of a batch call of one matrix: one grid per workgroup size among its parts, plus its tail.
 * There is no per-call choice between the two routes, and no companion inside hispmv_spmv_device_batch.
 * hispmv_companion_info: out = {1 if the handle owns a companion, its format (hispmv_matrix_info.format), its parts, its device bytes,
 * its value map slots, its tile kind (hispmv_matrix_info.tile_kind)}; zeros for a handle without one. */
int hispmv_companion_info(const hispmv_ctx* ctx, int matrix_idx, int64_t out[6]);
/* out = {1 if hispmv_spmv_device_t accepts the (loaded) handle; launches of one call with alpha != 0 (the prologue y = beta * bias +
 * one per part); bytes of float atomic adds to y per call (window flushes + stray flushes + direct adds); stream elements that add
 * to y directly, one atomic each (elements outside their group's window, every stored slot -- fillers included, which add nothing
 * at run time -- of a group or plan without a window)}.  The flushes are 256 contiguous bytes per wave-instruction, the cheap shape;
 * the direct adds scatter over up to 64 lines per wave-instruction, the expensive one.  An accepted tile stream reports {1, 1 + 1,
 * 4 * nnz, nnz}, nnz the stored words that are neither filler nor padding: upper bounds, since a word whose value is +-0 (an explicit
 * zero) issues no atomic; its adds touch tts_lines_per_gather lines per wave-instruction.  Zeros for a handle that is not
 * transposable or not loaded.  A handle with a stored transpose: {1, launches of a one-vector call over it, 0, 0} (see above). */
int hispmv_transpose_info(const hispmv_ctx* ctx, int matrix_idx, int64_t out[4]);

/* ---- several vectors on device pointers (no reference counterpart: FpgaHandle::runLinear takes host vectors and relaunches per
 * vector, fpga_handle.cpp:323-388) --------------------------------------------------------------------------------------------------
 * The device-pointer forms of hispmv_linear and of hispmv_spmv_device_t for num_vecs vectors that lie one after the other, row-major
 * and contiguous -- [num_vecs, cols] and [num_vecs, rows], the layout of a torch batch.  Asynchronous on `stream` (the stream rule
 * above: NULL = the context's stream).  The argument checks come before any device call: NULL context, num_vecs < 1, NULL d_x or d_y,
 * NULL d_bias with beta != 0, d_x == d_y -> HISPMV_EINVAL; rows * num_vecs or cols * num_vecs >= 2^30 -> HISPMV_EINVAL (the message
 * says to split the batch); before hispmv_load_matrices -> HISPMV_ESTATE.
 *
 *   hispmv_linear_device:    y[v*rows + i] = alpha * (A x_v)[i] + beta * bias[i],   x_v = d_x + v*cols,   one bias for all vectors
 *  - Every loaded handle is accepted, tile streams included.  It is the launch sequence of hispmv_linear on the caller's stream: up to
 *    4 (slice stream) or 8 (dense, tile stream) vectors share a pass over the matrix, rows cut by slice boundaries always take the
 *    fix-up variant.  With alpha = beta = 1 the result has the bits of hispmv_linear, and every vector the bits of a one-vector call
 *    of this entry, whatever the batch around it.
 *  - With beta == 0 a slice stream takes one vector per pass (the batched slice kernel reads a bias); hispmv_linear_info reports the
 *    passes for beta != 0 only.
 *  - ALIGNMENT OF d_x.  The window staging of the slice kernels and the dense and tile-stream passes read x with 16-byte loads at
 *    x_v + a multiple of 16 floats -- the single-vector kernels as well as the multi-vector ones.  With several vectors the address of
 *    vector v also depends on v * cols, which is why the batched slice pass asks for cols % 4 == 0 where the plan has a window.  A d_x
 *    that is not 16-byte aligned is not refused: the call then takes one vector per pass, with the same bits.  That keeps such a call
 *    on the launches hispmv_spmv_device makes for the same pointer; it does not make the 16-byte loads aligned.  They are global
 *    loads, which gfx950 executes at any 4-byte address (tests pass a d_x shifted by one float through both routes); an aligned d_x
 *    (hipMalloc, a torch tensor) is the layout the kernels were written and timed for.
 *  - OWNERSHIP, as for hispmv_spmv_device_batch: the carries of cut rows and the partial vectors of column parts belong to the handle,
 *    so one call per handle may be in flight; a second call on the same handle must be ordered behind the first (same stream, or an
 *    event).
 *
 *   hispmv_linear_device_t:  y[v*cols + j] = alpha * (A^T x_v)[j] + beta * bias[v*bias_stride + j],   x_v = d_x + v*rows
 *  - bias_stride is 0 (one bias of cols floats for all vectors) or cols (one per vector); anything else -> HISPMV_EINVAL.  With
 *    bias_stride = cols, d_bias == d_y is allowed: y += alpha * A^T x per vector, in place.  (d_bias == d_y with bias_stride 0 and
 *    several vectors -> HISPMV_EINVAL: vector 0 would overwrite the bias of the others.)
 *  - The handles hispmv_spmv_device_t accepts, and its promises: a tile stream that is not accepted -> HISPMV_ENOTSUP with the same
 *    messages; zero slots
 *    add nothing; d_y must be coarse-grained device memory; the sums arrive through float atomics in no fixed order; alpha == 0 gives
 *    exactly beta * bias per vector; beta == 0 does not read the bias; the handle's state is untouched, so calls may overlap each
 *    other and forward calls.  No alignment condition on any pointer.
 *  - One prologue launch covers all vectors.  The vectors then go in passes of the widest width that fits, 4, 2, 1 on a slice stream:
 *    a pass of NV vectors keeps NV accumulator windows in the LDS, so NV is the largest of {4, 2} that is <= the vectors left and
 *    whose windows fit the LDS of a CU for every part of the handle (a plan without a window always takes 4); dense handles go 8, 4,
 *    2, 1.  A slice's words are read and decoded once per pass.  Width-1 passes are the launches of hispmv_spmv_device_t.
 *    An accepted tile stream keeps NV copies of a tile's x rows and of the staging in the LDS: NV is the largest of {4, 2} that is <=
 *    the vectors left and for which NV * (accumulators + largest block in whole chunks + 64 + 64 floats) fits the LDS of a CU -- the
 *    rule of the forward tile kernel without its x-in-LDS branch; otherwise 1.
 * Out of scope: transposed calls inside hispmv_spmv_device_batch or the step kernel, sharding over
 * devices, host-pointer variants of these two entries, and any change to the widths of the forward path.  The gradient with respect to
 * the matrix values is hispmv_value_grad_device below. */
int hispmv_linear_device(hispmv_ctx* ctx, int matrix_idx, const float* d_x, int64_t num_vecs, const float* d_bias, float* d_y,
                         float alpha, float beta, void* stream);
int hispmv_linear_device_t(hispmv_ctx* ctx, int matrix_idx, const float* d_x, int64_t num_vecs, const float* d_bias, int64_t bias_stride,
                           float* d_y, float alpha, float beta, void* stream);
/* out = {forward (beta != 0, aligned d_x): vectors of the widest pass, passes over the matrix; transposed: vectors of the widest pass,
 * passes, launches of the call (the prologue + one per part and pass)}.  Transposed figures are zeros for a tile stream that
 * hispmv_linear_device_t does not accept, all five for a handle that is not loaded. */
int hispmv_linear_info(const hispmv_ctx* ctx, int matrix_idx, int64_t num_vecs, int64_t out[5]);

/* ---- value gradient (no reference counterpart; a sampled dense-dense product: rocSPARSE / cuSPARSE SDDMM restricted to the pattern) ----
 *   grad[k] = alpha * sum_v gy[v, row_k] * x[v, col_k] + beta * grad[k]        for every k in [0, n)
 * on a loaded handle created with value updates on: the gradient of sum_v gy_v . (A x_v) with respect to the value of entry k of the
 * creation input.  d_gy is [num_vecs, rows], d_x is [num_vecs, cols], row-major and contiguous (the layouts of hispmv_linear_device
 * and hispmv_linear_device_t); d_grad holds n = hispmv_value_update_info(...)[1] floats in the ORDER OF THE CREATION INPUT, the order
 * hispmv_update_values_device reads: the COO arrays (duplicates included, each with its own, equal gradient), col_idx / values of
 * _from_csr before its per-row sort, W row-major for a dense handle.  Device pointers, asynchronous on `stream` (the stream rule
 * above: NULL = the context's stream).  Nothing is stored for it: the row of a slice element is its slice's row base plus the row ends
 * before it, its column is the meta, its input position is the value map of the handle.
 *  - beta == 0: d_grad is not read; every one of its n positions is overwritten, whatever it held (NaN included).
 *  - alpha == 0: the result is exactly beta * grad (zeros with beta == 0); gy and x are not read.  One elementwise launch.
 *  - The gradient of an entry does not depend on its value: the kernels go by the map and do not read the values at all.  An explicit
 *    zero of the input gets its gradient like every other entry (the zero-slot rule of the transposed product has no place here);
 *    slots that hold no input entry (fillers of empty rows, row extensions, padding) write nothing.
 *  - NO ATOMICS: every input entry lives in exactly one slot of the handle's first layouts, so each grad[k] has one writer per launch.
 *    The result is deterministic: the same bits from run to run.
 *  - ORDER OF THE SUMS.  On a slice stream the vectors go in passes of 4, 2, 1 by the rule of hispmv_linear_device_t (the largest of
 *    {4, 2} that is <= the vectors left and whose x windows fit the LDS of a CU for every part; a plan without a window takes 4).
 *    Inside a pass the sum s_p starts at +0 and takes the vectors ascending, every product and every add unfused.  The first pass
 *    stores alpha * s_0 (+ beta * grad), every later pass grad + alpha * s_p.  A dense handle takes all vectors in one launch:
 *    alpha * s (+ beta * grad), s summed ascending from +0.  An accepted tile stream follows the same contract with the widths
 *    hispmv_linear_device_t takes on it.
 *  - ACCEPTED: every loaded, updatable slice-stream handle (all its parts: column tiles, band tiles, stray split), every loaded,
 *    updatable dense handle, and every loaded, updatable tile stream that hispmv_spmv_device_t accepts (created in state
 *    HISPMV_TRANSPOSABLE_KEEP_FORMAT; hispmv_set_value_updates already refuses the other geometries and HISPMV_TTS_SMALL).  Not loaded
 *    -> HISPMV_ESTATE; not created with value updates on -> HISPMV_ESTATE (the message names hispmv_set_value_updates; a bf16 handle
 *    created outside HISPMV_VALUE_UPDATES_ANY_STORAGE falls under this); a tile stream that is not accepted -> HISPMV_ENOTSUP (the messages of
 *    hispmv_spmv_device_t), in this order.
 *  - The argument checks come before any device call: NULL context, num_vecs < 1, NULL d_gy or d_x, NULL d_grad with n > 0, d_grad
 *    equal to d_gy or d_x, a bad index -> HISPMV_EINVAL; rows * num_vecs or cols * num_vecs >= 2^30 -> HISPMV_EINVAL (the message says
 *    to split the batch).  No alignment condition on any pointer.
 *  - HANDLE STATE: the entry reads metas, slice headers, fragment tables, stray columns and the value map.  It does not read the values
 *    and does not touch carries, tickets or cached batch plans, so it may overlap forward, transposed and update calls on the same
 *    handle (hispmv_update_values_device writes values only).
 *  - A bf16 handle made updatable under HISPMV_VALUE_UPDATES_ANY_STORAGE is accepted like an fp32 one: its half groups are decoded for
 *    their metas only, plan, pass widths and map are those of the fp32 handle of the same input, and so is every bit of grad.
 * Out of scope: gradients inside hispmv_spmv_device_batch or the step kernel,
 * sharding over devices, host-pointer variants, passes wider than the 4-2-1 rule. */
int hispmv_value_grad_device(hispmv_ctx* ctx, int matrix_idx, const float* d_gy, const float* d_x, int64_t num_vecs, float* d_grad,
                             float alpha, float beta, void* stream);
/* out = {1 if hispmv_value_grad_device accepts the (loaded) handle, vectors of the widest pass, passes, launches of a call with
 * alpha != 0 (one per part and pass; dense: one)}.  Zeros for a handle that is not accepted or not loaded. */
int hispmv_value_grad_info(const hispmv_ctx* ctx, int matrix_idx, int64_t num_vecs, int64_t out[4]);

/* ---- wide batch on feature-major operands (no reference counterpart: the reference relaunches per vector) --------------------------
 *   hispmv_spmm_device:    yt[r, v] = alpha * sum_k a_rk * xt[k, v] + beta * bias,      r < rows, v < num_vecs
 *   hispmv_spmm_device_t:  the same with A^T: xt is [rows, ld_x], yt is [cols, ld_y]
 * d_xt is [cols, ld_x], d_yt is [rows, ld_y], row-major, ld_x, ld_y >= num_vecs >= 1: one stored element of A needs one contiguous run
 * of num_vecs floats of xt.  The 64 lanes of a wavefront are 64 * VL vectors (VL = 4, 2 or 1 consecutive vectors per lane), the stored
 * elements are walked in stream order, and the matrix stream is read once per tile of 64 * VL vectors -- hispmv_linear_device reads it
 * once per 4 vectors.  Device pointers, 4-byte aligned, asynchronous on `stream` (the stream rule above: NULL = the context's stream).
 *  - BIAS: bias_stride == 0: d_bias is one vector of rows floats, bias[r] under every vector; bias_stride == ld_y: d_bias is a matrix
 *    laid out like d_yt and may BE d_yt (yt = alpha * A xt + beta * yt in place); anything else -> HISPMV_EINVAL.  beta == 0 never reads
 *    d_bias (it may be NULL or hold NaN).  alpha == 0 gives exactly beta * bias; neither xt nor the matrix is read.
 *  - The floats num_vecs .. ld_y - 1 of a row of d_yt are not written.
 *  - ZERO SLOTS: a stored slot whose value is +-0 contributes nothing, whatever xt holds (fillers of empty rows, row extensions,
 *    padding, explicit zeros): the rule of hispmv_spmv_device_t.
 *  - BITS: no float atomics, no look-back, no waiting between workgroups.  Every yt[r, v] has exactly one writer per launch, and its
 *    sum has a fixed order: inside a slice the elements in stream order from +0; a row cut by slice boundaries is the partial sums of
 *    its slices in ascending order from +0; then alpha * sum + beta * bias, every product and add unfused.  The bits of vector v
 *    therefore depend neither on num_vecs, nor on the tile or VL that carried it, nor on the run.  They are NOT the bits of
 *    hispmv_linear_device, whose row sums come out of a segmented scan.
 *  - ACCEPTED: every loaded sparse handle whose device format is the slice stream, whatever its groups (no window, compact, wide, stray
 *    slots, half) and parts (column tiles, band tiles, the two parts of a stray split).  The parts run one after the other on the
 *    stream inside every vector tile: part 0 with the caller's beta * bias, each later part adding into d_yt in place.  A tile-stream
 *    handle -> HISPMV_ENOTSUP (the message names hispmv_set_transposable(ctx, 1), which keeps the slice stream); a dense handle ->
 *    HISPMV_ENOTSUP (a wide batch against a dense W is a GEMM).  hispmv_spmm_device_t is accepted only on a handle created in state
 *    HISPMV_TRANSPOSABLE_COMPANION whose stored transpose is a slice stream, and runs the same launches over it: per vector the bits of
 *    hispmv_spmm_device on a handle made from the swapped input; any other handle -> HISPMV_ENOTSUP (the message names the state).
 *  - WORKSPACE: d_work holds at least the bytes hispmv_spmm_info reports for (num_vecs, ld) -- per slice of the largest part, two
 *    partial sums of 64 * VL floats for the rows cut by slice boundaries -- and is the caller's: the library allocates nothing for these
 *    entries and keeps no per-handle state for them.  Two calls on one handle with two workspaces may therefore be in flight at once
 *    (unlike hispmv_linear_device); two calls that share a workspace must be ordered.  Its contents mean nothing between calls.
 *  - Errors, all before any launch: not loaded -> HISPMV_ESTATE; HISPMV_ENOTSUP as above; num_vecs < 1, ld_x or ld_y < num_vecs,
 *    work_bytes smaller than hispmv_spmm_info reports for (num_vecs, ld_x, ld_y), NULL d_xt or d_yt, NULL d_bias with beta != 0,
 *    d_xt == d_yt, d_bias == d_yt with bias_stride 0, a bad index -> HISPMV_EINVAL.
 * Out of scope: tile-stream and dense handles, a transposed wide product without a stored transpose, wide calls
 * inside hispmv_spmv_device_batch or the step kernel, sharding over devices, host-pointer variants.  (bf16 activations:
 * hispmv_spmm_device_bf16 below.) */
int hispmv_spmm_device(hispmv_ctx* ctx, int matrix_idx, const float* d_xt, int64_t num_vecs, int64_t ld_x, const float* d_bias,
                       int64_t bias_stride, float* d_yt, int64_t ld_y, float alpha, float beta, void* d_work, int64_t work_bytes, void* stream);
int hispmv_spmm_device_t(hispmv_ctx* ctx, int matrix_idx, const float* d_xt, int64_t num_vecs, int64_t ld_x, const float* d_bias,
                         int64_t bias_stride, float* d_yt, int64_t ld_y, float alpha, float beta, void* d_work, int64_t work_bytes, void* stream);
/* For num_vecs vectors with ld_x = ld_y = ld and 16-byte aligned pointers, out = {1 if hispmv_spmm_device accepts the (loaded) handle,
 * 1 if hispmv_spmm_device_t does, VL of the first vector tile, vector tiles, launches of a call with alpha != 0 (per tile and part the
 * slice grid, and the cut rows where the part has any), work_bytes of hispmv_spmm_device, work_bytes of hispmv_spmm_device_t, 0}.
 * out[2..5] describe the forward entry and are zeros where it is not accepted.  Pointers aligned to less than 16 bytes may take a
 * smaller VL (hispmv_prep_spmm_tiles) and more tiles; the workspace figures hold for every alignment.  Zeros for a handle that is not loaded. */
int hispmv_spmm_info(const hispmv_ctx* ctx, int matrix_idx, int64_t num_vecs, int64_t ld, int64_t out[8]);
/* ---- wide-batch value gradient on feature-major operands -------------------------------------------------------------------------
 *   grad[k] = alpha * sum_{v < num_vecs} gyt[row_k, v] * xt[col_k, v] + beta * grad[k]
 * for every entry k of the creation input of a loaded, updatable slice-stream handle: hispmv_value_grad_device on the operand layout of
 * hispmv_spmm_device.  d_gyt is [rows, ld_gy], d_xt is [cols, ld_x], row-major, ld_gy, ld_x >= num_vecs >= 1; the pad floats num_vecs ..
 * ld - 1 of a row are never used (they may hold NaN).  d_grad holds n floats in the order hispmv_update_values_device reads.  Grid, groups
 * and walk are those of hispmv_spmm_device: the 64 lanes of a wavefront are 64 * VL vectors and the slice stream -- its metas only: the
 * values are never touched -- is read once per tile of 64 * VL vectors, where hispmv_value_grad_device reads it once per 4 vectors.
 * Device pointers, 4-byte aligned, asynchronous on `stream` (the stream rule above: NULL = the context's stream).
 *  - beta == 0: d_grad is not read; every one of its n positions is overwritten, whatever it held.  alpha == 0: exactly beta * grad
 *    (zeros with beta == 0); gyt and xt are not read.  One elementwise launch.
 *  - An explicit zero of the input gets its gradient like every other entry (the +-0 rule of hispmv_spmm_device has no place here);
 *    slots that hold no input entry write nothing.
 *  - TILES: vector tiles go one after the other by the rule of hispmv_prep_spmm_tiles, with align_bytes the smaller alignment of d_gyt
 *    and d_xt; the first tile stores alpha * s + beta * grad, every later one grad + alpha * s.  Inside a tile the parts of the handle
 *    run one after the other, each on its own entries.  No workspace, no second launch, no atomics, nothing kept in the handle.
 *  - BITS: every grad[k] has one writer per launch.  The sum s of an entry over one tile has a fixed order: the VL products of a lane
 *    ascending from +0, every product and add unfused; then the pairwise tree over the 64 lanes (lanes 2i and 2i + 1, then pairs of
 *    pairs, ...).  Two identical calls give identical bits.  The bits depend on (num_vecs, ld, alignment) through VL and the tiles:
 *    they are NOT the bits of hispmv_value_grad_device and they are NOT independent of the batch.
 *  - ACCEPTED: every loaded, updatable handle that hispmv_spmm_device accepts -- every slice-stream group kind, column tiles, band
 *    tiles, both parts of a stray split; fp32, and bf16 created under HISPMV_VALUE_UPDATES_ANY_STORAGE (same plan, same map, same bits).
 *    Not loaded -> HISPMV_ESTATE; a dense handle -> HISPMV_ENOTSUP (this is a GEMM); a tile stream -> HISPMV_ENOTSUP (the message names
 *    hispmv_set_transposable(ctx, 1)); not created with value updates on -> HISPMV_ESTATE (the message names hispmv_set_value_updates),
 *    in this order.
 *  - Argument errors, all before any launch: num_vecs < 1, ld_gy or ld_x < num_vecs, NULL d_gyt or d_xt, NULL d_grad with n > 0, a
 *    pointer that is not 4-byte aligned, d_grad equal to d_gyt or d_xt, a bad index -> HISPMV_EINVAL.
 *  - HANDLE STATE: the entry reads metas, slice headers, fragment tables, stray columns and the value map, and writes nothing but
 *    d_grad: it may overlap forward, transposed, wide and update calls on the same handle.
 * Out of scope: tile-stream and dense handles, gradients inside hispmv_spmv_device_batch or the step kernel, sharding over devices,
 * host-pointer variants.  bf16 activations: hispmv_spmm_value_grad_device_bf16. */
int hispmv_spmm_value_grad_device(hispmv_ctx* ctx, int matrix_idx, const float* d_gyt, int64_t ld_gy, const float* d_xt, int64_t ld_x,
                                  int64_t num_vecs, float* d_grad, float alpha, float beta, void* stream);
/* out = {1 if hispmv_spmm_value_grad_device accepts the (loaded) handle, VL of the first tile, vector tiles, launches of a call with
 * alpha != 0 (one per tile and part that holds slices; 0 for a handle without entries)} for ld_gy = ld_x = ld and 16-byte aligned
 * pointers.  Zeros for a handle that is not accepted or not loaded.  num_vecs < 1 or ld < num_vecs -> HISPMV_EINVAL. */
int hispmv_spmm_value_grad_info(const hispmv_ctx* ctx, int matrix_idx, int64_t num_vecs, int64_t ld, int64_t out[4]);
/* The vector tiles of a wide call (host-only, no device needed).  A lane owns VL in {4, 2, 1} consecutive vectors and reads them with
 * one dwordx4, dwordx2 or dword load per stored element; a tile is 64 * VL vectors.  Every tile takes the largest VL such that
 *   (a) 64 * (VL / 2) < vectors left;   (b) cols * 64 * VL * 4 <= 8 MiB: VL 4 up to 8192 columns, VL 2 up to 16384 (a cap
 *   on the columns taken from a measurement at 8192, not a cache bound: DESIGN.md 2.12);   (c) ld % VL == 0 and align_bytes % (4 * VL) == 0.
 * The last tile is masked per lane.  out = {VL of the first tile, tiles, vectors in the last tile, VL of the last tile}.  cols,
 * num_vecs, ld or align_bytes < 1, or ld < num_vecs -> HISPMV_EINVAL. */
int hispmv_prep_spmm_tiles(int64_t cols, int64_t num_vecs, int64_t ld, int64_t align_bytes, int64_t out[4]);

/* ---- wide batch with bf16 activations ---------------------------------------------------------------------------------------------
 *   hispmv_spmm_device_bf16:    yt[r, v] = bf16(alpha * sum_k a_rk * xt[k, v] + beta * bias),      r < rows, v < num_vecs
 *   hispmv_spmm_device_t_bf16:  the same with A^T: xt is [rows, ld_x], yt is [cols, ld_y]
 * hispmv_spmm_device / hispmv_spmm_device_t with 2-byte operands: d_xt [cols, ld_x] and d_yt [rows, ld_y] hold bfloat16 (uint16_t: the
 * upper half of the fp32), every other argument means what it means there.  The matrix values are the handle's (fp32 or bf16 storage),
 * products and sums are fp32.  A lane owns VB = 8, 4, 2 or 1 consecutive vectors (one dwordx4, dwordx2, dword or 16-bit load per stored
 * element): a tile is 64 * VB vectors, up to 512.  Asynchronous on `stream` (the stream rule above).
 *  - BIAS: bias_stride == 0: d_bias is one vector of rows FP32 values, as in hispmv_spmm_device; bias_stride == ld_y: d_bias is a BF16
 *    matrix laid out like d_yt and may BE d_yt (in place).  beta == 0 never reads d_bias.  alpha == 0 gives exactly bf16(beta * bias).
 *  - ALIGNMENT: d_xt, d_yt and a matrix bias 2 bytes at least; d_work and a shared bias 4 bytes.  Less than 16 bytes may take a smaller VB.
 *  - The elements num_vecs .. ld_y - 1 of a row of d_yt are not written.  ZERO SLOTS as in hispmv_spmm_device.
 *  - BITS: widening a bf16 is exact, and the fp32 value of yt[r, v] before it is stored has the fixed order of hispmv_spmm_device: it is
 *    bit for bit what hispmv_spmm_device stores for the widened operands (the bias widened), whatever num_vecs, the tile or VB.  It is
 *    then rounded ONCE: nearest, ties to even; +-Inf stay; overflow becomes Inf; a NaN becomes a quiet NaN with its sign
 *    (hispmv_update_values on a bf16 handle rounds by the same rule).  A handle of several parts does not round between them: the parts
 *    add into an fp32 tile accumulator [rows, 64 * VB] in the workspace and the last part alone stores to d_yt.
 *  - ACCEPTED, refused, and every error with its code and order: as hispmv_spmm_device / hispmv_spmm_device_t.  All before any launch.
 *  - WORKSPACE: the bytes hispmv_spmm_bf16_info reports: the fp32 partial sums of hispmv_spmm_device for tiles of 64 * VB vectors, and
 *    for a handle of more than one part the tile accumulator behind them.  The caller's; nothing is kept in the handle.
 * Out of scope: bf16 activations for hispmv_value_grad_device (the wide-batch value gradient takes them: hispmv_spmm_value_grad_device_bf16
 * below), hispmv_linear_device* and the one-vector entries; tile-stream and dense handles; wide calls inside hispmv_spmv_device_batch or
 * the step kernel; sharding over devices. */
int hispmv_spmm_device_bf16(hispmv_ctx* ctx, int matrix_idx, const uint16_t* d_xt, int64_t num_vecs, int64_t ld_x, const void* d_bias,
                            int64_t bias_stride, uint16_t* d_yt, int64_t ld_y, float alpha, float beta, void* d_work, int64_t work_bytes, void* stream);
int hispmv_spmm_device_t_bf16(hispmv_ctx* ctx, int matrix_idx, const uint16_t* d_xt, int64_t num_vecs, int64_t ld_x, const void* d_bias,
                              int64_t bias_stride, uint16_t* d_yt, int64_t ld_y, float alpha, float beta, void* d_work, int64_t work_bytes, void* stream);
/* hispmv_spmm_info for the bf16 entries: out = {1 if hispmv_spmm_device_bf16 accepts the (loaded) handle, 1 if hispmv_spmm_device_t_bf16
 * does, VB of the first vector tile, vector tiles, launches of a call with alpha != 0, work_bytes of hispmv_spmm_device_bf16, work_bytes of
 * hispmv_spmm_device_t_bf16, 0} for ld_x = ld_y = ld and 16-byte aligned pointers; the workspace figures hold for every alignment. */
int hispmv_spmm_bf16_info(const hispmv_ctx* ctx, int matrix_idx, int64_t num_vecs, int64_t ld, int64_t out[8]);
/* The vector tiles of a wide call with bf16 activations (host-only).  Every tile takes the largest VB in {8, 4, 2} such that
 *   (a) 64 * (VB / 2) < vectors left;   (b) cols * 64 * VB * 2 <= 8 MiB: VB 8 up to 8192 columns, VB 4 up to 16384, VB 2 up to 32768
 *   (the bound of hispmv_prep_spmm_tiles in bytes, reused unmeasured);   (c) ld % VB == 0 and align_bytes % (2 * VB) == 0;
 * otherwise VB = 1.  out = {VB of the first tile, tiles, vectors in the last tile, VB of the last tile}.  Errors as hispmv_prep_spmm_tiles. */
int hispmv_prep_spmm_bf16_tiles(int64_t cols, int64_t num_vecs, int64_t ld, int64_t align_bytes, int64_t out[4]);
/* ---- wide-batch value gradient with bf16 activations -----------------------------------------------------------------------------
 *   grad[k] = alpha * sum_{v < num_vecs} gyt[row_k, v] * xt[col_k, v] + beta * grad[k]
 * hispmv_spmm_value_grad_device with 2-byte operands: d_gyt [rows, ld_gy] and d_xt [cols, ld_x] hold bfloat16 (uint16_t: the upper half
 * of the fp32); d_grad, alpha and beta are fp32 and every other argument means what it means there.  A lane owns VB = 8, 4, 2 or 1
 * consecutive vectors (one dwordx4, dwordx2, dword or 16-bit load per stored element and per row of gyt): a tile is 64 * VB vectors, up
 * to 512.  The pad halves num_vecs .. ld - 1 of a row are never used (they may hold NaN).  Asynchronous on `stream`.
 *  - TILES: the rule of hispmv_prep_spmm_bf16_tiles with ld_x, ld_gy and align_bytes the smaller alignment of d_gyt and d_xt (its 8 MiB
 *    bound is reused, unmeasured for this kernel); the first tile stores alpha * s + beta * grad, every later one grad + alpha * s.
 *    Inside a tile the parts of the handle run one after the other.  No workspace, no second launch, no atomics, nothing kept in the handle.
 *  - BITS: widening a bf16 is exact.  The sum s of an entry over one tile: the VB products of a lane ascending from +0, every product and
 *    add unfused, the product of a vector >= num_vecs replaced by +0; then the pairwise tree over the 64 lanes.  Where a tile has
 *    VB <= 4 and the same boundaries as a tile of hispmv_spmm_value_grad_device, its bits are those of that entry on the widened operands.
 *    Two identical calls give identical bits.
 *  - ALIGNMENT: d_gyt and d_xt 2 bytes at least, d_grad 4 bytes.  Less than 16 bytes may take a smaller VB.
 *  - ACCEPTED, refused, and every error with its code and order: as hispmv_spmm_value_grad_device.  alpha == 0: exactly beta * grad,
 *    the operands not read; a handle without entries: HISPMV_OK without a launch.
 * Out of scope: bf16 operands for hispmv_value_grad_device, a bf16 d_grad, tile-stream and dense handles. */
int hispmv_spmm_value_grad_device_bf16(hispmv_ctx* ctx, int matrix_idx, const uint16_t* d_gyt, int64_t ld_gy, const uint16_t* d_xt, int64_t ld_x,
                                       int64_t num_vecs, float* d_grad, float alpha, float beta, void* stream);
/* hispmv_spmm_value_grad_info for the bf16 entry: out = {accepted, VB of the first tile, vector tiles, launches = tiles * parts that hold
 * slices (0 for a handle without entries)} for ld_gy = ld_x = ld and 16-byte aligned pointers.  Errors as hispmv_spmm_value_grad_info. */
int hispmv_spmm_value_grad_bf16_info(const hispmv_ctx* ctx, int matrix_idx, int64_t num_vecs, int64_t ld, int64_t out[4]);

/* Time `reps` back-to-back launches of matrix_idx on the context stream with HIP events
 * (kernel-only, the reference's convention: spmv-helper.cpp:1030-1035).  Returns ms per launch. */
float hispmv_time_device(hispmv_ctx* ctx, int matrix_idx, const float* d_x, const float* d_bias, float* d_y,
                         float alpha, float beta, int reps);

/* ---- multi-GPU boundary rows (no reference counterpart: the reference is single-device) ----
 * A matrix whose element sequence is split over ranks has at most one row cut at each rank boundary.  Per step
 * every rank publishes, for each of its n matrices, the last entry of its local y when that row continues on the
 * next rank (its "tail"), the tails are all-gathered (torch.distributed / RCCL), and each rank adds the chain of
 * tails that feeds its first row.  These two launches are the device side of that step on `stream`:
 *   pack:  send[i] = mask[i] * *last[i]                                   (last[i] may be NULL: 0)
 *   apply: *first[i] += sum_r recv[r*n + i] * weights[i*world + r]        (first[i] NULL: nothing), r ascending
 * All pointers are device pointers (last/first: device arrays of n device pointers).  `stream` as everywhere in this header:
 * NULL = the context's stream, so SpMVs and boundary kernels issued with NULL run on one queue, in order. */
int hispmv_boundary_pack(hispmv_ctx* ctx, const float* const* d_last, const float* d_mask, float* d_send, int32_t n, void* stream);
int hispmv_boundary_apply(hispmv_ctx* ctx, float* const* d_first, const float* d_recv, const float* d_weights, int32_t n, int32_t world,
                          void* stream);

/* ---- Krylov solvers on loaded handles (no counterpart in the reference, which multiplies only) -----------------------------------
 * A x = b solved on the device: the products are exactly the launches of hispmv_spmv_device / hispmv_spmv_device_t (the first with
 * alpha = -1, beta = 1, bias = b for the residual r = b - A x, every later one with alpha = 1, beta = 0), and everything between two
 * products runs in fused vector kernels that keep every scalar on the device.  The host looks at the result every check_every
 * iterations, or never.  The workspace is the caller's (hispmv_krylov_info: work_bytes, 16-byte aligned); nothing is kept in the
 * handle or the context.  ONE solve per handle may be in flight: the handle's carries and partial vectors belong to its products.
 *
 * THE DOT PRODUCT (a, b) of two fp32 vectors of n elements.  The product of two floats is exact in fp64; the sums are fp64 in an order
 * that depends on n alone -- not on the device, the stream or the run.  With C = ceil(n / 1024) chunks of 1024 elements and
 * G = min(C, 1024) workgroups (hispmv_prep_krylov_groups):
 *   - thread t (0 .. 255) of chunk c owns elements 1024 c + 4 t + j, j = 0 .. 3; s(c, t) = ((((+0 + a0 b0) + a1 b1) + a2 b2) + a3 b3),
 *     elements at or beyond n left out (adding +0 in their place gives the same bits);
 *   - workgroup g takes chunks g, g + G, g + 2 G, ... ascending: acc(g, t) = ((+0 + s(g, t)) + s(g + G, t)) + ...;
 *   - TREE over the 256 values v[t]: v[t] += v[t + 128] for t < 128, then v[t] += v[t + 64] for t < 64, then 32, 16, 8, 4, 2, 1;
 *     partial(g) = v[0];
 *   - the result is the same scheme over the partials: u[t] = ((((+0 + partial(4 t)) + partial(4 t + 1)) + partial(4 t + 2)) +
 *     partial(4 t + 3)), partials at or beyond G left out, then TREE over u.
 * Every kernel that needs a dot product's value sums the partials itself, in every workgroup, so all readers hold the same bits and
 * no atomic, ticket or launch of its own is spent on a scalar.
 *
 * THE UPDATES.  A scalar (alpha, beta, omega) is computed in fp64 with IEEE division from such sums and rounded ONCE to fp32 (nearest
 * even) before it meets a vector.  Vector arithmetic is fp32 and unfused, one rounding per operation:
 *   CG         q = A p; alpha = rho / (p, q); x = x + alpha32 * p; r = r - alpha32 * q; z = minv * r (or r); rho' = (r, z);
 *              beta = rho' / rho; p = z + beta32 * p.  Start: r = b - A x, p = z.
 *   BiCGSTAB   v = A p; alpha = rho / (rhat, v); s = r - alpha32 * v; t = A s; omega = (t, s) / (t, t); x = x + alpha32 * p;
 *              x = x + omega32 * s; r = s - omega32 * t; rho' = (rhat, r); beta = (rho' / rho) * (alpha / omega);
 *              p = r + beta32 * (p - omega32 * v).  Start: rhat = p = r = b - A x.  (s, s) within the tolerance ends the solve on the
 *              half step x = x + alpha32 * p.
 *   CGLS       q = A p; alpha = gamma / (q, q); x = x + alpha32 * p; r = r - alpha32 * q; s = A^T r; gamma' = (s, s);
 *              beta = gamma' / gamma; p = s + beta32 * p.  Start: r = b - A x, p = s = A^T r.
 * STOPPING is decided on the device: the kernel that finishes an iteration compares rr <= (rtol * rtol) * bb in fp64, rr = (r, r) and
 * bb = (b, b) -- CGLS: rr = (s, s), bb = (A^T b, A^T b) -- and sets `done`; from the next launch on every update is a no-op (the
 * products still run, their results are ignored).  x, iterations and relres are therefore those of the FIRST iteration that met the
 * tolerance, whatever check_every is.  A denominator ((p, q), (rhat, v), (t, t), (q, q), rho, omega, CGLS: bb) that is zero or not
 * finite sets `breakdown` before the update that would use it, and the updates freeze the same way: x stays the last good iterate.
 * b == 0 gives x = 0, CONVERGED, 0 iterations -- and, where the host looks (check_every > 0), no product.
 *
 * check_every = k > 0: after every k iterations the scalar block is copied to pinned memory (hipMemcpyAsync), the stream is
 * synchronised, and the loop ends on done, breakdown or max_iters; the call returns with *result filled.  check_every = 0: exactly
 * max_iters iterations are enqueued and the call returns without synchronising, *result = {HISPMV_KRYLOV_IN_FLIGHT, 0, 0, products
 * enqueued}; hispmv_krylov_status reads the outcome later.  Between checks the loop adds no allocation, synchronous copy or
 * synchronisation to what the product launches do. */
#define HISPMV_KRYLOV_CG        0
#define HISPMV_KRYLOV_BICGSTAB  1
#define HISPMV_KRYLOV_CGLS      2
#define HISPMV_KRYLOV_CONVERGED 0
#define HISPMV_KRYLOV_MAX_ITERS 1
#define HISPMV_KRYLOV_BREAKDOWN 2
#define HISPMV_KRYLOV_IN_FLIGHT 3
typedef struct hispmv_krylov_result {
    int32_t status;         /* HISPMV_KRYLOV_CONVERGED, _MAX_ITERS, _BREAKDOWN (_IN_FLIGHT: a check_every = 0 call that has returned) */
    int32_t iterations;     /* updates of x applied */
    double relres;          /* sqrt(rr / bb), from the recursive residual */
    int64_t products;       /* products issued, forward and transposed */
} hispmv_krylov_result;
/* The rule on the host (no device needed): *groups = min(ceil(n / 1024), 1024), the workgroups of a pass over n elements and the fp64
 * partials of a dot product.  n < 0 -> HISPMV_EINVAL. */
int hispmv_prep_krylov_groups(int64_t n, int64_t* groups);
/* out = {accepted, work_bytes, launches_per_iteration (vector kernels), products_per_iteration, products_t_per_iteration, byte offset
 * of the residual r in the workspace, elements of x, elements of b} for `solver` (HISPMV_KRYLOV_CG, ...) on this handle; zeros for a
 * handle the solver does not accept (not loaded, not square for CG and BiCGSTAB, refused by hispmv_spmv_device_t for CGLS). */
int hispmv_krylov_info(const hispmv_ctx* ctx, int matrix_idx, int solver, int64_t out[8]);
/* *d_out (a double in device memory, 8-byte aligned) = (a, b) in the order above; asynchronous on `stream`.  d_a and d_b need 4-byte
 * alignment (16-byte aligned operands are read in 16-byte accesses, same bits); work_bytes >= 8 * groups, 16-byte aligned. */
int hispmv_dot_device(hispmv_ctx* ctx, int64_t n, const float* d_a, const float* d_b, double* d_out, void* d_work, int64_t work_bytes,
                      void* stream);
/* Preconditioned CG for a symmetric positive definite handle.  d_x[cols] holds the initial guess on entry and the solution on return;
 * d_minv is NULL or the inverse diagonal (z = minv * r elementwise).  Every handle hispmv_spmv_device accepts is accepted (a bf16
 * handle solves the system of its rounded values).  HISPMV_EINVAL before any launch: a handle that is not square, rtol < 0,
 * max_iters < 1 or > 2^30 (the launches of a check_every = 0 call are counted in 64 bits, but nobody waits for more), check_every < 0,
 * a workspace that is NULL, too small or not 16-byte aligned.  d_b, d_x, d_minv: 4-byte aligned; each vector that is 16-byte aligned
 * is read and written in 16-byte accesses, the others in 4-byte ones, same bits.
 * Cost outside the loop: a call with check_every > 0 allocates and frees its 128 pinned bytes itself (hipHostMalloc / hipHostFree, both
 * of which synchronise the device) and looks at (b, b) once before the first product; check_every = 0 does neither. */
int hispmv_cg_device(hispmv_ctx* ctx, int matrix_idx, const float* d_b, float* d_x, const float* d_minv, double rtol, int64_t max_iters,
                     int64_t check_every, void* d_work, int64_t work_bytes, void* stream, hispmv_krylov_result* result);
/* BiCGSTAB for square, non-symmetric systems; the forward product only, two per iteration.  Arguments and errors as for CG. */
int hispmv_bicgstab_device(hispmv_ctx* ctx, int matrix_idx, const float* d_b, float* d_x, double rtol, int64_t max_iters, int64_t check_every,
                           void* d_work, int64_t work_bytes, void* stream, hispmv_krylov_result* result);
/* CGLS: min || b - A x || for any rows x cols, b[rows], x[cols]; stops on || A^T r || <= rtol * || A^T b ||; one forward and one
 * transposed product per iteration (three products before the first).  Accepts what hispmv_spmv_device_t accepts and refuses the rest
 * as it does (HISPMV_ENOTSUP, its message) before any launch, d_x untouched.  Over a stored transpose the solve is bit-reproducible;
 * over the atomic transposed path it is not.  A^T b == 0 with b != 0 is a breakdown. */
int hispmv_cgls_device(hispmv_ctx* ctx, int matrix_idx, const float* d_b, float* d_x, double rtol, int64_t max_iters, int64_t check_every,
                       void* d_work, int64_t work_bytes, void* stream, hispmv_krylov_result* result);
/* Synchronises `stream` and reads the outcome of a check_every = 0 solve that ran on it out of its workspace. */
int hispmv_krylov_status(hispmv_ctx* ctx, const void* d_work, void* stream, hispmv_krylov_result* result);

/* ---- Krylov solvers for several right-hand sides ------------------------------------------------------------------------------------
 * num_vecs INDEPENDENT solves A x_v = b_v that share their launches: column v has its own scalars, iteration count, stopping and
 * breakdown.  This is not block CG: no Krylov space is shared.  Operands are feature-major like hispmv_spmm_device: d_B is [n, ld_b],
 * d_X is [n, ld_x], row-major, ld >= num_vecs >= 1, pointers 4-byte aligned.  d_X holds the initial guesses on entry and the solutions
 * on return; the floats num_vecs .. ld_x - 1 of a row of d_X are never written, the pads of d_B never read.  d_minv is NULL or ONE
 * inverse diagonal minv[n] for all columns; rtol, max_iters and check_every are shared too.
 *
 * THE ARITHMETIC OF COLUMN v IS THAT OF THE SINGLE-VECTOR ENTRIES ABOVE with the product of hispmv_spmm_device in place of
 * hispmv_spmv_device's: the dot products in the order of hispmv_dot_device for that n, fp64 scalars rounded once, fp32 unfused vector
 * arithmetic, the update formulas, the stopping rule rr <= rtol^2 * bb and the denominators that set `breakdown` of the CG and
 * BiCGSTAB paragraphs.  b_v == 0 gives x_v = 0, CONVERGED, 0 iterations.  x_v, iterations_v and relres_v therefore depend neither on
 * check_every nor on the other columns, their number, ld, or the column's position (hispmv_spmm_device's bits of a vector do not
 * either); an Inf or NaN in b_v or in x_v's initial guess breaks column v down and no other.  From the launch after a column is done
 * or broken down every update of it is a no-op; the products still compute it and are ignored; the other columns go on.
 * To keep the order of a dot product a function of n alone with lanes running across columns, n <= 1024 * 1024: every workgroup owns
 * exactly one chunk of 1024 rows and G = ceil(n / 1024).  A larger n -> HISPMV_EINVAL.
 *
 * PRODUCTS: hispmv_spmm_device, called like any caller does.  The residual is one call with alpha = -1, beta = 1 in place on R (B
 * copied into it), every later product has alpha = 1, beta = 0; results[v].products counts these calls and is the same for every
 * column.  WORKSPACE (hispmv_krylov_multi_info: work_bytes, 16-byte aligned), laid out by the rule of hispmv_prep_krylov_multi: the
 * columns' scalar blocks (128 bytes each, twice), the partials [slot][G][ldw], the solver's vectors [n, ldw] with ldw = num_vecs
 * rounded up to 4 -- 16-byte aligned, so the products may take VL 4 --, then the workspace hispmv_spmm_info sizes for (num_vecs, ldw).
 * Nothing is kept in the handle or the context.
 *
 * check_every = k > 0: every k iterations ONE asynchronous copy of the columns' scalar blocks (128 * num_vecs bytes) to a pinned
 * buffer of the call's own and one synchronise; the loop ends when EVERY column is done or broken down, or at max_iters.  Before the
 * first product one look at the (b_v, b_v) (8 * num_vecs bytes): all zero -> X = 0 and no product.  check_every = 0: everything is
 * enqueued, nothing synchronises, every results[v] is HISPMV_KRYLOV_IN_FLIGHT and hispmv_krylov_multi_status reads the outcome.
 *
 * ACCEPTED: what hispmv_spmm_device accepts, square: a loaded slice-stream handle, all group kinds and parts, fp32 or bf16 storage.  A
 * tile-stream or dense handle -> hispmv_spmm_device's code and message; not square -> HISPMV_EINVAL, the "square" message above;
 * num_vecs < 1, ld < num_vecs, rtol < 0, max_iters < 1, check_every < 0, a workspace that is NULL, short or not 16-byte aligned, a bad
 * index -> HISPMV_EINVAL; not loaded -> HISPMV_ESTATE.  All before any launch, d_X untouched.
 * Out of scope: CGLS and any transposed multi solve, true block-Krylov methods, per-column rtol or preconditioners, n > 2^20, bf16
 * vectors, tile-stream and dense handles, solves inside hispmv_spmv_device_batch or the step kernel, sharding over devices, HIP-graph
 * capture, dot products fused into the product's stores. */
/* The layout rule on the host (no device needed): out = {G = ceil(n / 1024), ldw = num_vecs rounded up to 4, bytes of the scalar
 * blocks and the (b, b) row = 2 * 128 * ldw + 8 * ldw, bytes of the partials = 8 slots * G * ldw * 8}; R lies behind the two.
 * n < 0, n > 2^20, num_vecs < 1 or > 2^20 -> HISPMV_EINVAL. */
int hispmv_prep_krylov_multi(int64_t n, int64_t num_vecs, int64_t out[4]);
/* out = {accepted, work_bytes, vector kernels per iteration, hispmv_spmm_device calls per iteration, leading dimension of the
 * workspace's vectors, byte offset of R in the workspace, n, G} for `solver` (HISPMV_KRYLOV_CG or _BICGSTAB) and num_vecs columns;
 * zeros for a handle the entries do not accept. */
int hispmv_krylov_multi_info(const hispmv_ctx* ctx, int matrix_idx, int solver, int64_t num_vecs, int64_t out[8]);
/* d_out[v] = (a[:, v], b[:, v]), v < num_vecs, each in the order of hispmv_dot_device for n; d_a is [n, ld_a], d_b is [n, ld_b], 4-byte
 * aligned, pads never read; d_out 8-byte aligned; work_bytes >= 8 * G * ldw, 16-byte aligned.  n <= 2^20.  Asynchronous on `stream`. */
int hispmv_dot_multi_device(hispmv_ctx* ctx, int64_t n, int64_t num_vecs, const float* d_a, int64_t ld_a, const float* d_b, int64_t ld_b,
                            double* d_out, void* d_work, int64_t work_bytes, void* stream);
/* results: num_vecs of them. */
int hispmv_cg_multi_device(hispmv_ctx* ctx, int matrix_idx, const float* d_B, int64_t ld_b, float* d_X, int64_t ld_x, int64_t num_vecs,
                           const float* d_minv, double rtol, int64_t max_iters, int64_t check_every, void* d_work, int64_t work_bytes,
                           void* stream, hispmv_krylov_result* results);
int hispmv_bicgstab_multi_device(hispmv_ctx* ctx, int matrix_idx, const float* d_B, int64_t ld_b, float* d_X, int64_t ld_x, int64_t num_vecs,
                                 double rtol, int64_t max_iters, int64_t check_every, void* d_work, int64_t work_bytes, void* stream,
                                 hispmv_krylov_result* results);
/* Synchronises `stream` and reads the outcome of a check_every = 0 multi solve of num_vecs columns out of its workspace. */
int hispmv_krylov_multi_status(hispmv_ctx* ctx, const void* d_work, int64_t num_vecs, void* stream, hispmv_krylov_result* results);

/* ---- Restarted GMRES(m) on loaded handles ---------------------------------------------------------------------------------------------
 * A x = b for a square, non-symmetric handle with ONE product per inner iteration and a residual that never grows inside a cycle.
 * The products are hispmv_spmv_device's launches, written straight into the basis; everything between two products is a pass over
 * the basis in four vector kernels.  Arguments, errors, the stream rule and "ONE solve per handle in flight" are hispmv_cg_device's,
 * plus restart = m, 1 .. HISPMV_GMRES_MAX_RESTART.  d_minv is NULL or an inverse diagonal used as a RIGHT preconditioner:
 * A diag(minv) u = b, x = diag(minv) u; the residual the stopping rule sees stays that of A x = b.
 *
 * THE ARITHMETIC.  Every dot product is hispmv_dot_device's for n.  Scalars are fp64 with IEEE / and sqrt, unfused; a scalar is
 * rounded ONCE to fp32 before it meets a vector; vector arithmetic is fp32, one rounding per operation.  bb = (b, b), tol2 = rtol^2.
 * START OF A CYCLE of m = min(restart, iterations left) columns: r = b - A x (the product with alpha -1, beta 1, bias b, into basis
 *   slot 0); rr = (r, r); rr not finite: breakdown; else rr <= tol2 * bb: done (b == 0 gives x = 0, CONVERGED, 0 iterations, as in CG);
 *   else beta = sqrt(rr), v_0 = f32(1 / beta) * r in place, g_res[0] = beta, cols = 0.
 * INNER STEP j: z = minv * v_j (or v_j); w = A z, written into basis slot j + 1.  CGS2: h1_i = (v_i, w) for i <= j; then
 *   w = w - f32(h1_i) * v_i for i ascending (t = h32 * v is rounded before w = w - t); h2_i = (v_i, w); the same subtraction with h2;
 *   h_i = h1_i + h2_i; ww = (w, w); hn = sqrt(ww).  A h1_i, h2_i or ww that is not finite sets breakdown in the kernel that sums it,
 *   before that kernel writes a vector.  The earlier rotations, i < j ascending: t = c_i h_i + s_i h_{i+1};
 *   h_{i+1} = c_i h_{i+1} - s_i h_i; h_i = t.  The new one: d = sqrt(h_j h_j + hn hn); d zero or not finite: breakdown; else
 *   c_j = h_j / d, s_j = hn / d, R[i][j] = h_i (i < j), R[j][j] = d, g_fin[j] = c_j g_res[j], g_res[j+1] = -(s_j g_res[j]).  Then
 *   cols = j + 1, iterations += 1, rr = g_res[j+1]^2; rr <= tol2 * bb: done (a lucky breakdown hn == 0 lands here); else
 *   v_{j+1} = f32(1 / hn) * w in place.
 * CLOSE OF A CYCLE, acting once and only if cols > 0: back substitution in fp64, i descending: s = g_fin[i]; for k = i + 1 .. cols - 1
 *   ascending s = s - R[i][k] y_k; y_i = s / R[i][i].  u = f32(y_0) * v_0, then u = u + f32(y_i) * v_i for i ascending;
 *   x = x + minv * u (or x + u); cols = 0.
 * FREEZE: after done or breakdown every kernel copies the scalar block and writes no vector (the products still run and are ignored);
 * the close still applies the cols columns completed before, so iterations counts exactly the columns that entered x.
 * relres = sqrt(rr / bb), from the recomputed residual at a restart and from |g_res| inside a cycle.  products of a check_every = 0
 * call = cycles + max_iters.  The host looks every check_every inner iterations, counted across cycles, and once at the end; the close
 * of the cycle a look finds ended is enqueued and waited for before the call returns, so x, iterations and relres do not depend on
 * check_every.  Between looks the loop adds no allocation, synchronous copy or synchronisation.
 *
 * WORKSPACE (hispmv_gmres_info: work_bytes, 16-byte aligned; the rule is hispmv_prep_gmres's): the two 128-byte scalar blocks of the
 * other solvers first -- rr, bb, b2, iterations, done, breakdown and products keep their slots, slot 13 holds j and slot 14 cols,
 * and the last kernel of a check_every = 0 call writes block 0, so hispmv_krylov_status reads a GMRES workspace unchanged -- then
 * c, s, g_fin, g_res, h1, h (66 doubles each), R (64 x 64 doubles, row-major), the partials, the restart + 1 basis vectors
 * (ceil(n / 4) * 4 floats apart) and, with minv, one vector z.  No kernel reads a word one of its own workgroups writes: g_fin and
 * g_res are two arrays for that reason, and only workgroup 0 writes the Givens data and the block.
 * Out of scope: several right-hand sides, flexible or left preconditioning, restart above 64, dot products fused into the product's
 * stores, HIP-graph capture, sharding over devices, fp64 vectors. */
#define HISPMV_GMRES_MAX_RESTART 64
/* The workspace rule on the host (no device needed): out = {work_bytes, byte offset of the basis V, floats between two basis vectors,
 * groups (hispmv_prep_krylov_groups(n)), dot_tile (basis vectors one pass of the multi-dot kernel accumulates per thread), vector
 * kernels per inner iteration, vector kernels per cycle besides, basis vectors held (restart + 1)}.  n < 0 or restart outside
 * 1 .. 64 -> HISPMV_EINVAL. */
int hispmv_prep_gmres(int64_t n, int64_t restart, int with_minv, int64_t out[8]);
/* out = {accepted, work_bytes, launches per inner iteration, launches per cycle besides, products per inner iteration (1), byte offset
 * of V, vector stride in floats, n}; zeros for a handle that is not loaded or not square. */
int hispmv_gmres_info(const hispmv_ctx* ctx, int matrix_idx, int64_t restart, int with_minv, int64_t out[8]);
/* d_out[i] = (V_i, w), i < k <= 65, V_i = d_V + i * ld_v: each value bit for bit hispmv_dot_device(n, V_i, w), all from one pass that
 * loads w once per dot_tile basis vectors.  Operands 4-byte aligned (16-byte accesses per vector where that vector is 16-byte
 * aligned), d_out 8-byte aligned, work_bytes >= 8 * k * groups, 16-byte aligned.  Asynchronous on `stream`. */
int hispmv_dot_basis_device(hispmv_ctx* ctx, int64_t n, int64_t k, const float* d_V, int64_t ld_v, const float* d_w, double* d_out,
                            void* d_work, int64_t work_bytes, void* stream);
int hispmv_gmres_device(hispmv_ctx* ctx, int matrix_idx, const float* d_b, float* d_x, const float* d_minv, int64_t restart, double rtol,
                        int64_t max_iters, int64_t check_every, void* d_work, int64_t work_bytes, void* stream,
                        hispmv_krylov_result* result);

/* ---- Block-Jacobi preconditioner for CG and GMRES -------------------------------------------------------------------------------------
 * M = the block diagonal of a square handle in blocks of bs = 4, 8, 16 or 32: block k covers rows and columns k bs ..
 * min(n, (k + 1) bs) - 1, n_blocks = ceil(n / bs).  The preconditioner is z = M^-1 r with the blocks inverted once.  It lives in a
 * buffer of the CALLER's; nothing is kept in the handle or the context, and a companion (stored transpose) plays no part.
 *
 * THE BUFFER (hispmv_prep_block_jacobi: pre_bytes, 16-byte aligned): first n_blocks * bs * bs floats, block k row-major, the INVERSE
 * of diagonal block k (a multiple of 16 bytes); then n_blocks int32 flags, 0 = inverted, 1 = replaced by the identity; the whole
 * rounded up to 16 bytes.  The last block of an n that is no multiple of bs is padded before the inversion: 1 on the diagonal of
 * its absent rows, 0 elsewhere in their rows and columns -- so its inverse is the inverse of the present part, padded the same way.
 *
 * EXTRACTION writes the padded diagonal blocks, not yet inverted.  Slice-stream handles (every group kind, column and band tiles,
 * both parts of a stray split, fp32 and bf16 storage -- the rounded values, the system the solvers solve): a fill kernel, then one
 * walk per part over the slice stream, which adds every stored value v at (row, col) with row / bs == col / bs and both below n
 * into word (row / bs, row % bs, col % bs) with a hardware float atomic.  An entry stored once is one add onto +0: the same bits
 * every run.  Two duplicates of one position give the same bits in either order.  THREE OR MORE duplicates of one position are summed
 * in no fixed order.  A stored +-0 changes no value.  As for d_y of hispmv_spmv_device_t, the buffer must be ordinary device memory
 * (hipMalloc, a torch tensor: coarse-grained); on fine-grained or host-pinned memory the adds are not guaranteed to land.  Dense
 * handles (fp32 and bf16 W): one plain kernel reads the blocks of W, no atomics.  Tile-stream handles -> HISPMV_ENOTSUP with the
 * message of the transposed entries' refusal; not square, a bad bs, a buffer that is NULL, short or not 16-byte aligned ->
 * HISPMV_EINVAL; before hispmv_load_matrices -> HISPMV_ESTATE.  All before any launch.
 *
 * INVERSION, per block, in place: Gauss-Jordan with partial pivoting in fp32, unfused, one rounding per operation.  `used` = no row.
 *   for k = 0 .. bs - 1:
 *     p = the row not in `used` whose |a[p][k]| is largest, the magnitudes compared as their bit patterns without the sign (so a
 *         NaN counts above Inf); the lowest such row on ties.  pv = a[p][k]; pv zero or not finite: the block is BAD.
 *     inv = 1 / pv (one IEEE division).  The new pivot row: w[j] = a[p][j] * inv for j != k, w[k] = inv.
 *     every other row i (used or not): f = a[i][k]; a[i][k] = +0; then for every j: t = f * w[j]; a[i][j] = a[i][j] - t.
 *     a[p][:] = w; p joins `used`; sigma(k) = p.
 *   The inverse: out[k][sigma(j)] = a[sigma(k)][j].  Any word of it not finite: the block is BAD.
 * A BAD block is replaced by the identity and flagged 1, so a solve is never poisoned by a block that cannot be inverted.
 *
 * THE MULTIPLY z = M^-1 r: z_i = ((+0 + B[i][0] r_0) + B[i][1] r_1) + ... in fp32, every product rounded and then added, k ascending
 * over the bs columns of row i's block B; r at or beyond n counts as +0, z at or beyond n is not stored.  It runs on the Krylov
 * layer's chunk walk (1024 elements per workgroup step, a thread owns 4 consecutive rows) without LDS or barrier; d_r and d_z need
 * 4-byte alignment only and may be the same vector.
 *
 * THE SOLVERS hispmv_cg_bj_device and hispmv_gmres_bj_device are hispmv_cg_device and hispmv_gmres_device with (d_pre, block_size)
 * in place of d_minv: wherever those form minv * v elementwise, these form the multiply above on the same values (CG: z = M^-1 r, so
 * M should be symmetric positive definite like A; GMRES: right preconditioning, A M^-1 u = b, x = M^-1 u).  Everything else is
 * theirs: the workspace of the minv variants (hispmv_krylov_info; hispmv_gmres_info with with_minv = 1), the scalar rules, freeze,
 * breakdown, check_every, hispmv_krylov_status, the stream rule, the launch counts.  d_pre must stay unchanged while a solve is in
 * flight.  block_size outside {4, 8, 16, 32}, d_pre NULL or not 16-byte aligned -> HISPMV_EINVAL before any launch.
 * Out of scope: preconditioned BiCGSTAB or CGLS, blocks for the multi-right-hand-side solvers, block sizes above 32, variable blocks,
 * symmetrising the computed inverse, ILU / IC, tile-stream handles, a fixed summation order for three or more duplicates. */
/* The layout rule on the host (no device needed): out = {n_blocks, pre_bytes, byte offset of the flags, floats of a block}.  n < 0,
 * n >= 2^31 or bs outside {4, 8, 16, 32} -> HISPMV_EINVAL. */
int hispmv_prep_block_jacobi(int64_t n, int64_t block_size, int64_t out[4]);
/* out = {accepted, n_blocks, pre_bytes, launches of a setup (extraction and inversion), work_bytes of hispmv_cg_bj_device, work_bytes
 * of hispmv_gmres_bj_device with restart 1, bytes each further step of restart adds, n}; zeros for a handle the extraction does not
 * accept (not loaded, not square, a tile stream).  A bad index or block_size -> HISPMV_EINVAL. */
int hispmv_block_jacobi_info(const hispmv_ctx* ctx, int matrix_idx, int64_t block_size, int64_t out[8]);
/* The padded diagonal blocks of the loaded matrix, not inverted, into the block area of d_pre; the flags are not written.
 * Asynchronous on `stream`. */
int hispmv_block_jacobi_extract_device(hispmv_ctx* ctx, int matrix_idx, int64_t block_size, void* d_pre, int64_t pre_bytes, void* stream);
/* Inverts the n_blocks blocks at d_pre in place and writes their flags behind them (the layout of n = n_blocks * block_size).
 * Asynchronous on `stream`; needs no handle.  The result is bit for bit the rule above. */
int hispmv_block_invert_device(hispmv_ctx* ctx, void* d_pre, int64_t n_blocks, int64_t block_size, void* stream);
/* Extraction followed by inversion: d_pre is ready for the multiply and the solvers behind it on `stream`. */
int hispmv_block_jacobi_setup_device(hispmv_ctx* ctx, int matrix_idx, int64_t block_size, void* d_pre, int64_t pre_bytes, void* stream);
/* Synchronises `stream` and returns in *flagged the number of blocks replaced by the identity. */
int hispmv_block_jacobi_status(hispmv_ctx* ctx, const void* d_pre, int64_t n, int64_t block_size, void* stream, int64_t* flagged);
/* d_z = M^-1 d_r over n elements; asynchronous on `stream`. */
int hispmv_block_jacobi_apply_device(hispmv_ctx* ctx, const void* d_pre, int64_t n, int64_t block_size, const float* d_r, float* d_z,
                                     void* stream);
int hispmv_cg_bj_device(hispmv_ctx* ctx, int matrix_idx, const float* d_b, float* d_x, const void* d_pre, int64_t block_size, double rtol,
                        int64_t max_iters, int64_t check_every, void* d_work, int64_t work_bytes, void* stream,
                        hispmv_krylov_result* result);
int hispmv_gmres_bj_device(hispmv_ctx* ctx, int matrix_idx, const float* d_b, float* d_x, const void* d_pre, int64_t block_size,
                           int64_t restart, double rtol, int64_t max_iters, int64_t check_every, void* d_work, int64_t work_bytes,
                           void* stream, hispmv_krylov_result* result);

/* ---- Lanczos / eigsh: a few eigenvalues of a symmetric handle ---------------------------------------------------------------------
 * Thick-restart Lanczos with full reorthogonalisation for the k algebraically largest (LA), algebraically smallest (SA) or largest in
 * magnitude (LM) eigenvalues of a square handle, and their eigenvectors.  The library cannot check symmetry, as with hispmv_cg_device:
 * the caller owes it.  A step is a GMRES inner iteration without the Givens rotation -- the product of hispmv_spmv_device written
 * straight into the basis, the multi-dot kernel, the subtract-and-dot kernel twice (hispmv_gmres_device's, unchanged) -- and one kernel
 * that normalises and records.  The restart is one tall-skinny in-place rotation of the basis.  The host looks ONCE PER CYCLE, behind
 * the last step it has enqueued: there is no check_every.  The grid, the chunk order and every dot product are hispmv_dot_device's
 * for n; vectors are fp32, unfused, one rounding per operation; sums and scalars are fp64 with IEEE / and sqrt; a scalar is rounded
 * ONCE to fp32 before it meets a vector.  ONE run per handle in flight; the whole state lies in the caller's workspace.
 *
 * OPEN: slot 0 of the basis = v0; vv = (v0, v0).  vv zero or not finite: BREAKDOWN (slot 0 keeps the copy).  Otherwise
 *   V_0 = f32(1 / sqrt(vv)) * v0.  The scalar block is built from nothing.
 * STEP j (V_0 .. V_j orthonormal): w = A V_j into slot j + 1 (alpha 1, beta 0, no bias).  CGS2 exactly as GMRES's inner step:
 *   h1_i = (V_i, w), i <= j; w = w - f32(h1_i) * V_i for i ascending; h2_i = (V_i, w); the same subtraction with h2; h_i = h1_i + h2_i;
 *   a h1_i or h2_i that is not finite sets breakdown in the kernel that sums it.  Then the normalise-and-record kernel: ww = (w, w);
 *   not finite: BREAKDOWN.  Otherwise products += 1, steps = j + 1, Hc[j][i] = h_i for i <= j, beta_j = sqrt(ww), and
 *   THE INVARIANT SUBSPACE RULE: t = +0, t = t + h_i * h_i for i ascending; if ww <= tiny^2 * (ww + t), tiny = 2^-12
 *   (HISPMV_LANCZOS_TINY_LOG2), w is rounding noise: it is not normalised, the word `invariant` is set and the state freezes (the word
 *   `done` of the other solvers: every later kernel of the cycle copies the block and writes no vector; the products still run and are
 *   ignored).  An all-zero matrix gives 0 <= 0: invariant with eigenvalue 0, not a breakdown.  Otherwise V_{j+1} = f32(1 / beta_j) * w.
 *   `products` counts the steps that reached this kernel unfrozen, so a run that freezes reports the products it used.
 * HOST LOOK, once per cycle: the scalar block, Hc and the betas come to pinned memory, the stream is synchronised.  m = steps.  The
 *   projected matrix H (m x m) holds the kept Ritz values on its leading diagonal after a restart (zero elsewhere); every column j the
 *   device computed in this cycle is mirrored into its row, H[i][j] = H[j][i] = Hc[j][i], i <= j.  With full CGS2 the arrowhead column
 *   at index keep comes out of the dots by itself.
 * RITZ STEP (hispmv_prep_ritz, fp64): cyclic Jacobi on H; theta its eigenvalues, Y orthonormal.  Order by `which`: LA descending, SA
 *   ascending, LM descending in |theta|, ties in Jacobi's order.  res_i = beta_{m-1} * |Y[m-1][i]|; scale = max |theta_i| over all m;
 *   pair i is converged when res_i <= tol * scale.
 * STOP: CONVERGED when the first min(k, m) pairs in order are converged and m >= k; else INVARIANT (HISPMV_KRYLOV_INVARIANT) when the
 *   subspace is invariant -- found = min(k, m) pairs are returned with their honest residuals; else MAX_ITERS when products >=
 *   max_products at the look (found = min(k, m) pairs are returned as they stand).  BREAKDOWN returns found = 0 and leaves d_vecs
 *   untouched.
 * RESTART otherwise: keep = min(k + (ncv - k) / 2, ncv - 1); V[:, c] = sum_i f32(Y[i][order c]) * V[:, i] for c < keep -- fp32, the
 *   product rounded, then added, i ascending from 0.0f --; slot keep takes slot m, the normalised residual vector; H = diag(theta in
 *   order, keep of them); the next cycle runs steps keep .. ncv - 1.
 * FINISH: the same rotation with the `found` wanted columns, out of place, into d_vecs (vector c at d_vecs + c * ld_vecs).  The vectors
 *   are not renormalised: their norm is 1 to a few fp32 ulps times sqrt(m).  vals_out[i] = theta_i and res_out[i] = res_i for
 *   i < found; the entries behind are not written.
 *
 * WORKSPACE (hispmv_lanczos_info: work_bytes, 16-byte aligned; the rule is hispmv_prep_lanczos's): three 128-byte scalar blocks in the
 * 512 bytes the other solvers open with -- breakdown, done and products keep their slots, slot 13 holds steps and slot 14
 * `invariant`; the kernels of a step that write the block pass it on by the one rule of the thick-restart solvers (every kernel but the
 * step's last writes block 1 or 2, whichever it does not read, the last writes block 0), which for Lanczos's three kernels gives
 * 0 -> 1 -> 2 -> 0, so a kernel never writes the block it
 * reads and every step, hence every call, leaves the state in block 0 --, then h1 and h (66 doubles each), Hc (64 columns of 66 doubles, column j at
 * hc_offset + 528 j), the 66 betas right behind Hc, Yt (64 x 65 floats: the coefficients of the last rotation, row c = output c), the
 * partials, and the ncv + 1 basis vectors (ceil(n / 4) * 4 floats apart).  Only workgroup 0 writes Hc, the betas and the block.
 * ACCEPTED: every square handle hispmv_spmv_device accepts -- slice streams, tile streams, dense, fp32 or bf16 storage (a bf16 handle
 * has the eigenvalues of its rounded values).  HISPMV_EINVAL before any launch, outputs untouched: a handle that is not square, k < 1,
 * ncv outside k + 1 .. HISPMV_LANCZOS_MAX_NCV, tol < 0, max_products < 1 or > 2^30, an unknown `which`, a NULL pointer or one not 4-byte
 * aligned, a workspace that is NULL, short or not 16-byte aligned; a call before load_matrices -> HISPMV_ESTATE.
 * Out of scope: multiple or tightly clustered eigenvalues beyond one copy (single-vector Lanczos finds ONE eigenvector of a multiple
 * eigenvalue), a random restart after an invariant subspace, shift-invert, generalised problems, singular values (those are hispmv_svds_device's, below), non-symmetric
 * Arnoldi, ncv > 64, locking and deflation, fp64 vectors, several start vectors, sharding over devices, HIP-graph capture. */
#define HISPMV_LANCZOS_MAX_NCV 64
#define HISPMV_LANCZOS_TINY_LOG2 (-12)
#define HISPMV_KRYLOV_INVARIANT 4
#define HISPMV_EIGSH_LA 0
#define HISPMV_EIGSH_SA 1
#define HISPMV_EIGSH_LM 2
typedef struct hispmv_eigsh_result {
    int32_t status;         /* HISPMV_KRYLOV_CONVERGED, _MAX_ITERS, _BREAKDOWN, _INVARIANT */
    int32_t found;          /* pairs returned */
    int64_t products;
    int64_t cycles;         /* host looks */
    double scale;           /* max |theta| of the last look: what tol is relative to */
} hispmv_eigsh_result;
/* The workspace rule on the host (no device needed): out = {work_bytes, byte offset of the basis V, floats between two basis vectors,
 * groups, byte offset of Hc, byte offset of Yt, launches per step (5, the product included), basis vectors held (ncv + 1)}.  n < 0 or
 * ncv outside 2 .. 64 -> HISPMV_EINVAL. */
int hispmv_prep_lanczos(int64_t n, int64_t ncv, int64_t out[8]);
/* The Ritz step on the host and nothing else (no device needed): H is symmetric m x m, row-major with ld doubles between rows (the
 * upper triangle is read), 1 <= m <= 64.  theta_out[m] and res_out[m] in the order of `which`; Yt_out[m * m], row c the eigenvector of
 * theta_out[c]; counts_out = {converged among the first min(k, m), Jacobi sweeps}.  Bad arguments -> HISPMV_EINVAL. */
int hispmv_prep_ritz(const double* H, int64_t ld, int64_t m, int64_t k, int which, double beta, double tol, double* theta_out, double* Yt_out,
                     double* res_out, int64_t counts_out[2]);
/* out = {accepted, work_bytes, byte offset of V, vector stride in floats, byte offset of Hc, byte offset of Yt, launches per step, n};
 * zeros for a handle that is not loaded or not square.  A bad index, ncv outside 2 .. 64 -> HISPMV_EINVAL. */
int hispmv_lanczos_info(const hispmv_ctx* ctx, int matrix_idx, int64_t ncv, int64_t out[8]);
/* d_out[c * ld_out + e] = sum_{i < m} d_Yt[c * m + i] * d_V[i * ld_v + e], c < k <= 64, e < n, 1 <= m <= 65: fp32, the product rounded
 * and then added, i ascending, starting from 0.0f.  d_out may be d_V itself (ld_out == ld_v): vector c then lands over slot c, and the
 * slots at or above k are untouched.  Any other overlap is undefined.  Pointers 4-byte aligned, pads never read or written.
 * Asynchronous on `stream`. */
int hispmv_basis_rotate_device(hispmv_ctx* ctx, int64_t n, int64_t m, int64_t k, const float* d_V, int64_t ld_v, const float* d_Yt,
                               float* d_out, int64_t ld_out, void* stream);
/* Enqueues the open (first != 0: j0 must be 0, d_v0 the start vector) and the steps j0 .. j1 - 1, 0 <= j0 < j1 <= 64, with no host
 * look.  The workspace is that of hispmv_prep_lanczos(n, max(j1, 2)): j1 + 1 basis vectors, and never less than the smallest layout
 * the rule knows.  Asynchronous on `stream`. */
int hispmv_lanczos_steps_device(hispmv_ctx* ctx, int matrix_idx, int64_t j0, int64_t j1, int first, const float* d_v0, void* d_work,
                                int64_t work_bytes, void* stream);
/* Synchronises `stream` and reads out = {steps, invariant, breakdown, products} out of the workspace of a run on it. */
int hispmv_lanczos_status(hispmv_ctx* ctx, const void* d_work, void* stream, int64_t out[4]);
/* The driver above.  d_v0[n] is the start vector (not written); d_vecs takes `found` vectors, ld_vecs >= n floats apart; vals_out and
 * res_out are host doubles [k].  The call returns with *result filled and the stream synchronised.  It allocates and frees its
 * pinned buffer itself, like a hispmv_cg_device call with check_every > 0. */
int hispmv_eigsh_device(hispmv_ctx* ctx, int matrix_idx, int64_t k, int64_t ncv, int which, double tol, int64_t max_products,
                        const float* d_v0, float* d_vecs, int64_t ld_vecs, double* vals_out, double* res_out, void* d_work,
                        int64_t work_bytes, void* stream, hispmv_eigsh_result* result);

/* ---- Golub-Kahan / svds: a few singular values of a handle of any shape ----------------------------------------------------------------
 * Thick-restart Golub-Kahan bidiagonalisation with full reorthogonalisation on both sides for the k LARGEST singular values of a
 * rows x cols handle, with their left and right singular vectors.  A step is two Lanczos steps on two bases of different lengths: V
 * holds ncv + 1 vectors of cols floats, U holds ncv vectors of rows floats, each with its own stride ceil(n / 4) * 4 and its own dot
 * grid, hispmv_dot_device's for that length.  The forward product is hispmv_spmv_device's, the transposed one hispmv_spmv_device_t's,
 * each written straight into the other basis; the multi-dot kernel and the subtract-and-dot kernel are hispmv_gmres_device's, unchanged,
 * the open is Lanczos's, the restart and the finish are hispmv_basis_rotate_device's kernel; one new kernel normalises and records, for
 * either side.  The host looks ONCE PER CYCLE.  All arithmetic follows the rules of "Lanczos / eigsh": vectors fp32, unfused, one
 * rounding per operation; sums and scalars fp64 with IEEE / and sqrt; a scalar is rounded ONCE to fp32 before it meets a vector.  ONE run
 * per handle in flight; the whole state lies in the caller's workspace.
 *
 * OPEN: Lanczos's, on V slot 0 with v0 (cols floats): vv = (v0, v0) zero or not finite: BREAKDOWN; else V_0 = f32(1 / sqrt(vv)) * v0.
 * STEP j, U side (V_0 .. V_j and U_0 .. U_{j-1} orthonormal): u = A V_j into U slot j (alpha 1, beta 0, no bias).  CGS2 against
 *   U_0 .. U_{j-1} exactly as Lanczos's against its basis: g1_i = (U_i, u); u = u - f32(g1_i) * U_i, i ascending; g2_i = (U_i, u); the same
 *   subtraction; g_i = g1_i + g2_i; a sum that is not finite sets breakdown in the kernel that sums it.  At j = 0 there is nothing to
 *   subtract: (u, u) comes from the dot kernel's partials alone.  Then the record kernel: uu = (u, u); not finite: BREAKDOWN.  Otherwise
 *   Gc[j][i] = g_i for i < j, and THE CLOSED-SPACE RULE: t = +0, t = t + g_i * g_i for i ascending; if uu <= tiny^2 * (uu + t), tiny =
 *   2^-12 as in Lanczos, A V_j lies in span U: steps = j, products += 1 (the product that found this out is work the answer uses: its
 *   coefficients are the last column of B'), the words `invariant`, `closed_u` and `done` are set, U slot j is not normalised, alpha_j is
 *   not written, and the state freezes.  Otherwise alpha_j = sqrt(uu) and U_j = f32(1 / alpha_j) * u.  (0 <= 0 holds: A v0 = 0 closes
 *   at step 0 with steps = 0.)
 * STEP j, V side: w = A^T U_j into V slot j + 1.  CGS2 against V_0 .. V_j, coefficients h_i, i <= j.  The record kernel: ww = (w, w);
 *   not finite: BREAKDOWN.  Otherwise beta_j = sqrt(ww), steps = j + 1, products += 2 (this step's two products: `products` counts
 *   unfrozen work only), and Lanczos's invariant rule on ww and the h_i: if it holds, `invariant` and `done` are set and w is not
 *   normalised; otherwise V_{j+1} = f32(1 / beta_j) * w.  The V-side coefficients serve the orthogonalisation and the rule only.
 *   The products of a frozen run still land in their slots (U slot j', V slot j' + 1 of the later steps) and are ignored.
 * HOST LOOK, once per cycle: the scalar block, Gc, the alphas and the betas come to pinned memory, the stream is synchronised.  m =
 *   steps.  The projected matrix B (m x m, upper) holds the kept singular values on its leading diagonal after a restart; every column
 *   j the device computed in this cycle is B[i][j] = Gc[j][i] for i < j and B[j][j] = alpha_j.  The arrow column at index keep comes out
 *   of the U-side dots by itself: (U_i, A V_keep) = beta * P[m-1][i].  hispmv_prep_bsvd gives B = P diag(s) Q^T, s descending;
 *   res_i = beta_{m-1} * |P[m-1][i]|; scale = s_0; pair i is converged when res_i <= tol * scale.
 *   After closed_u: A V_{m+1} = U_m B' and A^T U_m = V_{m+1} B'^T hold exactly with B' = [B | g] (m x (m + 1), g_i = Gc[m][i]); the SVD
 *   of B' gives singular values of A with residual estimates 0, the right vectors over m + 1 basis vectors.  m = 0 returns found = 0
 *   with status INVARIANT: the all-zero matrix and A v0 = 0 both end this way.
 * STOP (eigsh's rule): CONVERGED when the first min(k, m) pairs are converged and m >= k; else INVARIANT when the state froze by either
 *   rule, found = min(k, m) pairs with their honest residuals; else MAX_ITERS when products >= max_products at the look.  BREAKDOWN
 *   returns found = 0 and leaves the outputs untouched.
 * RESTART otherwise: keep = min(k + (ncv - k) / 2, ncv - 1); U[:, c] = sum_i f32(P[i][c]) * U_i and V[:, c] = sum_i f32(Q[i][c]) * V_i for
 *   c < keep, i < m: two in-place rotations with the arithmetic of hispmv_basis_rotate_device; V slot keep takes V slot m; B =
 *   diag(s_0 .. s_{keep-1}); the next cycle runs steps keep .. ncv - 1.
 * FINISH: the same rotations with the `found` wanted columns, out of place, into d_u (vector c at d_u + c * ld_u, rows floats) and d_v
 *   (d_v + c * ld_v, cols floats), not renormalised.  s_out[i] and res_out[i] for i < found; the entries behind are not written.
 *
 * THE SMALL SVD (hispmv_prep_bsvd, fp64): one-sided (Hestenes) Jacobi on G = B^T: rotations from the right over the column pairs
 *   (p, q), p < q, row-cyclic, make the columns orthogonal; a pair rotates when |g_p . g_q| > 8 eps |g_p| |g_q|; at most 64 sweeps.
 *   s = the column norms, Q = the normalised columns, P = the accumulated rotations; descending, ties in Jacobi's order.  A zero column
 *   has its place in Q filled by the first unit vector that two Gram-Schmidt passes against the columns before it leave longer than 1/2.
 *
 * WORKSPACE (hispmv_gk_info: work_bytes, 16-byte aligned; the rule is hispmv_prep_gk's): three 128-byte scalar blocks in the 512 bytes
 * the other solvers open with -- breakdown, done and products keep their slots, slot 13 holds steps, slot 14 `invariant`, slot 15
 * `closed_u` --, then g1 and g (66 doubles each, the two sides in turn), Gc (64 columns of 66 doubles, column j at gc_offset + 528 j),
 * the 66 alphas and then the 66 betas right behind Gc, Yt (64 x 65 floats, the two rotations of a look in turn), the partials (sized by
 * the larger of krylov_groups(rows) and krylov_groups(cols)), V, then U.  THE BLOCKS: a kernel reads the block the kernel before it
 * wrote; every kernel of a step but the last writes block 1 or 2, whichever it does not read; the last, the V side's record kernel,
 * writes block 0.  So no kernel writes the block it reads, and every step, hence every call, leaves the state in block 0.  A step is
 * 10 launches beside what the two products launch themselves.  Only workgroup 0 writes Gc, the alphas, the betas and the block.
 * ACCEPTED: every handle both hispmv_spmv_device and hispmv_spmv_device_t accept -- slice streams, dense, fp32 or bf16 storage (a bf16
 * handle has the singular values of its rounded values), tile streams under _KEEP_FORMAT, _COMPANION handles.  A handle
 * hispmv_spmv_device_t refuses is refused with that entry's message and status before any launch.  HISPMV_EINVAL before any launch,
 * outputs untouched: k < 1, k > min(rows, cols), ncv outside k + 1 .. HISPMV_GK_MAX_NCV, tol < 0, max_products outside 2 .. 2^30, a NULL
 * pointer or one not 4-byte aligned, a workspace that is NULL, short or not 16-byte aligned; a call before load_matrices ->
 * HISPMV_ESTATE.
 * DETERMINISM: on a _COMPANION handle both products have a fixed order, so the whole run is bit for bit tests/gk_model.py's.  On every
 * other handle the transposed product meets its sums in y through atomics -- the dense transposed kernel too, whenever it splits the
 * rows over several workgroups --: the run is correct, its bits are not promised.
 * Out of scope: the smallest singular values (which = "SM", harmonic Ritz), multiple singular values beyond one copy, shift-invert,
 * ncv > 64, fp64 vectors, the multi-vector layout, sharding over devices, HIP-graph capture, lsqr / lsmr on the same recurrence. */
#define HISPMV_GK_MAX_NCV 64
/* The workspace rule on the host (no device needed): out = {work_bytes, byte offset of V, floats between two V vectors, byte offset of
 * U, floats between two U vectors, byte offset of Gc, byte offset of Yt, byte offset of the partials (132 arrays of gp doubles up to
 * V, gp = the larger grid rounded up to 2)}.  rows or cols < 0, ncv outside 2 .. 64 -> HISPMV_EINVAL. */
int hispmv_prep_gk(int64_t rows, int64_t cols, int64_t ncv, int64_t out[8]);
/* The small SVD on the host and nothing else (no device needed): B is rows_b x cols_b, row-major with ld doubles between rows,
 * 1 <= rows_b <= 64, rows_b <= cols_b <= rows_b + 1.  s_out[rows_b] descending; Pt_out[rows_b * rows_b], row c the left vector of
 * s_out[c]; Qt_out[rows_b * cols_b], row c its right vector; res_out[c] = beta * |Pt_out[c][rows_b - 1]|; counts_out = {converged among
 * the first min(k, rows_b): res <= tol * s_out[0], Jacobi sweeps}.  Bad arguments (beta or tol negative or NaN too) -> HISPMV_EINVAL. */
int hispmv_prep_bsvd(const double* B, int64_t ld, int64_t rows_b, int64_t cols_b, int64_t k, double beta, double tol, double* s_out,
                     double* Pt_out, double* Qt_out, double* res_out, int64_t counts_out[2]);
/* out = {accepted, work_bytes, byte offset of V, V stride in floats, byte offset of U, U stride in floats, byte offset of Gc, byte
 * offset of Yt}; zeros for a handle that is not loaded or that the transposed product refuses.  A bad index, ncv outside 2 .. 64 ->
 * HISPMV_EINVAL. */
int hispmv_gk_info(const hispmv_ctx* ctx, int matrix_idx, int64_t ncv, int64_t out[8]);
/* Enqueues the open (first != 0: j0 must be 0, d_v0 the start vector of cols floats) and the steps j0 .. j1 - 1, 0 <= j0 < j1 <= ncv,
 * with no host look.  The workspace is that of the rule for ncv (2 .. 64), which is an argument because U lies behind the ncv + 1
 * vectors of V: the calls of one run give the same ncv.  Asynchronous on `stream`. */
int hispmv_gk_steps_device(hispmv_ctx* ctx, int matrix_idx, int64_t ncv, int64_t j0, int64_t j1, int first, const float* d_v0,
                           void* d_work, int64_t work_bytes, void* stream);
/* Synchronises `stream` and reads out = {steps, invariant, closed_u, breakdown, products} out of the workspace of a run on it. */
int hispmv_gk_status(hispmv_ctx* ctx, const void* d_work, void* stream, int64_t out[5]);
/* The driver above.  d_v0[cols] is the start vector (not written).  vectors != 0: d_u takes `found` left vectors ld_u >= rows floats
 * apart, d_v the right vectors ld_v >= cols floats apart; vectors == 0: the two finishing rotations are skipped and d_u, d_v are not
 * looked at.  s_out and res_out are host doubles [k].  *result is hispmv_eigsh_result, `scale` = s_0 of the last look.  The call
 * returns with *result filled and the stream synchronised; it allocates and frees its pinned buffer itself. */
int hispmv_svds_device(hispmv_ctx* ctx, int matrix_idx, int64_t k, int64_t ncv, double tol, int64_t max_products, const float* d_v0,
                       int vectors, float* d_u, int64_t ld_u, float* d_v, int64_t ld_v, double* s_out, double* res_out, void* d_work,
                       int64_t work_bytes, void* stream, hispmv_eigsh_result* result);

/* ---- getters (HiSpmvHandle getters, spmv-helper.cpp:752-810) ------------------------------------ */
typedef struct hispmv_matrix_info {
    int32_t rows, cols;
    int64_t nnz;            /* getNNZ */
    int32_t is_dense;       /* isDense */
    int32_t loaded;
    int64_t n_slices;       /* wavefront slices (the analogue of getRunLength's beats) */
    int64_t n_elems;        /* stream elements before tail padding (nnz + empty-row fillers) */
    int64_t n_split_rows;   /* rows shared between slices (the analogue of the shared-row list) */
    int64_t device_bytes;   /* bytes this handle takes in the arena */
    double prep_seconds;    /* host preprocessing time ("Pre-processing Time") */
    int32_t block_threads;  /* launch plan chosen at load time: workgroup size, */
    int32_t group_slices;   /*   slices per workgroup (format 1: K-slots per block of the tile geometry, 28 or 13), */
    int32_t lds_bytes;      /*   LDS bytes of the x window (0 = x gathered through L2) */
    int32_t col_tiles;      /* number of column tiles (1 = untiled) */
    int32_t carry_lookback; /* 1 = rows shared between slices are merged inside the launch (look-back), 0 = fix-up launch */
    int32_t col_tile_width; /* columns per tile when col_tiles > 1, else 0 */
    int32_t col_tile_base;  /* tile t covers columns [base + t*width, base + (t+1)*width) of the range holding 99.8 % of the
                               elements; the first tile also takes every column below, the last every column above */
    int32_t compact_slices; /* slices stored with 6-byte elements (fp32 value + 16-bit {rowEnd, index into the LDS window of x -- or into the
                               owning wavefront's stray area behind it, for up to 64 elements per slice whose column lies outside the window});
                               the others take 8 bytes per element (32-bit meta) */
    int32_t format;         /* 0 = slice stream (rows in order, segmented scan); 1 = transposed tile stream (scattered short-row matrices:
                               row tiles with LDS accumulators, elements streamed sorted by column, transposed through LDS; n_slices then
                               counts its 1024-word slices, n_split_rows the rows cut into pieces: longer than a tile and a quarter) */
    float tts_lines_per_gather;  /* format 1: distinct 128-byte lines of x per 64-lane gather (64 = no lane shares a line) */
    int32_t tile_kind;      /* col_tiles > 1: 1 = tiles are column ranges (col_tile_base / col_tile_width above); 2 = BAND tiles: the same
                               base / width describe ranges of the OFFSET col - row*cols/rows from the scaled diagonal (a banded matrix
                               whose band is wider than an LDS window, cut along the diagonal); 3 = STRAY SPLIT: part 0 holds the elements that lie
                               inside the x window of their workgroup (6-byte elements from LDS), part 1 the few per cent that do not (gathered
                               through L2 into a partial vector the tail launch adds); 0 = untiled */
    int32_t batch_group_slices; /* > 0: the handle also holds a BATCH LAYOUT of its slices -- groups of this many slices (twice group_slices,
                               half as many workgroups) that hispmv_spmv_device_batch uses when a call shares the chip between its matrices
                               (two launch lanes); single launches keep group_slices.  0 = none.  Same results bit for bit. */
} hispmv_matrix_info;
int hispmv_get_matrix_info(const hispmv_ctx* ctx, int matrix_idx, hispmv_matrix_info* out);
int hispmv_num_matrices(const hispmv_ctx* ctx);

/* ---- host-only preprocessor access (no device needed): lets tests check the CSR indices and the
 * packed stream against the oracle on a CPU-only box.  Mirrors HiSpmvHandle::getPreparedMtx
 * (spmv-helper.cpp:800-802). ------------------------------------------------------------------- */
typedef struct hispmv_prep hispmv_prep;
int hispmv_prep_from_coo(hispmv_prep** out, const int32_t* coo_rows, const int32_t* coo_cols,
                         const float* coo_values, int64_t nnz, int32_t rows, int32_t cols);
int hispmv_prep_from_mtx(hispmv_prep** out, const char* mtx_path, int flavor);
/* The same object with COO -> CSR (stable radix sort) and CSR -> slice stream computed ON THE DEVICE `device_id`
 * (retires the hotspot of common/src/spmv-helper.cpp:139-227): CSR, words, headers and split-row list
 * are byte-identical to hispmv_prep_from_coo's.  seconds (may be NULL) = {upload, COO->CSR on the device, row offsets on
 * the host, stream on the device, downloads}.  create_sparse_handle uses this path from 2 M entries
 * (HISPMV_PREP=host|device|auto). */
int hispmv_prep_from_coo_device(hispmv_prep** out, int device_id, const int32_t* coo_rows, const int32_t* coo_cols,
                                const float* coo_values, int64_t nnz, int32_t rows, int32_t cols, double seconds[5]);
void hispmv_prep_free(hispmv_prep* p);
const char* hispmv_prep_last_error(void);
/* dims[0..7] = rows, cols, nnz, n_elems, n_slices, slice_elems, n_split_rows, stream_bytes */
int hispmv_prep_dims(const hispmv_prep* p, int64_t dims[8]);
const int64_t* hispmv_prep_csr_row_ptr(const hispmv_prep* p);
const int32_t* hispmv_prep_csr_col(const hispmv_prep* p);
const float* hispmv_prep_csr_val(const hispmv_prep* p);
const uint64_t* hispmv_prep_words(const hispmv_prep* p);     /* n_slices * slice_elems 64-bit words */
const int32_t* hispmv_prep_slice_hdr(const hispmv_prep* p);   /* n_slices x {row_base, chain_len, x_base, x_span} */
const int32_t* hispmv_prep_fix(const hispmv_prep* p);         /* n_split_rows x {row, first_slice, len, 0} */

/* Launch plan the loader would choose for this stream on a device with n_cus compute units (host-only, no
 * device needed): plan[0..5] = workgroup threads, slices per workgroup, x-window LDS floats, row-total LDS
 * floats per wavefront, workgroups, total dynamic LDS bytes per workgroup. */
int hispmv_prep_plan(const hispmv_prep* p, int n_cus, int64_t plan[6]);

/* The widest pass hispmv_linear_device (out[0]; beta != 0) and hispmv_linear_device_t (out[1]) take for num_vecs vectors on this
 * stream as a single-part handle planned for n_cus compute units: 4, 2 or 1 (host-only, no device needed). */
int hispmv_prep_vector_widths(const hispmv_prep* p, int n_cus, int64_t num_vecs, int64_t out[2]);

/* The FORMAT AND TILING the loader would choose for this matrix on a device with n_cus compute units -- the MI355X analogue of
 * the reference's per-matrix configuration search (automation_tool/src/dse.py:23-95) -- computed by the same host-only function
 * hispmv_create_sparse_handle* calls (hispmv_amd/csrc/hispmv_choose.cpp; no device needed).  out[0..13] = format (0 slice
 * stream, 1 transposed tile stream), tile kind (0 untiled, 1 column tiles, 2 band tiles), parts, tile width, tile base, 1 if the
 * tiles gather x through L2 (XCD-pinned in a batch call), workgroup threads / slices per workgroup (tile stream: K-slots per
 * block) / LDS window floats of part 0, slices, stream elements, rows cut between slices (pieces), 1000 x lines per gather of a
 * tile stream, elements that gather x through L2.  Honours the HISPMV_FORMAT / _BAND_TILES / _TTS_GEOMETRY / _COL_TILE_BYTES /
 * _TTS_MIN_NNZ switches like the loader. */
int hispmv_prep_choose_format(const hispmv_prep* p, int n_cus, int64_t out[16]);

/* The order of the step kernel's queue (hispmv_spmv_device_batch, hispmv_batch_call_info), host-only (hispmv_choose.cpp:
 * order_step_queue, the function the batch planner calls): n_slice slice items and n_tile tiles with a cost each (microseconds of a
 * CU), n_wg workgroups; mode 0 = long tiles (> a quarter of the step) alternating with the longest slice items, then longest first
 * (default), 1 = longest first, 2 = tiles then slice items as given (3, 4, 16*t + s: experiments -- two / three slice items per long tile,
 * cycles of t long tiles and s slice items).  out_class[i] (0 slice item, 1 tile) and out_index[i] name the
 * item at queue position i (n_slice + n_tile positions).  No reference counterpart (the reference runs one matrix at a time). */
int hispmv_prep_step_queue(const double* slice_costs, int32_t n_slice, const double* tile_costs, int32_t n_tile, int32_t n_wg, int32_t mode,
                           int32_t* out_class, int32_t* out_index);

/* inside[nnz] (CSR order): 1 for the entries whose 64-byte block of x is held by the x window of their workgroup under the launch
 * plan for n_cus compute units, 0 for the entries that gather through L2 -- the criterion by which the loader splits a matrix with a
 * few per cent of stray couplings into a windowed part and a stray part (hispmv_matrix_info.tile_kind 3). */
int hispmv_prep_window_membership(const hispmv_prep* p, int n_cus, uint8_t* inside);

/* The swapped COO of a CSR input in INPUT ORDER -- what hispmv_create_sparse_handle_from_csr makes a stored transpose from
 * (HISPMV_TRANSPOSABLE_COMPANION): for entry k of col_idx, in ascending k and before any per-row sort, out_rows[k] = col_idx[k] and
 * out_cols[k] = the row whose row_ptr range holds k.  Both outputs hold row_ptr[rows] entries.  row_ptr must start at 0 and be
 * non-decreasing -> HISPMV_EINVAL otherwise. */
int hispmv_prep_swapped_coo_from_csr(const int32_t* row_ptr, const int32_t* col_idx, int32_t rows, int32_t* out_rows, int32_t* out_cols);

/* Applies that plan to the prepared stream IN PLACE (the words of LDS-staged groups then carry window
 * indices instead of columns -- or 0x40000000 | column for the elements of the group whose 64-byte block of x
 * is not in the window) and exposes its tables: groups = n x {frag_begin, frag_count, lds_floats, elements
 * outside the window}, frags = m x {col_start, len, lds_off, 0}.  counts[0..1] = n, m. */
int hispmv_prep_apply_plan(hispmv_prep* p, int n_cus, int64_t counts[2]);
const int32_t* hispmv_prep_groups(const hispmv_prep* p);
/* Host-only counterpart of hispmv_set_value_storage: HISPMV_VALUES_BF16 rounds the prepared values in place (CSR and stream words;
 * call it before hispmv_prep_apply_plan) and makes hispmv_prep_device_stream pack every compact group as HALF slices -- 1024 x 16-byte
 * pieces {v0 | v1 << 16, v2 | v3 << 16, m0 | m1 << 16, m2 | m3 << 16} of four consecutive elements (bf16 values, the compact metas),
 * 4096 B per slice, groups[].w |= 4; hispmv_prep_build_tts then carries the rounded values.  Back to HISPMV_VALUES_FP32 restores the
 * layout, not the values. */
int hispmv_prep_set_value_storage(hispmv_prep* p, int storage);
/* The planned stream in its DEVICE LAYOUT (hispmv_amd/csrc/hispmv_format.h; call hispmv_prep_apply_plan first): counts = {bytes, groups,
 * compact slices, slices of groups with stray slots, LDS floats of the wavefronts' stray areas, LDS floats of the x window}.  Arrays:
 * 0 = the slices, group after group (compact: 1024 x fp32 then 1024 x u16 {rowEnd:1 | LDS index:15}; wide: 1024 x u32 metas);
 * 1 = groups x {frag_begin, frag_count, offset of the group's first slice / 2048, 1 = compact | 2 = stray slots | 4 = half}; 2 = slices x 64 stray
 * columns (0xffffffff = unused; empty when no group has stray slots).  For tests: the packer without a device. */
int hispmv_prep_device_stream(hispmv_prep* p, int64_t counts[6]);
const void* hispmv_prep_device_array(const hispmv_prep* p, int which);
/* The same layout written on the DEVICE from the planned host words (the kernel hispmv_load_matrices runs with HISPMV_LAYOUT=device):
 * after hispmv_prep_apply_plan + hispmv_prep_device_stream; bytes_out takes counts[0] bytes, stray_cols_out slices x 64 u32 (may be
 * NULL when counts[4] == 0).  For tests (device == host, byte for byte); HISPMV_EDEVICE without a GPU. */
int hispmv_prep_device_stream_on_device(hispmv_prep* p, int device_id, uint8_t* bytes_out, uint32_t* stray_cols_out);
const int32_t* hispmv_prep_frags(const hispmv_prep* p);

/* Every device layout of the handle hispmv_create_sparse_handle makes from this COO input on a device with n_cus CUs (the parts'
 * slice layouts, each followed by its batch layout if any, or the tile streams' words), packed twice by the same host path: with the
 * real values and -- as for a handle created with value updates on -- with the index payloads bits(k + 1) of the input positions.
 * counts = {layout bytes, map slots, chunks, slots an update writes, format, tile kind, parts, batch layouts}; arrays of
 * hispmv_prep_value_array: 0 real layouts, 1 payload layouts, 2 the map read out of 1 (int32; 0 = filler / padding), 3 per chunk of
 * 1024 map slots the byte offsets {first destination, second destination or -1} (int64 x 2).  For tests, no device needed. */
int hispmv_prep_value_layouts(hispmv_prep** out, const int32_t* coo_rows, const int32_t* coo_cols, const float* coo_values, int64_t nnz,
                              int32_t rows, int32_t cols, int n_cus, int64_t counts[8]);
/* The same with a value storage (HISPMV_VALUES_FP32: exactly the call above).  HISPMV_VALUES_BF16: the layouts of an updatable bf16
 * handle (HISPMV_VALUE_UPDATES_ANY_STORAGE) -- array 0 packed from R(values), half groups included; array 1 the same layouts packed
 * with the payloads (its half slices hold no usable values: an update overwrites them); array 2 the map as the loader uploads it,
 * word for word that of the fp32 call; array 4 one int32 kind per chunk destination, in the shape of array 3: 0 = 1024 fp32 slots,
 * 1 = a half slice, whose values are the first 8 bytes of each 16-byte piece (0 where array 3 holds -1). */
int hispmv_prep_value_layouts_storage(hispmv_prep** out, const int32_t* coo_rows, const int32_t* coo_cols, const float* coo_values, int64_t nnz,
                                      int32_t rows, int32_t cols, int n_cus, int storage, int64_t counts[8]);
const void* hispmv_prep_value_array(const hispmv_prep* p, int which);

/* Number of device / pinned-memory frees the runtime rejected since the library was loaded (a pointer released twice
 * or never allocated); 0 in a correct run.  For tests. */
int64_t hispmv_free_failures(void);

/* The transposed tile stream of the prepared matrix (the second device format: hispmv_matrix_info.format == 1), packed
 * on the host: counts = {tiles, blocks, column-order slices of 1024 words, row-major chunks of 1024 slots, fillers,
 * padding words, max rows of a tile, max slots of a block}; arrays: 0 words (per slice 1024 x fp32 then 1024 x
 * {col_off:16 | slot:16}), 1 col_base (int32 per slice), 2 flags (64 x u16 per chunk), 3 chunk_info ({rows ending
 * before, chain_len} per chunk), 4 tiles ({row0, n_rows, block_begin, n_blocks}; row0 < 0: carry tile), 5 blocks (8 x int32: slice_begin,
 * n_slices, chunk_begin, n_chunks, n_slots, 0, 0, 0).  target_tile_elems 0 = the loader's choice; small_geometry: 0 = tiles of
 * <= 8192 rows and blocks of <= 28 K slots (one workgroup per CU), 1 = <= 4096 rows / 13 K slots (two per CU: what the
 * loader takes when a gather of the tall geometry touches <= 8 lines; hispmv_matrix_info.group_slices = 28 or 13), 2 + q =
 * column part q (0 or 1) of the TALL geometry as the loader builds it for 256 CUs: the matrix cut at the column that halves
 * its elements, each half packed into tiles of <= 16384 rows and blocks of <= 23 K slots in which rows absent from a block
 * own a slot but no word (hispmv_matrix_info.group_slices = 23, col_tiles = 2: part 0 gives alpha*A_0*x + beta*bias, part 1
 * the partial vector alpha*A_1*x that the merge launch adds), 8 + q = column part q of the same geometry with GAP-CODED row
 * ends (HISPMV_TTS_GEOMETRY=tallgap): absent rows own no slot, a row end's 2-bit code = bit of array 2 | bit of array 7 << 1
 * (1 end, next row present; 2 end, one absent row follows; 3 end, two follow), chunk_info = {last slot-owning row before
 * the chunk, chain_len | first code << 16}; array 7 = flags_hi (64 x u16 per chunk; null for the other geometries). */
int hispmv_prep_build_tts(hispmv_prep* p, int64_t target_tile_elems, int small_geometry, int64_t counts[8], double* lines_per_gather);
const void* hispmv_prep_tts_array(const hispmv_prep* p, int which);
/* Rows longer than two tiles are cut into pieces, each a tile of its own; all but a row's last piece are carry tiles
 * (tiles[.].row0 = -(carry index + 1)) whose sums a fix-up launch adds: counts = {rows cut, carry tiles}; array 6 of
 * hispmv_prep_tts_array = {row, first carry, carries, 0} per row cut (int32 x 4). */
int hispmv_prep_tts_pieces(const hispmv_prep* p, int64_t counts[2]);

/* OpenMP threads the host preprocessor uses: the CPUs this process may use (cgroup cpu.max quota, e.g. 16 of the 256 a GPU
 * box shows), set once at the first call of the library unless OMP_NUM_THREADS is given. */
int hispmv_host_threads(void);

/* Library identification: "hispmv-amd <version> gfx950". */
const char* hispmv_version(void);

#ifdef __cplusplus
}
#endif
#endif /* HISPMV_H */
