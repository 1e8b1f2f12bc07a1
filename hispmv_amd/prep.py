"""Host-only access to the preprocessor (COO / MatrixMarket -> CSR -> slice stream) through the
C ABI's ``hispmv_prep_*`` entry points.  No device is needed; tests use it to compare the CSR
indices and the packed stream against the oracle on a CPU-only box.  Mirrors
``HiSpmvHandle::getPreparedMtx`` (common/src/spmv-helper.cpp:800-802)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from ._lib import lib, EIGSH_WHICH, HISPMV_OK, VALUE_STORAGES


@dataclass
class Prepared:
    rows: int
    cols: int
    nnz: int
    n_elems: int
    n_slices: int
    slice_elems: int
    stream_bytes: int
    row_ptr: np.ndarray    # int64 [rows+1]
    col_idx: np.ndarray    # int32 [nnz]
    values: np.ndarray     # float32 [nnz]
    words: np.ndarray      # uint64 [n_slices*slice_elems]: low 32 = fp32 bits, high 32 = rowEnd<<31 | col
    hdr: np.ndarray        # int32 [n_slices,4]: row_base, chain_len, x_base, x_span
    fix: np.ndarray        # int32 [n_split,4]: row, first_slice, len, 0
    plan: dict = None      # launch plan on a 256-CU device: threads, group_slices, lds_floats, ytile_floats, groups, lds_bytes
    staged_words: np.ndarray = None   # the stream as the device gets it: staged groups carry window indices, not columns
    groups: np.ndarray = None         # int32 [n_groups,4]: frag_begin, frag_count, lds_floats, 0
    frags: np.ndarray = None          # int32 [n_frags,4]: col_start, len, lds_off, 0
    tts: dict = None                  # the transposed tile stream (prep_from_coo(..., tts=True)): arrays + counts


def _collect_tts(p, target, geometry: int = 0):
    """geometry: 0 standard (8 K-row tiles), 1 small, "tall" = the list of the tall geometry's column parts (codes 2 + q)."""
    if isinstance(target, tuple):
        target, geometry = target
    if geometry in ("tall", "paired", "tallgap"):
        return [_collect_tts(p, target, {"tall": 2, "paired": 4, "tallgap": 8}[geometry] + q) for q in range(2)]
    geometry = 6 if geometry == "zerofill" else int(geometry)
    cnt = (C.c_int64 * 8)()
    lpg = C.c_double()
    if lib.hispmv_prep_build_tts(p, int(target), geometry, cnt, C.byref(lpg)) != HISPMV_OK:
        raise ValueError(lib.hispmv_prep_last_error().decode())
    tiles, blocks, slices, chunks, fillers, pads, max_rows, max_slots = (int(v) for v in cnt)

    def arr(which, n, dt, shape=None):
        ptr = lib.hispmv_prep_tts_array(p, which)
        if n == 0 or not ptr:
            a = np.zeros(0, dtype=dt)
        else:
            a = np.frombuffer((C.c_char * (n * np.dtype(dt).itemsize)).from_address(ptr), dtype=dt).copy()
        return a.reshape(shape) if shape else a
    pc = (C.c_int64 * 2)()
    lib.hispmv_prep_tts_pieces(p, pc)
    gap = geometry >= 8
    return dict(zero_fill=2 <= geometry < 8, flags_hi=arr(7, chunks * 64, np.uint16, (-1, 64)) if gap else None, n_tiles=tiles, n_blocks=blocks, n_slices=slices, n_chunks=chunks, fillers=fillers, pad_words=pads, max_rows=max_rows,
                max_slots=max_slots, lines_per_gather=float(lpg.value), n_carry=int(pc[1]), fix=arr(6, int(pc[0]) * 4, np.int32, (-1, 4)),
                words=arr(0, slices * 2048, np.uint32, (-1, 2, 1024)), col_base=arr(1, slices, np.int32), flags=arr(2, chunks * 64, np.uint16, (-1, 64)),
                chunk_info=arr(3, chunks * 2, np.int32, (-1, 2)), tiles=arr(4, tiles * 4, np.int32, (-1, 4)), blocks=arr(5, blocks * 8, np.int32, (-1, 8)))


def _collect(p, tts=None) -> Prepared:
    d = (C.c_int64 * 8)()
    lib.hispmv_prep_dims(p, d)
    rows, cols, nnz, n_elems, n_slices, se, n_fix, nbytes = (int(v) for v in d)

    def arr(ptr, n, shape=None):
        if n == 0:   # an empty std::vector hands out a NULL data pointer
            a = np.zeros(0, dtype=np.ctypeslib.as_ctypes_type(ptr._type_))
        else:
            a = np.ctypeslib.as_array(ptr, shape=(n,)).copy()
        return a.reshape(shape) if shape else a
    out = Prepared(rows, cols, nnz, n_elems, n_slices, se, nbytes,
                   arr(lib.hispmv_prep_csr_row_ptr(p), rows + 1),
                   arr(lib.hispmv_prep_csr_col(p), nnz),
                   arr(lib.hispmv_prep_csr_val(p), nnz),
                   arr(lib.hispmv_prep_words(p), n_slices * se),
                   arr(lib.hispmv_prep_slice_hdr(p), n_slices * 4, (-1, 4)),
                   arr(lib.hispmv_prep_fix(p), n_fix * 4, (-1, 4)))
    pl = (C.c_int64 * 6)()
    if lib.hispmv_prep_plan(p, 256, pl) == HISPMV_OK:
        out.plan = dict(zip(("threads", "group_slices", "lds_floats", "ytile_floats", "groups", "lds_bytes"), (int(v) for v in pl)))
    cnt = (C.c_int64 * 2)()
    if lib.hispmv_prep_apply_plan(p, 256, cnt) == HISPMV_OK:
        out.staged_words = arr(lib.hispmv_prep_words(p), n_slices * se)
        out.groups = arr(lib.hispmv_prep_groups(p), int(cnt[0]) * 4, (-1, 4))
        out.frags = arr(lib.hispmv_prep_frags(p), int(cnt[1]) * 4, (-1, 4))
    if tts is not None:
        out.tts = _collect_tts(p, tts)
    lib.hispmv_prep_free(p)
    return out


def _set_storage(p, value_storage: str) -> None:
    if value_storage not in VALUE_STORAGES:
        lib.hispmv_prep_free(p)
        raise ValueError('value_storage must be "fp32" or "bf16"')
    if lib.hispmv_prep_set_value_storage(p, VALUE_STORAGES[value_storage]) != HISPMV_OK:
        lib.hispmv_prep_free(p)
        raise ValueError(lib.hispmv_prep_last_error().decode())


def prep_from_coo(coo_rows, coo_cols, coo_values, rows: int, cols: int, tts=None, value_storage: str = "fp32") -> Prepared:
    """value_storage "bf16": the prepared values (CSR, words, tile stream) are rounded to bfloat16 (hispmv_prep_set_value_storage).
    tts: None, or the target elements per row tile of the transposed tile stream to pack as well (0 = loader's choice),
    or (target, geometry) with geometry 0 standard / 1 small / "tall" (Prepared.tts is then the list of the two column
    parts) -- see hispmv_prep_build_tts."""
    r = np.ascontiguousarray(coo_rows, dtype=np.int32)
    c = np.ascontiguousarray(coo_cols, dtype=np.int32)
    v = np.ascontiguousarray(coo_values, dtype=np.float32)
    p = C.c_void_p()
    rc = lib.hispmv_prep_from_coo(C.byref(p), C.c_void_p(r.ctypes.data), C.c_void_p(c.ctypes.data),
                                  C.c_void_p(v.ctypes.data), r.size, rows, cols)
    if rc != HISPMV_OK:
        raise ValueError(lib.hispmv_prep_last_error().decode())
    _set_storage(p, value_storage)
    return _collect(p, tts)


def prep_from_coo_device(coo_rows, coo_cols, coo_values, rows: int, cols: int, device: int = 0):
    """The same object with both heavy stages computed on the MI355X (hispmv_prep_from_coo_device) -> (Prepared, seconds
    dict).  Needs a gfx950 device."""
    r = np.ascontiguousarray(coo_rows, dtype=np.int32)
    c = np.ascontiguousarray(coo_cols, dtype=np.int32)
    v = np.ascontiguousarray(coo_values, dtype=np.float32)
    p = C.c_void_p()
    secs = (C.c_double * 5)()
    rc = lib.hispmv_prep_from_coo_device(C.byref(p), int(device), C.c_void_p(r.ctypes.data), C.c_void_p(c.ctypes.data),
                                         C.c_void_p(v.ctypes.data), r.size, rows, cols, secs)
    if rc != HISPMV_OK:
        raise ValueError(lib.hispmv_prep_last_error().decode())
    return _collect(p), dict(zip(("upload", "csr_device", "offsets_host", "stream_device", "download"), (float(x) for x in secs)))


def prep_from_mtx(path, flavor: int = 0) -> Prepared:
    p = C.c_void_p()
    rc = lib.hispmv_prep_from_mtx(C.byref(p), str(path).encode(), int(flavor))
    if rc != HISPMV_OK:
        raise OSError(lib.hispmv_prep_last_error().decode())
    return _collect(p)


FORMAT_FIELDS = ("format", "tile_kind", "parts", "tile_width", "tile_base", "l2_tiles", "threads", "group", "lds_floats", "n_slices",
                 "n_elems", "n_split", "lines_per_gather_x1000", "l2_gather_elems")


def choose_format_from_csr(row_ptr, col_idx, values, rows: int, cols: int, n_cus: int = 256) -> dict:
    """The loader's format / tiling decision for a CSR matrix on an `n_cus`-CU device (hispmv_prep_choose_format): host-only,
    the same code path hispmv_create_sparse_handle_from_csr takes.  The CSR goes in as COO triplets in row-major order."""
    rp = np.asarray(row_ptr, dtype=np.int64)
    r = np.repeat(np.arange(rows, dtype=np.int32), np.diff(rp).astype(np.int64))
    c = np.ascontiguousarray(col_idx, dtype=np.int32)
    v = np.ascontiguousarray(values, dtype=np.float32)
    p = C.c_void_p()
    rc = lib.hispmv_prep_from_coo(C.byref(p), C.c_void_p(r.ctypes.data), C.c_void_p(c.ctypes.data), C.c_void_p(v.ctypes.data), r.size, rows, cols)
    if rc != HISPMV_OK:
        raise ValueError(lib.hispmv_prep_last_error().decode())
    try:
        out = (C.c_int64 * 16)()
        if lib.hispmv_prep_choose_format(p, int(n_cus), out) != HISPMV_OK:
            raise ValueError(lib.hispmv_prep_last_error().decode())
        return dict(zip(FORMAT_FIELDS, (int(x) for x in out)))
    finally:
        lib.hispmv_prep_free(p)


def vector_widths_from_coo(coo_rows, coo_cols, coo_values, rows: int, cols: int, n_cus: int = 256, num_vecs: int = 4) -> dict:
    """{"forward", "transposed"}: the widest pass (4, 2 or 1 vectors) linear_device and linear_device_t take for `num_vecs` vectors on
    this matrix as a single-part slice stream planned for `n_cus` CUs (hispmv_prep_vector_widths): host-only."""
    r = np.ascontiguousarray(coo_rows, dtype=np.int32)
    c = np.ascontiguousarray(coo_cols, dtype=np.int32)
    v = np.ascontiguousarray(coo_values, dtype=np.float32)
    p = C.c_void_p()
    if lib.hispmv_prep_from_coo(C.byref(p), C.c_void_p(r.ctypes.data), C.c_void_p(c.ctypes.data), C.c_void_p(v.ctypes.data), r.size, rows, cols) != HISPMV_OK:
        raise ValueError(lib.hispmv_prep_last_error().decode())
    try:
        out = (C.c_int64 * 2)()
        if lib.hispmv_prep_vector_widths(p, int(n_cus), int(num_vecs), out) != HISPMV_OK:
            raise ValueError("bad vector_widths arguments")
        return {"forward": int(out[0]), "transposed": int(out[1])}
    finally:
        lib.hispmv_prep_free(p)


def window_membership(coo_rows, coo_cols, coo_values, rows: int, cols: int, n_cus: int = 256):
    """-> (inside, order): `inside[k]` for the matrix's CSR entries (1 = the entry's block of x lies in the LDS window of its
    workgroup, hispmv_prep_window_membership) and `order`, the permutation that brings the COO triplets into that CSR order."""
    r = np.ascontiguousarray(coo_rows, dtype=np.int32)
    c = np.ascontiguousarray(coo_cols, dtype=np.int32)
    v = np.ascontiguousarray(coo_values, dtype=np.float32)
    p = C.c_void_p()
    if lib.hispmv_prep_from_coo(C.byref(p), C.c_void_p(r.ctypes.data), C.c_void_p(c.ctypes.data), C.c_void_p(v.ctypes.data), r.size, rows, cols) != HISPMV_OK:
        raise ValueError(lib.hispmv_prep_last_error().decode())
    try:
        inside = np.zeros(r.size, dtype=np.uint8)
        if lib.hispmv_prep_window_membership(p, int(n_cus), C.c_void_p(inside.ctypes.data)) != HISPMV_OK:
            raise ValueError(lib.hispmv_prep_last_error().decode())
    finally:
        lib.hispmv_prep_free(p)
    return inside, np.lexsort((np.arange(r.size), c, r))     # stable: duplicates keep their input order, as in coo_to_csr


def device_layout_from_coo(coo_rows, coo_cols, coo_values, rows: int, cols: int, n_cus: int = 256, on_device: int = -1,
                           value_storage: str = "fp32") -> dict:
    """The stream of a matrix as the device gets it (hispmv_prep_device_stream), host-only: -> dict with the host words before
    planning (`words`; value_storage "bf16": with the rounded values, and the compact groups of `bytes` packed as half slices), the plan (`threads`, `group_slices`, `window_floats`, `stray_floats`, `groups`, `frags`) and the device
    arrays (`bytes` u8, `dgroups` [n,4], `stray_cols` [n_slices,64] or empty)."""
    r = np.ascontiguousarray(coo_rows, dtype=np.int32)
    c = np.ascontiguousarray(coo_cols, dtype=np.int32)
    v = np.ascontiguousarray(coo_values, dtype=np.float32)
    p = C.c_void_p()
    if lib.hispmv_prep_from_coo(C.byref(p), C.c_void_p(r.ctypes.data), C.c_void_p(c.ctypes.data), C.c_void_p(v.ctypes.data), r.size, rows, cols) != HISPMV_OK:
        raise ValueError(lib.hispmv_prep_last_error().decode())
    _set_storage(p, value_storage)
    try:
        d = (C.c_int64 * 8)()
        lib.hispmv_prep_dims(p, d)
        n_slices, se = int(d[4]), int(d[5])
        words = np.ctypeslib.as_array(lib.hispmv_prep_words(p), shape=(n_slices * se,)).copy()
        pl = (C.c_int64 * 6)()
        lib.hispmv_prep_plan(p, int(n_cus), pl)
        cnt = (C.c_int64 * 2)()
        lib.hispmv_prep_apply_plan(p, int(n_cus), cnt)
        groups = np.ctypeslib.as_array(lib.hispmv_prep_groups(p), shape=(int(cnt[0]) * 4,)).copy().reshape(-1, 4) if cnt[0] else np.zeros((0, 4), np.int32)
        frags = np.ctypeslib.as_array(lib.hispmv_prep_frags(p), shape=(int(cnt[1]) * 4,)).copy().reshape(-1, 4) if cnt[1] else np.zeros((0, 4), np.int32)
        dc = (C.c_int64 * 6)()
        if lib.hispmv_prep_device_stream(p, dc) != HISPMV_OK:
            raise ValueError(lib.hispmv_prep_last_error().decode())

        def arr(which, n, dt):
            ptr = lib.hispmv_prep_device_array(p, which)
            return np.frombuffer((C.c_char * (n * np.dtype(dt).itemsize)).from_address(ptr), dtype=dt).copy() if (n and ptr) else np.zeros(0, dt)
        n_groups = int(dc[1])
        stray_floats = int(dc[4])
        extra = {}
        if on_device >= 0:          # the loader's layout kernel over the same planned words (needs a GPU): bytes_device / stray_cols_device
            bd = np.zeros(int(dc[0]), np.uint8)
            sd = np.zeros((n_slices, 64) if stray_floats else (0, 64), np.uint32)
            if lib.hispmv_prep_device_stream_on_device(p, int(on_device), C.c_void_p(bd.ctypes.data), C.c_void_p(sd.ctypes.data) if stray_floats else None) != HISPMV_OK:
                raise RuntimeError(lib.hispmv_prep_last_error().decode())
            extra = dict(bytes_device=bd, stray_cols_device=sd)
        return dict(**extra, words=words, n_slices=n_slices, threads=int(pl[0]), group_slices=int(pl[1]), window_floats=int(dc[5]), stray_floats=stray_floats,
                    compact_slices=int(dc[2]), stray_slices=int(dc[3]), groups=groups, frags=frags, bytes=arr(0, int(dc[0]), np.uint8),
                    dgroups=arr(1, n_groups * 4, np.int32).reshape(-1, 4),
                    stray_cols=arr(2, n_slices * 64 if stray_floats else 0, np.uint32).reshape(-1, 64))
    finally:
        lib.hispmv_prep_free(p)


def step_queue(slice_costs, tile_costs, n_wg: int = 256, mode: int = 0):
    """The order of the step kernel's queue (hispmv_prep_step_queue: the function the batch planner calls), host-only.
    -> (classes, indices): per queue position 0 = slice item / 1 = tile, and its index in that class's cost list."""
    a = np.ascontiguousarray(slice_costs, dtype=np.float64)
    b = np.ascontiguousarray(tile_costs, dtype=np.float64)
    n = a.size + b.size
    cls = np.zeros(n, np.int32)
    idx = np.zeros(n, np.int32)
    rc = lib.hispmv_prep_step_queue(C.c_void_p(a.ctypes.data) if a.size else None, a.size, C.c_void_p(b.ctypes.data) if b.size else None, b.size,
                                    int(n_wg), int(mode), C.c_void_p(cls.ctypes.data) if n else None, C.c_void_p(idx.ctypes.data) if n else None)
    if rc != HISPMV_OK:
        raise ValueError("hispmv_prep_step_queue: invalid argument")
    return cls, idx


def spmm_tiles(cols: int, num_vecs: int, ld=None, align_bytes: int = 16) -> dict:
    """The vector tiles of a wide call (hispmv_prep_spmm_tiles), host-only: {"vl", "tiles", "last_vecs", "vl_last"} for num_vecs
    vectors against a matrix of `cols` columns, leading dimension ld (default num_vecs), pointers aligned to align_bytes."""
    out = (C.c_int64 * 4)()
    rc = lib.hispmv_prep_spmm_tiles(int(cols), int(num_vecs), int(num_vecs if ld is None else ld), int(align_bytes), out)
    if rc != HISPMV_OK:
        raise ValueError("hispmv_prep_spmm_tiles: cols, num_vecs, ld and align_bytes must be at least 1, ld at least num_vecs")
    return {"vl": int(out[0]), "tiles": int(out[1]), "last_vecs": int(out[2]), "vl_last": int(out[3])}


def spmm_bf16_tiles(cols: int, num_vecs: int, ld=None, align_bytes: int = 16) -> dict:
    """The vector tiles of a wide call with bf16 activations (hispmv_prep_spmm_bf16_tiles), host-only: {"vb", "tiles", "last_vecs",
    "vb_last"} for num_vecs vectors against a matrix of `cols` columns, leading dimension ld (default num_vecs, in elements), pointers
    aligned to align_bytes.  A lane owns vb in {8, 4, 2, 1} bf16, a tile is 64 * vb vectors."""
    out = (C.c_int64 * 4)()
    rc = lib.hispmv_prep_spmm_bf16_tiles(int(cols), int(num_vecs), int(num_vecs if ld is None else ld), int(align_bytes), out)
    if rc != HISPMV_OK:
        raise ValueError("hispmv_prep_spmm_bf16_tiles: cols, num_vecs, ld and align_bytes must be at least 1, ld at least num_vecs")
    return {"vb": int(out[0]), "tiles": int(out[1]), "last_vecs": int(out[2]), "vb_last": int(out[3])}


def krylov_groups(n: int) -> int:
    """The workgroups of a pass of the Krylov layer over n elements, which are the fp64 partials of a dot product: chunks of 1024
    elements, at most 1024 workgroups, workgroup g taking chunks g, g + groups, ...  The rule of hispmv_prep_krylov_groups, restated
    here (tests compare the two): the order of a dot product's sum depends on n through it alone."""
    if n < 0:
        raise ValueError("krylov_groups: n must not be negative")
    return min((int(n) + 1023) // 1024, 1024)


def krylov_multi(n: int, num_vecs: int) -> dict:
    """The layout rule of the multi-right-hand-side Krylov entries (hispmv_prep_krylov_multi), host-only: {"groups", "ld", "state_bytes",
    "partial_bytes"} for num_vecs columns of n rows -- one workgroup and one fp64 partial per chunk of 1024 rows (n <= 2^20, so the
    order of a column's dot product is that of krylov_groups(n)), the workspace's leading dimension (num_vecs rounded up to 4), the
    bytes of the columns' scalar blocks and of the partials; the residual R lies behind the two."""
    out = (C.c_int64 * 4)()
    if lib.hispmv_prep_krylov_multi(int(n), int(num_vecs), out) != HISPMV_OK:
        raise ValueError("hispmv_prep_krylov_multi: 0 <= n <= 2^20 and 1 <= num_vecs <= 2^20")
    return {"groups": int(out[0]), "ld": int(out[1]), "state_bytes": int(out[2]), "partial_bytes": int(out[3])}


def gmres(n: int, restart: int, with_minv: bool = False) -> dict:
    """The workspace rule of restarted GMRES (hispmv_prep_gmres), host-only: {"work_bytes", "v_offset", "stride", "groups", "dot_tile",
    "launches_per_iteration", "launches_per_cycle", "basis_vectors"} for a system of n unknowns -- the bytes a solve needs, where the
    basis lies and how many floats apart its vectors are, the partials of a dot product, how many basis vectors one pass of the
    multi-dot kernel accumulates per thread, the vector kernels of an inner iteration and of a cycle besides, and restart + 1."""
    out = (C.c_int64 * 8)()
    if lib.hispmv_prep_gmres(int(n), int(restart), int(bool(with_minv)), out) != HISPMV_OK:
        raise ValueError("hispmv_prep_gmres: n >= 0 and 1 <= restart <= 64")
    keys = ("work_bytes", "v_offset", "stride", "groups", "dot_tile", "launches_per_iteration", "launches_per_cycle", "basis_vectors")
    return dict(zip(keys, (int(x) for x in out)))


def lanczos(n: int, ncv: int) -> dict:
    """The workspace rule of thick-restart Lanczos (hispmv_prep_lanczos), host-only: {"work_bytes", "v_offset", "stride", "groups",
    "hc_offset", "yt_offset", "launches_per_step", "basis_vectors"} for a matrix of order n and ncv basis vectors -- the bytes a run
    needs, where the basis lies and how many floats apart its vectors are, the partials of a dot product, where Hc lies (64 columns of
    66 doubles, the 66 betas right behind them) and the fp32 coefficients of the last rotation, the launches of a step with its product,
    and ncv + 1."""
    out = (C.c_int64 * 8)()
    if lib.hispmv_prep_lanczos(int(n), int(ncv), out) != HISPMV_OK:
        raise ValueError("hispmv_prep_lanczos: n >= 0 and 2 <= ncv <= 64")
    keys = ("work_bytes", "v_offset", "stride", "groups", "hc_offset", "yt_offset", "launches_per_step", "basis_vectors")
    return dict(zip(keys, (int(x) for x in out)))


def ritz(H, k: int, which: str, beta: float, tol: float) -> dict:
    """The Ritz step of the eigensolver on the host (hispmv_prep_ritz): the eigenvalues of the symmetric float64 matrix H (m x m,
    m <= 64) by cyclic Jacobi, ordered by `which` ("LA" largest first, "SA" smallest first, "LM" largest magnitude first).  Returns
    {"theta" [m], "Yt" [m, m] (row c the eigenvector of theta[c]), "res" [m] = beta * |Yt[:, m - 1]|, "converged" (how many of the
    first min(k, m) have res <= tol * max |theta|), "sweeps"}."""
    H = np.ascontiguousarray(H, dtype=np.float64)
    if H.ndim != 2 or H.shape[0] != H.shape[1] or which not in EIGSH_WHICH:
        raise ValueError('hispmv_prep_ritz: H must be square and which "LA", "SA" or "LM"')
    m = H.shape[0]
    theta, Yt, res = np.zeros(m, np.float64), np.zeros((m, m), np.float64), np.zeros(m, np.float64)
    counts = (C.c_int64 * 2)()
    dp = C.POINTER(C.c_double)
    rc = lib.hispmv_prep_ritz(H.ctypes.data_as(dp), m, m, int(k), EIGSH_WHICH[which], float(beta), float(tol), theta.ctypes.data_as(dp), Yt.ctypes.data_as(dp),
                              res.ctypes.data_as(dp), counts)
    if rc != HISPMV_OK:
        raise ValueError("hispmv_prep_ritz: 1 <= m <= 64, k >= 1 and tol >= 0")
    return {"theta": theta, "Yt": Yt, "res": res, "converged": int(counts[0]), "sweeps": int(counts[1])}


def gk(rows: int, cols: int, ncv: int) -> dict:
    """The workspace rule of thick-restart Golub-Kahan (hispmv_prep_gk), host-only: {"work_bytes", "v_offset", "v_stride", "u_offset",
    "u_stride", "gc_offset", "yt_offset", "part_offset"} for a rows x cols matrix and ncv basis vectors -- the bytes a run needs, where
    V (ncv + 1 vectors of cols floats) and U (ncv vectors of rows floats) lie and how many floats apart their vectors are, where Gc lies
    (64 columns of 66 doubles, the 66 alphas and the 66 betas right behind them), the fp32 coefficients of the last rotation, and the
    partials: 132 arrays between part_offset and v_offset, each as long as the larger of the two sides' grids rounded up to 2."""
    out = (C.c_int64 * 8)()
    if lib.hispmv_prep_gk(int(rows), int(cols), int(ncv), out) != HISPMV_OK:
        raise ValueError("hispmv_prep_gk: rows >= 0, cols >= 0 and 2 <= ncv <= 64")
    keys = ("work_bytes", "v_offset", "v_stride", "u_offset", "u_stride", "gc_offset", "yt_offset", "part_offset")
    return dict(zip(keys, (int(x) for x in out)))


def bsvd(B, k: int, beta: float, tol: float) -> dict:
    """The small SVD of the singular-value solver on the host (hispmv_prep_bsvd): B = P diag(s) Q^T for the float64 matrix B
    (m x m or m x (m + 1), m <= 64) by one-sided Jacobi, s descending.  Returns {"s" [m], "Pt" [m, m] (row c the left vector of s[c]),
    "Qt" [m, cols] (row c its right vector), "res" [m] = beta * |Pt[:, m - 1]|, "converged" (how many of the first min(k, m) have
    res <= tol * s[0]), "sweeps"}."""
    B = np.ascontiguousarray(B, dtype=np.float64)
    if B.ndim != 2:
        raise ValueError("hispmv_prep_bsvd: B must be a matrix")
    m, cols = B.shape
    s, Pt, Qt, res = np.zeros(max(m, 1), np.float64), np.zeros((max(m, 1), max(m, 1)), np.float64), np.zeros((max(m, 1), max(cols, 1)), np.float64), np.zeros(max(m, 1), np.float64)
    counts = (C.c_int64 * 2)()
    dp = C.POINTER(C.c_double)
    rc = lib.hispmv_prep_bsvd(B.ctypes.data_as(dp), cols, m, cols, int(k), float(beta), float(tol), s.ctypes.data_as(dp), Pt.ctypes.data_as(dp),
                              Qt.ctypes.data_as(dp), res.ctypes.data_as(dp), counts)
    if rc != HISPMV_OK:
        raise ValueError("hispmv_prep_bsvd: 1 <= m <= 64, m <= cols <= m + 1, k >= 1, beta >= 0 and tol >= 0")
    return {"s": s, "Pt": Pt, "Qt": Qt, "res": res, "converged": int(counts[0]), "sweeps": int(counts[1])}


def block_jacobi(n: int, block_size: int) -> dict:
    """The layout rule of a block-Jacobi buffer (hispmv_prep_block_jacobi), host-only: {"n_blocks", "pre_bytes", "flags_offset",
    "block_floats"} for a system of n unknowns in blocks of block_size (4, 8, 16, 32) -- ceil(n / block_size) blocks of block_size^2
    floats each, row-major, then one int32 flag per block at flags_offset, pre_bytes in all (a multiple of 16)."""
    out = (C.c_int64 * 4)()
    if lib.hispmv_prep_block_jacobi(int(n), int(block_size), out) != HISPMV_OK:
        raise ValueError("hispmv_prep_block_jacobi: 0 <= n < 2^31 and block_size 4, 8, 16 or 32")
    return dict(zip(("n_blocks", "pre_bytes", "flags_offset", "block_floats"), (int(x) for x in out)))


VALUE_LAYOUT_FIELDS = ("bytes", "map_slots", "chunks", "written", "format", "tile_kind", "parts", "batch_layouts")


def value_layouts_from_coo(coo_rows, coo_cols, coo_values, rows: int, cols: int, n_cus: int = 256, value_storage: str = "fp32") -> dict:
    """Every device layout of the handle a COO input makes, packed twice on the host (hispmv_prep_value_layouts): `real` with the
    values, `index` with the index payloads of a handle created with value updates on; `map` (int32, read out of `index`) and
    `chunks` ([n, 2] byte offsets of each chunk's first and second destination, -1 = none), plus the VALUE_LAYOUT_FIELDS counts.
    value_storage="bf16": the layouts of an updatable bf16 handle -- `real` packed from the rounded values with its half groups, `map`
    as the loader uploads it -- and `kinds` ([n, 2] int32 beside `chunks`: 0 = 1024 fp32 slots, 1 = a half slice)."""
    if value_storage not in VALUE_STORAGES:
        raise ValueError('value storage must be "fp32" or "bf16"')
    r = np.ascontiguousarray(coo_rows, dtype=np.int32)
    c = np.ascontiguousarray(coo_cols, dtype=np.int32)
    v = np.ascontiguousarray(coo_values, dtype=np.float32)
    p = C.c_void_p()
    cnt = (C.c_int64 * 8)()
    rc = lib.hispmv_prep_value_layouts_storage(C.byref(p), C.c_void_p(r.ctypes.data), C.c_void_p(c.ctypes.data), C.c_void_p(v.ctypes.data), r.size,
                                               int(rows), int(cols), int(n_cus), VALUE_STORAGES[value_storage], cnt)
    if rc != HISPMV_OK:
        raise ValueError(lib.hispmv_prep_last_error().decode())
    try:
        d = dict(zip(VALUE_LAYOUT_FIELDS, (int(x) for x in cnt)))

        def arr(which, n, dt):
            ptr = lib.hispmv_prep_value_array(p, which)
            return np.frombuffer((C.c_char * (n * np.dtype(dt).itemsize)).from_address(ptr), dtype=dt).copy() if (n and ptr) else np.zeros(0, dt)
        d.update(real=arr(0, d["bytes"], np.uint8), index=arr(1, d["bytes"], np.uint8), map=arr(2, d["map_slots"], np.int32),
                 chunks=arr(3, 2 * d["chunks"], np.int64).reshape(-1, 2), kinds=arr(4, 2 * d["chunks"], np.int32).reshape(-1, 2))
        return d
    finally:
        lib.hispmv_prep_free(p)
