"""``FpgaHandle`` -- host-side mirror of the reference's pybind11 class
(pyhispmv/include/fpga_handle.h:9-74, pyhispmv/src/fpga_handle.cpp, bindings
pyhispmv/src/pyhispmv_bindings.cpp:3-39) over the C ABI of libhispmv.so.

Same method names, keyword names, argument meaning and return values as the reference, so
apps/general_test.py and apps/model_test.py run against it unchanged.  Differences, all on
the error path: the reference prints and calls ``std::exit`` (fpga_handle.cpp:58-64,82-88,
267-270) or ``assert``s (:292); here the same conditions raise Python exceptions.
There is no CPU execution path: every method that computes needs the gfx950 device.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import lib


def _ptr(a: np.ndarray) -> C.c_void_p:
    return C.c_void_p(a.ctypes.data)


def _as(a, dtype) -> np.ndarray:
    # pybind11's py::array_t<T> default flags (c_style | forcecast): other dtypes / layouts are
    # converted by copy (e.g. torch int64 COO indices from apps/fpga_layer_manager.py:29-33).
    return np.ascontiguousarray(a, dtype=dtype)


class FpgaHandle:
    """y = alpha * A @ x + beta * bias on one MI355X; A sparse (COO in) or dense (row-major in)."""

    def __init__(self, xclbin_path: str, device_id: int, num_ch_A: int, num_ch_B: int, num_ch_C: int,
                 urams_per_pe: int, fp_acc_latency: int, dense_overlay: bool, pre_accumulator: bool,
                 row_dist_net: bool):
        self._ctx = C.c_void_p()
        rc = lib.hispmv_create(C.byref(self._ctx), str(xclbin_path).encode(), int(device_id),
                               int(num_ch_A), int(num_ch_B), int(num_ch_C), int(urams_per_pe),
                               int(fp_acc_latency), int(bool(dense_overlay)), int(bool(pre_accumulator)),
                               int(bool(row_dist_net)))
        if rc != _lib.HISPMV_OK:
            msg = lib.hispmv_last_error(None).decode()
            self._ctx = C.c_void_p()
            if rc == _lib.HISPMV_EINVAL:
                raise ValueError(f"Error initializing device: {msg}")
            raise RuntimeError(f"Error initializing device: {msg}")
        self.num_ch_A, self.num_ch_B, self.num_ch_C = num_ch_A, num_ch_B, num_ch_C
        self.device_id = device_id
        self._selected = None

    # -- lifetime -------------------------------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_ctx", None):
            lib.hispmv_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _err(self) -> str:
        return lib.hispmv_last_error(self._ctx).decode()

    def _check(self, rc: int) -> int:
        if rc >= 0:
            return rc
        msg = self._err()
        if rc == _lib.HISPMV_EINVAL:
            raise IndexError(msg) if "out of range" in msg else ValueError(msg)
        if rc == _lib.HISPMV_ESTATE:
            raise AssertionError(msg)
        if rc == _lib.HISPMV_ENOTDENSE:
            raise AssertionError(msg)
        if rc == _lib.HISPMV_EIO:
            raise OSError(msg)
        if rc == _lib.HISPMV_ENOMEM:
            raise MemoryError(msg)
        if rc == _lib.HISPMV_ENOTSUP:
            raise NotImplementedError(msg)
        raise RuntimeError(msg)

    # -- reference API (bindings :15-38) --------------------------------------------------------
    def create_dense_handle(self, flattened_dense_values, rows: int, cols: int) -> int:
        """Creates a matrix handle for a dense matrix; returns its index, or -1 if it does not fit."""
        a = _as(flattened_dense_values, np.float32).reshape(-1)
        if a.size < int(rows) * int(cols):
            raise ValueError("flattened_dense_values shorter than rows*cols")
        rc = lib.hispmv_create_dense_handle(self._ctx, _ptr(a), int(rows), int(cols))
        return rc if rc == _lib.HISPMV_FULL else self._check(rc)

    def create_sparse_handle(self, coo_rows, coo_cols, coo_values, rows: int, cols: int) -> int:
        """Creates a matrix handle for a sparse matrix (COO); returns its index, or -1 if it does not fit."""
        r = _as(coo_rows, np.int32).reshape(-1)
        c = _as(coo_cols, np.int32).reshape(-1)
        v = _as(coo_values, np.float32).reshape(-1)
        if not (r.size == c.size == v.size):
            raise ValueError("coo_rows, coo_cols and coo_values must have the same length")
        rc = lib.hispmv_create_sparse_handle(self._ctx, _ptr(r), _ptr(c), _ptr(v), r.size, int(rows), int(cols))
        return rc if rc == _lib.HISPMV_FULL else self._check(rc)

    def load_matrices(self) -> None:
        """Loads matrices into HBM (call after all create_* and before any run)."""
        self._check(lib.hispmv_load_matrices(self._ctx))

    def select_matrix(self, matrix_idx: int) -> None:
        """Select a matrix by its index."""
        if matrix_idx < 0:
            raise IndexError("Matrix idx out of range")
        self._check(lib.hispmv_select_matrix(self._ctx, int(matrix_idx)))
        self._selected = int(matrix_idx)

    def run_kernel(self, x, bias, y, alpha: float, beta: float) -> None:
        """Runs y = alpha*A*x + beta*bias for the selected matrix; y is written in place."""
        if not (isinstance(y, np.ndarray) and y.dtype == np.float32 and y.flags.c_contiguous and y.flags.writeable):
            raise TypeError("y must be a writable C-contiguous float32 numpy array (it is written in place)")
        xa = _as(x, np.float32).reshape(-1)
        ba = _as(bias, np.float32).reshape(-1)
        if self._selected is not None:   # the reference reads out of bounds instead
            info = self.matrix_info(self._selected)
            if xa.size < info["cols"] or y.size < info["rows"] or (beta != 0.0 and ba.size < info["rows"]):
                raise ValueError("vector shorter than the selected matrix dimension")
        self._check(lib.hispmv_run_kernel(self._ctx, _ptr(xa), _ptr(ba), _ptr(y), float(alpha), float(beta)))

    def linear(self, matrix_idx: int, x, bias) -> np.ndarray:
        """Run y = A*x + bias for each of the len(x)//cols vectors in the flattened x; returns a new array."""
        info = self.matrix_info(matrix_idx)
        xa = _as(x, np.float32).reshape(-1)
        ba = _as(bias, np.float32).reshape(-1)
        if ba.size < info["rows"]:
            raise ValueError("bias shorter than the matrix row dimension")
        num_vecs = xa.size // info["cols"]
        out = np.empty(num_vecs * info["rows"], dtype=np.float32)
        self._check(lib.hispmv_linear(self._ctx, int(matrix_idx), _ptr(xa), xa.size, _ptr(ba), _ptr(out)))
        return out

    # -- additions (no reference counterpart) ----------------------------------------------------
    def create_sparse_handle_from_mtx(self, path: str, flavor: int = 0) -> int:
        """MatrixMarket file -> handle (HiSpmvHandle::prepareSparseMtxForFPGA(mtx_file), spmv-helper.cpp:642)."""
        rc = lib.hispmv_create_sparse_handle_from_mtx(self._ctx, str(path).encode(), int(flavor))
        return rc if rc == _lib.HISPMV_FULL else self._check(rc)

    def create_sparse_handle_from_csr(self, row_ptr, col_idx, values, rows: int, cols: int) -> int:
        rp = _as(row_ptr, np.int32).reshape(-1)
        ci = _as(col_idx, np.int32).reshape(-1)
        va = _as(values, np.float32).reshape(-1)
        if rp.size != rows + 1 or ci.size != va.size or (rp.size and rp[-1] != ci.size):
            raise ValueError("inconsistent CSR arrays")
        rc = lib.hispmv_create_sparse_handle_from_csr(self._ctx, _ptr(rp), _ptr(ci), _ptr(va), int(rows), int(cols))
        return rc if rc == _lib.HISPMV_FULL else self._check(rc)

    def set_value_updates(self, enable) -> None:
        """Handles created from now on (until switched off) can have their values updated in place (hispmv_set_value_updates).
        True / False as ever: under True, creating a handle while the value storage is "bf16" raises ValueError.  "any_storage": fp32
        handles exactly as under True, and bf16 handles are created updatable too -- their updates take fp32 values and round them on
        the device to the nearest bfloat16 (ties to even).  Any other string raises ValueError."""
        if isinstance(enable, str):
            if enable != "any_storage":
                raise ValueError('set_value_updates takes False, True or "any_storage"')
            state = _lib.HISPMV_VALUE_UPDATES_ANY_STORAGE
        else:
            state = int(bool(enable))
        self._check(lib.hispmv_set_value_updates(self._ctx, state))

    def update_values(self, matrix_idx: int, values) -> None:
        """New values for a loaded updatable handle, in the order of its creation input (COO arrays, CSR values before the per-row
        sort, W row-major); returns when the device holds them."""
        v = _as(values, np.float32).reshape(-1)
        self._check(lib.hispmv_update_values(self._ctx, int(matrix_idx), _ptr(v), v.size))

    def update_values_device(self, matrix_idx: int, d_values: int, n: int, stream: int = 0) -> None:
        """The same from device memory (an int pointer, e.g. a torch tensor's ``data_ptr()``): asynchronous and ordered on `stream`
        (0 = the context's stream); ordering against other streams is the caller's job."""
        self._check(lib.hispmv_update_values_device(self._ctx, int(matrix_idx), C.c_void_p(d_values), int(n), C.c_void_p(stream)))

    def value_update_info(self, matrix_idx: int) -> dict:
        """{"updatable", "n", "map_slots", "written"} of a handle (hispmv_value_update_info)."""
        out = (C.c_int64 * 4)()
        rc = lib.hispmv_value_update_info(self._ctx, int(matrix_idx), out)
        if rc != _lib.HISPMV_OK:
            raise IndexError("Matrix idx out of range")
        return {"updatable": bool(out[0]), "n": int(out[1]), "map_slots": int(out[2]), "written": int(out[3])}

    def set_value_storage(self, storage: str) -> None:
        """"fp32" (default) or "bf16": how handles created from now on store their values (hispmv_set_value_storage).  A bf16 handle
        rounds its values once, at creation, and computes with fp32 x, products and sums; compact slice groups and dense W shrink."""
        if storage not in _lib.VALUE_STORAGES:
            raise ValueError('value storage must be "fp32" or "bf16"')
        self._check(lib.hispmv_set_value_storage(self._ctx, _lib.VALUE_STORAGES[storage]))

    def value_storage_info(self, matrix_idx: int) -> dict:
        """{"storage", "slots_2byte", "slots_4byte", "saved_bytes"} of a handle (hispmv_value_storage_info)."""
        out = (C.c_int64 * 4)()
        rc = lib.hispmv_value_storage_info(self._ctx, int(matrix_idx), out)
        if rc != _lib.HISPMV_OK:
            raise IndexError("Matrix idx out of range")
        return {"storage": "bf16" if out[0] == _lib.HISPMV_VALUES_BF16 else "fp32", "slots_2byte": int(out[1]), "slots_4byte": int(out[2]),
                "saved_bytes": int(out[3])}

    @staticmethod
    def transposable_state(enable) -> int:
        """The integer state of hispmv_set_transposable that `enable` spells: False / True / 0, 1, 2 as they are, "keep_format" = 2,
        "companion" = 3.  The stored transpose costs arena bytes, so it is asked for by name only: the bare integer 3 raises
        ValueError, as it did before the state existed, and so does any other string.  (Other integers are the library's to judge.)"""
        if isinstance(enable, str):
            states = {"keep_format": _lib.HISPMV_TRANSPOSABLE_KEEP_FORMAT, "companion": _lib.HISPMV_TRANSPOSABLE_COMPANION}
            if enable not in states:
                raise ValueError('set_transposable takes False, True, "keep_format", "companion" or 0, 1, 2')
            return states[enable]
        if int(enable) == _lib.HISPMV_TRANSPOSABLE_COMPANION:
            raise ValueError('set_transposable: the stored transpose is asked for by name, set_transposable("companion"), not by the integer 3')
        return int(enable)

    def set_transposable(self, enable) -> None:
        """The state sparse handles are created under from now on (hispmv_set_transposable): False / 0 = off; True / 1 = they keep the
        slice stream, so that spmv_device_t, linear_device_t and value_grad_device accept them; "keep_format" / 2 = they keep the
        format the loader picks, and a tile stream among them (one part, the standard or the small geometry) is accepted by the same
        three entries through the tile-stream kernels; "companion" (by name only) = as "keep_format", and the handle also owns a stored transpose
        (companion_info): spmv_device_t and linear_device_t then run the forward kernels over it, without atomics, for the price of
        its device bytes and creation time.  Anything else raises ValueError."""
        self._check(lib.hispmv_set_transposable(self._ctx, self.transposable_state(enable)))

    def companion_info(self, matrix_idx: int) -> dict:
        """{"has", "format", "parts", "device_bytes", "map_slots", "tile_kind"} of the stored transpose of a handle
        (hispmv_companion_info); has is False and the rest zero for a handle without one."""
        out = (C.c_int64 * 6)()
        rc = lib.hispmv_companion_info(self._ctx, int(matrix_idx), out)
        if rc != _lib.HISPMV_OK:
            raise IndexError("Matrix idx out of range")
        return {"has": bool(out[0]), "format": int(out[1]), "parts": int(out[2]), "device_bytes": int(out[3]), "map_slots": int(out[4]),
                "tile_kind": int(out[5])}

    def spmv_device_t(self, matrix_idx: int, d_x: int, d_bias: int, d_y: int, alpha: float, beta: float,
                      stream: int = 0) -> None:
        """y[cols] = alpha * A^T x[rows] + beta * bias[cols] on device pointers (ints), asynchronous on `stream` (hispmv_spmv_device_t).
        Two contracts.  Without a stored transpose the sums arrive through float atomics: the last bits may differ from run to run, a
        +-0 slot adds nothing, and d_y must be ordinary device memory (not fine-grained or host-pinned); a tile-stream handle raises
        NotImplementedError unless it was created under set_transposable("keep_format").  A handle created under
        set_transposable("companion") runs the forward kernels over its stored transpose: plain stores into any device-writable d_y,
        and the bits of a one-vector linear_device call on a handle made from the swapped COO -- the same from run to run, zero slots
        and non-finite inputs as in that forward product; one transposed call per handle in flight."""
        self._check(lib.hispmv_spmv_device_t(self._ctx, int(matrix_idx), C.c_void_p(d_x), C.c_void_p(d_bias),
                                             C.c_void_p(d_y), float(alpha), float(beta), C.c_void_p(stream)))

    def transpose_info(self, matrix_idx: int) -> dict:
        """{"transposable", "launches", "atomic_bytes", "direct_elems"} of a handle (hispmv_transpose_info)."""
        out = (C.c_int64 * 4)()
        rc = lib.hispmv_transpose_info(self._ctx, int(matrix_idx), out)
        if rc != _lib.HISPMV_OK:
            raise IndexError("Matrix idx out of range")
        return {"transposable": bool(out[0]), "launches": int(out[1]), "atomic_bytes": int(out[2]), "direct_elems": int(out[3])}

    def linear_device(self, matrix_idx: int, d_x: int, num_vecs: int, d_bias: int, d_y: int, alpha: float = 1.0, beta: float = 1.0,
                      stream: int = 0) -> None:
        """y[v] = alpha * A x[v] + beta * bias for num_vecs vectors on device pointers (ints): x is [num_vecs, cols], y [num_vecs, rows],
        row-major and contiguous, one bias for all (hispmv_linear_device).  Asynchronous on `stream`.  With alpha = beta = 1 the bits of
        `linear`.  One call per handle in flight: carries and partial vectors belong to the handle."""
        self._check(lib.hispmv_linear_device(self._ctx, int(matrix_idx), C.c_void_p(d_x), int(num_vecs), C.c_void_p(d_bias), C.c_void_p(d_y),
                                             float(alpha), float(beta), C.c_void_p(stream)))

    def linear_device_t(self, matrix_idx: int, d_x: int, num_vecs: int, d_bias: int, d_y: int, alpha: float, beta: float,
                        bias_stride: int = 0, stream: int = 0) -> None:
        """y[v] = alpha * A^T x[v] + beta * bias[v * bias_stride] for num_vecs vectors on device pointers (ints): x is [num_vecs, rows],
        y [num_vecs, cols] (hispmv_linear_device_t).  bias_stride 0 = one bias for all, cols = one per vector (then d_bias may be d_y:
        in place).  The promises and preconditions of spmv_device_t and the handles it accepts, under both of its contracts: atomics in
        no fixed order without a stored transpose; with one (set_transposable("companion")) every vector has the bits of a one-vector
        linear_device call on a handle made from the swapped COO, whatever num_vecs, and the vectors go in the passes linear_device
        takes there (a per-vector bias on a tile-stream companion: one vector per launch)."""
        self._check(lib.hispmv_linear_device_t(self._ctx, int(matrix_idx), C.c_void_p(d_x), int(num_vecs), C.c_void_p(d_bias), int(bias_stride),
                                               C.c_void_p(d_y), float(alpha), float(beta), C.c_void_p(stream)))

    def linear_info(self, matrix_idx: int, num_vecs: int) -> dict:
        """{"width", "passes"} of linear_device (beta != 0) and {"width_t", "passes_t", "launches_t"} of linear_device_t for num_vecs
        vectors on a handle (hispmv_linear_info): the vectors of the widest pass over the matrix, the passes, the launches."""
        out = (C.c_int64 * 5)()
        rc = lib.hispmv_linear_info(self._ctx, int(matrix_idx), int(num_vecs), out)
        if rc != _lib.HISPMV_OK:
            raise IndexError("Matrix idx out of range") if num_vecs >= 1 else ValueError("num_vecs must be at least 1")
        return {"width": int(out[0]), "passes": int(out[1]), "width_t": int(out[2]), "passes_t": int(out[3]), "launches_t": int(out[4])}

    def value_grad_device(self, matrix_idx: int, d_gy: int, d_x: int, num_vecs: int, d_grad: int, alpha: float = 1.0, beta: float = 0.0,
                          stream: int = 0) -> None:
        """grad[k] = alpha * sum_v gy[v, row_k] * x[v, col_k] + beta * grad[k] for every entry k of the creation input of a loaded,
        updatable handle, on device pointers (ints): gy is [num_vecs, rows], x [num_vecs, cols], grad holds value_update_info()["n"]
        floats in the order update_values_device reads (hispmv_value_grad_device).  Asynchronous on `stream`.  Plain stores, one writer
        per entry: the same bits run to run.  beta == 0 does not read grad.  A handle created with value updates off raises
        AssertionError, a tile-stream handle that was not created under set_transposable("keep_format") NotImplementedError."""
        self._check(lib.hispmv_value_grad_device(self._ctx, int(matrix_idx), C.c_void_p(d_gy), C.c_void_p(d_x), int(num_vecs), C.c_void_p(d_grad),
                                                 float(alpha), float(beta), C.c_void_p(stream)))

    def value_grad_info(self, matrix_idx: int, num_vecs: int) -> dict:
        """{"accepted", "width", "passes", "launches"} of value_grad_device for num_vecs vectors on a handle (hispmv_value_grad_info):
        the vectors of the widest pass, the passes, the launches of a call with alpha != 0; zeros for a handle it does not accept."""
        out = (C.c_int64 * 4)()
        rc = lib.hispmv_value_grad_info(self._ctx, int(matrix_idx), int(num_vecs), out)
        if rc != _lib.HISPMV_OK:
            raise IndexError("Matrix idx out of range") if num_vecs >= 1 else ValueError("num_vecs must be at least 1")
        return {"accepted": bool(out[0]), "width": int(out[1]), "passes": int(out[2]), "launches": int(out[3])}

    def spmm_device(self, matrix_idx: int, d_xt: int, num_vecs: int, d_bias: int, d_yt: int, alpha: float = 1.0, beta: float = 0.0,
                    ld_x=None, ld_y=None, bias_stride: int = 0, work: int = 0, work_bytes: int = 0, stream: int = 0) -> None:
        """yt[r, v] = alpha * sum_k a_rk * xt[k, v] + beta * bias for num_vecs vectors on device pointers (ints), operands FEATURE-MAJOR:
        xt is [cols, ld_x], yt [rows, ld_y], row-major, ld (default num_vecs) >= num_vecs (hispmv_spmm_device).  The lanes of a wavefront
        are vectors and the matrix is read once per tile of up to 256 vectors, not once per 4 as in linear_device.  bias_stride 0: d_bias
        is bias[rows]; ld_y: a matrix laid out like yt, which may be yt (in place).  `work` points at work_bytes >=
        spmm_info(...)["work_bytes"] bytes of the caller's; nothing is kept in the handle, so calls with different workspaces may overlap.
        No atomics: the bits of a vector depend neither on the batch nor on the run (they are not linear_device's bits).  Asynchronous on
        `stream`.  Slice-stream handles only: a tile-stream or dense handle raises NotImplementedError."""
        self._check(lib.hispmv_spmm_device(self._ctx, int(matrix_idx), C.c_void_p(d_xt), int(num_vecs), int(num_vecs if ld_x is None else ld_x),
                                           C.c_void_p(d_bias), int(bias_stride), C.c_void_p(d_yt), int(num_vecs if ld_y is None else ld_y),
                                           float(alpha), float(beta), C.c_void_p(work), int(work_bytes), C.c_void_p(stream)))

    def spmm_device_t(self, matrix_idx: int, d_xt: int, num_vecs: int, d_bias: int, d_yt: int, alpha: float = 1.0, beta: float = 0.0,
                      ld_x=None, ld_y=None, bias_stride: int = 0, work: int = 0, work_bytes: int = 0, stream: int = 0) -> None:
        """spmm_device with A^T: xt is [rows, ld_x], yt [cols, ld_y] (hispmv_spmm_device_t); work_bytes >= spmm_info(...)["work_bytes_t"].
        Runs the same launches over the handle's stored transpose: only a handle created under set_transposable("companion") whose
        companion is a slice stream is accepted, any other raises NotImplementedError.  Per vector the bits of spmm_device on a handle
        made from the swapped COO."""
        self._check(lib.hispmv_spmm_device_t(self._ctx, int(matrix_idx), C.c_void_p(d_xt), int(num_vecs), int(num_vecs if ld_x is None else ld_x),
                                             C.c_void_p(d_bias), int(bias_stride), C.c_void_p(d_yt), int(num_vecs if ld_y is None else ld_y),
                                             float(alpha), float(beta), C.c_void_p(work), int(work_bytes), C.c_void_p(stream)))

    def spmm_info(self, matrix_idx: int, num_vecs: int, ld=None) -> dict:
        """{"accepted", "accepted_t", "vl", "tiles", "launches", "work_bytes", "work_bytes_t"} of spmm_device / spmm_device_t for num_vecs
        vectors with ld_x = ld_y = ld (default num_vecs) and 16-byte aligned pointers (hispmv_spmm_info): the vectors per lane of the
        first tile, the vector tiles, the launches of a call with alpha != 0, the workspace bytes (valid for every alignment)."""
        out = (C.c_int64 * 8)()
        rc = lib.hispmv_spmm_info(self._ctx, int(matrix_idx), int(num_vecs), int(num_vecs if ld is None else ld), out)
        if rc != _lib.HISPMV_OK:
            if 0 <= int(matrix_idx) < self.num_matrices():
                raise ValueError("num_vecs must be at least 1 and ld at least num_vecs")
            raise IndexError("Matrix idx out of range")
        return {"accepted": bool(out[0]), "accepted_t": bool(out[1]), "vl": int(out[2]), "tiles": int(out[3]), "launches": int(out[4]),
                "work_bytes": int(out[5]), "work_bytes_t": int(out[6])}

    def spmm_device_bf16(self, matrix_idx: int, d_xt: int, num_vecs: int, d_bias: int, d_yt: int, alpha: float = 1.0, beta: float = 0.0,
                         ld_x=None, ld_y=None, bias_stride: int = 0, work: int = 0, work_bytes: int = 0, stream: int = 0) -> None:
        """spmm_device with bf16 activations (hispmv_spmm_device_bf16): xt [cols, ld_x] and yt [rows, ld_y] hold bfloat16, ld in elements.
        bias_stride 0: d_bias is an FP32 bias[rows]; ld_y: a BF16 matrix laid out like yt, which may be yt (in place).  Products and
        sums are fp32 in the order of spmm_device; the finished value -- bit for bit what spmm_device stores for the widened operands --
        is rounded once to bf16 (nearest, ties to even).  A lane owns up to 8 vectors, a tile is up to 512.  work_bytes >=
        spmm_bf16_info(...)["work_bytes"].  Same handles, same exceptions as spmm_device."""
        self._check(lib.hispmv_spmm_device_bf16(self._ctx, int(matrix_idx), C.c_void_p(d_xt), int(num_vecs), int(num_vecs if ld_x is None else ld_x),
                                                C.c_void_p(d_bias), int(bias_stride), C.c_void_p(d_yt), int(num_vecs if ld_y is None else ld_y),
                                                float(alpha), float(beta), C.c_void_p(work), int(work_bytes), C.c_void_p(stream)))

    def spmm_device_t_bf16(self, matrix_idx: int, d_xt: int, num_vecs: int, d_bias: int, d_yt: int, alpha: float = 1.0, beta: float = 0.0,
                           ld_x=None, ld_y=None, bias_stride: int = 0, work: int = 0, work_bytes: int = 0, stream: int = 0) -> None:
        """spmm_device_bf16 with A^T: xt is [rows, ld_x], yt [cols, ld_y], bfloat16 (hispmv_spmm_device_t_bf16); work_bytes >=
        spmm_bf16_info(...)["work_bytes_t"].  Same handles, same exceptions as spmm_device_t."""
        self._check(lib.hispmv_spmm_device_t_bf16(self._ctx, int(matrix_idx), C.c_void_p(d_xt), int(num_vecs), int(num_vecs if ld_x is None else ld_x),
                                                  C.c_void_p(d_bias), int(bias_stride), C.c_void_p(d_yt), int(num_vecs if ld_y is None else ld_y),
                                                  float(alpha), float(beta), C.c_void_p(work), int(work_bytes), C.c_void_p(stream)))

    def spmm_bf16_info(self, matrix_idx: int, num_vecs: int, ld=None) -> dict:
        """{"accepted", "accepted_t", "vb", "tiles", "launches", "work_bytes", "work_bytes_t"} of spmm_device_bf16 / spmm_device_t_bf16 for
        num_vecs vectors with ld_x = ld_y = ld (default num_vecs) and 16-byte aligned pointers (hispmv_spmm_bf16_info): the bf16 per lane
        of the first tile, the vector tiles, the launches of a call with alpha != 0, the workspace bytes (valid for every alignment)."""
        out = (C.c_int64 * 8)()
        rc = lib.hispmv_spmm_bf16_info(self._ctx, int(matrix_idx), int(num_vecs), int(num_vecs if ld is None else ld), out)
        if rc != _lib.HISPMV_OK:
            if 0 <= int(matrix_idx) < self.num_matrices():
                raise ValueError("num_vecs must be at least 1 and ld at least num_vecs")
            raise IndexError("Matrix idx out of range")
        return {"accepted": bool(out[0]), "accepted_t": bool(out[1]), "vb": int(out[2]), "tiles": int(out[3]), "launches": int(out[4]),
                "work_bytes": int(out[5]), "work_bytes_t": int(out[6])}

    def spmm_value_grad_device(self, matrix_idx: int, d_gyt: int, d_xt: int, num_vecs: int, d_grad: int, alpha: float = 1.0, beta: float = 0.0,
                               ld_gy=None, ld_x=None, stream: int = 0) -> None:
        """grad[k] = alpha * sum_v gyt[row_k, v] * xt[col_k, v] + beta * grad[k] for every entry k of the creation input of a loaded,
        updatable slice-stream handle, on device pointers (ints), operands FEATURE-MAJOR as in spmm_device: gyt is [rows, ld_gy], xt
        [cols, ld_x], row-major, ld (default num_vecs) >= num_vecs; the pad floats of a row are never used (hispmv_spmm_value_grad_device).
        The lanes of a wavefront are vectors and the slice stream (its metas only) is read once per tile of up to 256 vectors, not once
        per 4 as in value_grad_device.  No workspace, no atomics, nothing kept in the handle; plain stores, one writer per entry: the
        same bits run to run.  The bits depend on (num_vecs, ld, alignment) through the lane width and the tiles: they are not the bits
        of value_grad_device and not independent of the batch.  beta == 0 does not read grad.  Asynchronous on `stream`.  A tile-stream
        or dense handle raises NotImplementedError, a handle created with value updates off AssertionError, a bad argument ValueError."""
        self._check(lib.hispmv_spmm_value_grad_device(self._ctx, int(matrix_idx), C.c_void_p(d_gyt), int(num_vecs if ld_gy is None else ld_gy),
                                                      C.c_void_p(d_xt), int(num_vecs if ld_x is None else ld_x), int(num_vecs), C.c_void_p(d_grad),
                                                      float(alpha), float(beta), C.c_void_p(stream)))

    def spmm_value_grad_info(self, matrix_idx: int, num_vecs: int, ld=None) -> dict:
        """{"accepted", "vl", "tiles", "launches"} of spmm_value_grad_device for num_vecs vectors with ld_gy = ld_x = ld (default num_vecs)
        and 16-byte aligned pointers (hispmv_spmm_value_grad_info): the vectors per lane of the first tile, the vector tiles, the launches
        of a call with alpha != 0 (one per tile and part that holds slices); zeros for a handle it does not accept."""
        out = (C.c_int64 * 4)()
        rc = lib.hispmv_spmm_value_grad_info(self._ctx, int(matrix_idx), int(num_vecs), int(num_vecs if ld is None else ld), out)
        if rc != _lib.HISPMV_OK:
            if 0 <= int(matrix_idx) < self.num_matrices():
                raise ValueError("num_vecs must be at least 1 and ld at least num_vecs")
            raise IndexError("Matrix idx out of range")
        return {"accepted": bool(out[0]), "vl": int(out[1]), "tiles": int(out[2]), "launches": int(out[3])}

    def spmm_value_grad_device_bf16(self, matrix_idx: int, d_gyt: int, d_xt: int, num_vecs: int, d_grad: int, alpha: float = 1.0, beta: float = 0.0,
                                    ld_gy=None, ld_x=None, stream: int = 0) -> None:
        """spmm_value_grad_device with bfloat16 gyt [rows, ld_gy] and xt [cols, ld_x] (hispmv_spmm_value_grad_device_bf16); grad, alpha and
        beta stay float32.  A lane owns 8, 4, 2 or 1 vectors (prep.spmm_bf16_tiles with the smaller alignment of the two operands), a
        tile is up to 512 vectors.  Widening is exact and the order of the sum is that of spmm_value_grad_device: where both take the
        same lane width and tiles, the bits are those of spmm_value_grad_device on the widened operands.  Operands 2-byte aligned, grad
        4-byte.  Same handles, same exceptions as spmm_value_grad_device."""
        self._check(lib.hispmv_spmm_value_grad_device_bf16(self._ctx, int(matrix_idx), C.c_void_p(d_gyt), int(num_vecs if ld_gy is None else ld_gy),
                                                           C.c_void_p(d_xt), int(num_vecs if ld_x is None else ld_x), int(num_vecs), C.c_void_p(d_grad),
                                                           float(alpha), float(beta), C.c_void_p(stream)))

    def spmm_value_grad_bf16_info(self, matrix_idx: int, num_vecs: int, ld=None) -> dict:
        """{"accepted", "vb", "tiles", "launches"} of spmm_value_grad_device_bf16 for num_vecs vectors with ld_gy = ld_x = ld (default
        num_vecs) and 16-byte aligned pointers (hispmv_spmm_value_grad_bf16_info): the bf16 per lane of the first tile, the vector tiles,
        the launches of a call with alpha != 0 (one per tile and part that holds slices); zeros for a handle it does not accept."""
        out = (C.c_int64 * 4)()
        rc = lib.hispmv_spmm_value_grad_bf16_info(self._ctx, int(matrix_idx), int(num_vecs), int(num_vecs if ld is None else ld), out)
        if rc != _lib.HISPMV_OK:
            if 0 <= int(matrix_idx) < self.num_matrices():
                raise ValueError("num_vecs must be at least 1 and ld at least num_vecs")
            raise IndexError("Matrix idx out of range")
        return {"accepted": bool(out[0]), "vb": int(out[1]), "tiles": int(out[2]), "launches": int(out[3])}

    # -- Krylov solvers (hispmv_krylov_abi.cpp; hispmv_amd.solvers wraps these for torch tensors) -----------------------------------
    def krylov_info(self, matrix_idx: int, solver: str) -> dict:
        """{"accepted", "work_bytes", "launches_per_iteration", "products_per_iteration", "products_t_per_iteration", "r_offset",
        "x_len", "b_len"} of `solver` ("cg", "bicgstab", "cgls") on a handle (hispmv_krylov_info): the workspace a solve needs, the
        vector kernels and the products of one iteration, where the workspace keeps the residual; zeros for a handle it refuses."""
        if solver not in _lib.KRYLOV_SOLVERS:
            raise ValueError('solver must be "cg", "bicgstab" or "cgls"')
        out = (C.c_int64 * 8)()
        rc = lib.hispmv_krylov_info(self._ctx, int(matrix_idx), _lib.KRYLOV_SOLVERS[solver], out)
        if rc != _lib.HISPMV_OK:
            raise IndexError("Matrix idx out of range")
        return {"accepted": bool(out[0]), "work_bytes": int(out[1]), "launches_per_iteration": int(out[2]), "products_per_iteration": int(out[3]),
                "products_t_per_iteration": int(out[4]), "r_offset": int(out[5]), "x_len": int(out[6]), "b_len": int(out[7])}

    @staticmethod
    def _krylov_result(res) -> dict:
        return {"status": _lib.KRYLOV_STATUS[res.status], "iterations": int(res.iterations), "relres": float(res.relres), "products": int(res.products)}

    def dot_device(self, n: int, d_a: int, d_b: int, d_out: int, work: int, work_bytes: int, stream: int = 0) -> None:
        """*d_out (a float64 in device memory) = sum a[i] * b[i] of two float32 device vectors, exact products summed in fp64 in an order
        that depends on n alone (hispmv_dot_device; include/hispmv.h writes the order down).  Asynchronous on `stream`.  `work` points
        at work_bytes >= 8 * prep.krylov_groups(n) bytes, 16-byte aligned; a and b need 4-byte alignment only."""
        self._check(lib.hispmv_dot_device(self._ctx, int(n), C.c_void_p(d_a), C.c_void_p(d_b), C.c_void_p(d_out), C.c_void_p(work), int(work_bytes),
                                          C.c_void_p(stream)))

    def cg_device(self, matrix_idx: int, d_b: int, d_x: int, d_minv: int = 0, rtol: float = 1e-6, max_iters: int = 1000, check_every: int = 8,
                  work: int = 0, work_bytes: int = 0, stream: int = 0) -> dict:
        """Preconditioned CG on device pointers (hispmv_cg_device): d_x holds the initial guess and then the solution, d_minv is 0 or
        the inverse diagonal.  Returns {"status", "iterations", "relres", "products"}; with check_every = 0 the call returns at once
        with status "IN_FLIGHT" and krylov_status reads the outcome.  A handle that is not square, a bad rtol / max_iters /
        check_every or a short, missing or misaligned workspace raises ValueError, a call before load_matrices AssertionError."""
        res = _lib.KrylovResult()
        self._check(lib.hispmv_cg_device(self._ctx, int(matrix_idx), C.c_void_p(d_b), C.c_void_p(d_x), C.c_void_p(d_minv), float(rtol), int(max_iters),
                                         int(check_every), C.c_void_p(work), int(work_bytes), C.c_void_p(stream), C.byref(res)))
        return self._krylov_result(res)

    def bicgstab_device(self, matrix_idx: int, d_b: int, d_x: int, rtol: float = 1e-6, max_iters: int = 1000, check_every: int = 8,
                        work: int = 0, work_bytes: int = 0, stream: int = 0) -> dict:
        """BiCGSTAB for a square handle, forward products only (hispmv_bicgstab_device); arguments, result and exceptions as cg_device."""
        res = _lib.KrylovResult()
        self._check(lib.hispmv_bicgstab_device(self._ctx, int(matrix_idx), C.c_void_p(d_b), C.c_void_p(d_x), float(rtol), int(max_iters),
                                               int(check_every), C.c_void_p(work), int(work_bytes), C.c_void_p(stream), C.byref(res)))
        return self._krylov_result(res)

    def cgls_device(self, matrix_idx: int, d_b: int, d_x: int, rtol: float = 1e-6, max_iters: int = 1000, check_every: int = 8,
                    work: int = 0, work_bytes: int = 0, stream: int = 0) -> dict:
        """CGLS, min ||b - A x|| for any shape, one forward and one transposed product per iteration (hispmv_cgls_device).  A handle
        spmv_device_t refuses raises its NotImplementedError before anything is launched; otherwise as cg_device."""
        res = _lib.KrylovResult()
        self._check(lib.hispmv_cgls_device(self._ctx, int(matrix_idx), C.c_void_p(d_b), C.c_void_p(d_x), float(rtol), int(max_iters),
                                           int(check_every), C.c_void_p(work), int(work_bytes), C.c_void_p(stream), C.byref(res)))
        return self._krylov_result(res)

    def krylov_status(self, work: int, stream: int = 0) -> dict:
        """Waits for `stream` and reads the outcome of the check_every = 0 solve that ran on it with workspace `work` (hispmv_krylov_status)."""
        res = _lib.KrylovResult()
        self._check(lib.hispmv_krylov_status(self._ctx, C.c_void_p(work), C.c_void_p(stream), C.byref(res)))
        return self._krylov_result(res)

    # -- several right-hand sides (hispmv_krylov_multi_abi.cpp; hispmv_amd.solvers.cg_multi / bicgstab_multi wrap these) ------------
    def krylov_multi_info(self, matrix_idx: int, solver: str, num_vecs: int) -> dict:
        """{"accepted", "work_bytes", "launches_per_iteration", "products_per_iteration", "ld", "r_offset", "n", "groups"} of `solver` ("cg",
        "bicgstab") for num_vecs right-hand sides on a handle (hispmv_krylov_multi_info): the workspace, the vector kernels and the
        spmm_device calls of one iteration, the leading dimension of the workspace's vectors and where R lies; zeros for a handle the
        entries refuse."""
        if solver not in ("cg", "bicgstab"):
            raise ValueError('solver must be "cg" or "bicgstab"')
        out = (C.c_int64 * 8)()
        rc = lib.hispmv_krylov_multi_info(self._ctx, int(matrix_idx), _lib.KRYLOV_SOLVERS[solver], int(num_vecs), out)
        if rc != _lib.HISPMV_OK:
            if 0 <= int(matrix_idx) < self.num_matrices():
                raise ValueError("num_vecs must be at least 1 (and at most 2^20)")
            raise IndexError("Matrix idx out of range")
        return {"accepted": bool(out[0]), "work_bytes": int(out[1]), "launches_per_iteration": int(out[2]), "products_per_iteration": int(out[3]),
                "ld": int(out[4]), "r_offset": int(out[5]), "n": int(out[6]), "groups": int(out[7])}

    def dot_multi_device(self, n: int, num_vecs: int, d_a: int, d_b: int, d_out: int, work: int, work_bytes: int, ld_a=None, ld_b=None,
                         stream: int = 0) -> None:
        """d_out[v] (float64, device) = sum_i a[i, v] * b[i, v] for the num_vecs columns of two feature-major float32 operands [n, ld]
        (hispmv_dot_multi_device): every column in the order of dot_device for n.  `work` points at work_bytes >= 8 * groups * ld of
        prep.krylov_multi(n, num_vecs), 16-byte aligned; n <= 2^20."""
        self._check(lib.hispmv_dot_multi_device(self._ctx, int(n), int(num_vecs), C.c_void_p(d_a), int(num_vecs if ld_a is None else ld_a), C.c_void_p(d_b),
                                                int(num_vecs if ld_b is None else ld_b), C.c_void_p(d_out), C.c_void_p(work), int(work_bytes), C.c_void_p(stream)))

    def cg_multi_device(self, matrix_idx: int, d_b: int, d_x: int, num_vecs: int, d_minv: int = 0, ld_b=None, ld_x=None, rtol: float = 1e-6,
                        max_iters: int = 1000, check_every: int = 8, work: int = 0, work_bytes: int = 0, stream: int = 0) -> list:
        """num_vecs independent preconditioned CG solves that share their launches (hispmv_cg_multi_device): d_b is [n, ld_b], d_x
        [n, ld_x] (initial guesses, then the solutions), d_minv 0 or ONE inverse diagonal for all columns.  Column v is bit for bit
        cg_device's arithmetic over spmm_device's products, with its own stopping and breakdown.  Returns the list of the columns'
        {"status", "iterations", "relres", "products"}; check_every = 0 returns at once with every status "IN_FLIGHT" and
        krylov_multi_status reads the outcome.  Exceptions as cg_device; a tile-stream or dense handle raises spmm_device's
        NotImplementedError."""
        res = (_lib.KrylovResult * int(max(num_vecs, 1)))()
        self._check(lib.hispmv_cg_multi_device(self._ctx, int(matrix_idx), C.c_void_p(d_b), int(num_vecs if ld_b is None else ld_b), C.c_void_p(d_x),
                                               int(num_vecs if ld_x is None else ld_x), int(num_vecs), C.c_void_p(d_minv), float(rtol), int(max_iters),
                                               int(check_every), C.c_void_p(work), int(work_bytes), C.c_void_p(stream), res))
        return [self._krylov_result(r) for r in res]

    def bicgstab_multi_device(self, matrix_idx: int, d_b: int, d_x: int, num_vecs: int, ld_b=None, ld_x=None, rtol: float = 1e-6,
                              max_iters: int = 1000, check_every: int = 8, work: int = 0, work_bytes: int = 0, stream: int = 0) -> list:
        """num_vecs independent BiCGSTAB solves that share their launches (hispmv_bicgstab_multi_device); arguments, result and
        exceptions as cg_multi_device."""
        res = (_lib.KrylovResult * int(max(num_vecs, 1)))()
        self._check(lib.hispmv_bicgstab_multi_device(self._ctx, int(matrix_idx), C.c_void_p(d_b), int(num_vecs if ld_b is None else ld_b), C.c_void_p(d_x),
                                                     int(num_vecs if ld_x is None else ld_x), int(num_vecs), float(rtol), int(max_iters),
                                                     int(check_every), C.c_void_p(work), int(work_bytes), C.c_void_p(stream), res))
        return [self._krylov_result(r) for r in res]

    def krylov_multi_status(self, work: int, num_vecs: int, stream: int = 0) -> list:
        """Waits for `stream` and reads the columns' outcomes of the check_every = 0 multi solve that ran on it with workspace `work`
        (hispmv_krylov_multi_status)."""
        res = (_lib.KrylovResult * int(max(num_vecs, 1)))()
        self._check(lib.hispmv_krylov_multi_status(self._ctx, C.c_void_p(work), int(num_vecs), C.c_void_p(stream), res))
        return [self._krylov_result(r) for r in res]

    # -- restarted GMRES (hispmv_gmres_abi.cpp; hispmv_amd.solvers.gmres wraps these) --------------------------------------------------
    def gmres_info(self, matrix_idx: int, restart: int = 30, with_minv: bool = False) -> dict:
        """{"accepted", "work_bytes", "launches_per_iteration", "launches_per_cycle", "products_per_iteration", "v_offset", "stride",
        "n"} of GMRES(restart) on a handle (hispmv_gmres_info): the workspace, the vector kernels of an inner iteration and of a cycle
        besides, where the workspace keeps the basis and how many floats lie between two basis vectors; zeros for a handle that is not
        loaded or not square."""
        out = (C.c_int64 * 8)()
        rc = lib.hispmv_gmres_info(self._ctx, int(matrix_idx), int(restart), int(bool(with_minv)), out)
        if rc != _lib.HISPMV_OK:
            if 0 <= int(matrix_idx) < self.num_matrices():
                raise ValueError(f"restart must be 1 .. {_lib.HISPMV_GMRES_MAX_RESTART}")
            raise IndexError("Matrix idx out of range")
        return {"accepted": bool(out[0]), "work_bytes": int(out[1]), "launches_per_iteration": int(out[2]), "launches_per_cycle": int(out[3]),
                "products_per_iteration": int(out[4]), "v_offset": int(out[5]), "stride": int(out[6]), "n": int(out[7])}

    def dot_basis_device(self, n: int, k: int, d_V: int, d_w: int, d_out: int, work: int, work_bytes: int, ld_v=None, stream: int = 0) -> None:
        """d_out[i] (float64, device) = (V_i, w) for the k <= 65 float32 vectors V_i = d_V + i * ld_v (default ld_v = n) and w, each
        value bit for bit dot_device's (hispmv_dot_basis_device).  `work` points at work_bytes >= 8 * k * prep.krylov_groups(n) bytes,
        16-byte aligned.  Asynchronous on `stream`."""
        self._check(lib.hispmv_dot_basis_device(self._ctx, int(n), int(k), C.c_void_p(d_V), int(n if ld_v is None else ld_v), C.c_void_p(d_w),
                                                C.c_void_p(d_out), C.c_void_p(work), int(work_bytes), C.c_void_p(stream)))

    def gmres_device(self, matrix_idx: int, d_b: int, d_x: int, d_minv: int = 0, restart: int = 30, rtol: float = 1e-6, max_iters: int = 1000,
                     check_every: int = 8, work: int = 0, work_bytes: int = 0, stream: int = 0) -> dict:
        """Restarted GMRES(restart) for a square handle, one product per inner iteration (hispmv_gmres_device); d_minv is 0 or an
        inverse diagonal used as a right preconditioner; max_iters counts inner iterations.  Result and exceptions as cg_device; a
        restart outside 1 .. 64 raises ValueError."""
        res = _lib.KrylovResult()
        self._check(lib.hispmv_gmres_device(self._ctx, int(matrix_idx), C.c_void_p(d_b), C.c_void_p(d_x), C.c_void_p(d_minv), int(restart), float(rtol),
                                            int(max_iters), int(check_every), C.c_void_p(work), int(work_bytes), C.c_void_p(stream), C.byref(res)))
        return self._krylov_result(res)

    # -- thick-restart Lanczos (hispmv_lanczos_abi.cpp; hispmv_amd.solvers.eigsh wraps these) -----------------------------------------
    def lanczos_info(self, matrix_idx: int, ncv: int = 20) -> dict:
        """{"accepted", "work_bytes", "v_offset", "stride", "hc_offset", "yt_offset", "launches_per_step", "n"} of a Lanczos run with
        ncv basis vectors on a handle (hispmv_lanczos_info): the workspace, where it keeps the basis, Hc (the betas lie right behind
        its 64 columns of 66 doubles) and the coefficients of the last rotation; zeros for a handle that is not loaded or not square."""
        return self._basis_info(lib.hispmv_lanczos_info, matrix_idx, ncv, _lib.HISPMV_LANCZOS_MAX_NCV,
                                ("accepted", "work_bytes", "v_offset", "stride", "hc_offset", "yt_offset", "launches_per_step", "n"))

    def _basis_info(self, entry, matrix_idx: int, ncv: int, max_ncv: int, keys) -> dict:
        """The eight words of lanczos_info and gk_info under `keys`."""
        out = (C.c_int64 * 8)()
        if entry(self._ctx, int(matrix_idx), int(ncv), out) != _lib.HISPMV_OK:
            if 0 <= int(matrix_idx) < self.num_matrices():
                raise ValueError(f"ncv must be 2 .. {max_ncv}")
            raise IndexError("Matrix idx out of range")
        d = dict(zip(keys, (int(x) for x in out)))
        d["accepted"] = bool(d["accepted"])
        return d

    def basis_rotate_device(self, n: int, m: int, k: int, d_V: int, d_Yt: int, d_out: int, ld_v=None, ld_out=None, stream: int = 0) -> None:
        """out[c] = sum_{i < m} Yt[c, i] * V[i] for c < k <= 64 over float32 vectors of n elements, V_i = d_V + i * ld_v, m <= 65, Yt
        float32 [k, m] in device memory (hispmv_basis_rotate_device): fp32, unfused, i ascending.  d_out may be d_V (in place, vector c
        over slot c).  Asynchronous on `stream`."""
        ld_v = int(n if ld_v is None else ld_v)
        self._check(lib.hispmv_basis_rotate_device(self._ctx, int(n), int(m), int(k), C.c_void_p(d_V), ld_v, C.c_void_p(d_Yt), C.c_void_p(d_out),
                                                   int(ld_v if ld_out is None else ld_out), C.c_void_p(stream)))

    def lanczos_steps_device(self, matrix_idx: int, j0: int, j1: int, first: bool, d_v0: int, work: int, work_bytes: int, stream: int = 0) -> None:
        """Enqueues the open (first: from the start vector d_v0) and the Lanczos steps j0 .. j1 - 1 on a square handle with no host look
        (hispmv_lanczos_steps_device); lanczos_status reads the outcome.  Exceptions as gmres_device."""
        self._check(lib.hispmv_lanczos_steps_device(self._ctx, int(matrix_idx), int(j0), int(j1), int(bool(first)), C.c_void_p(d_v0), C.c_void_p(work),
                                                    int(work_bytes), C.c_void_p(stream)))

    def lanczos_status(self, work: int, stream: int = 0) -> dict:
        """Waits for `stream` and reads {"steps", "invariant", "breakdown", "products"} of the Lanczos run with workspace `work`."""
        out = (C.c_int64 * 4)()
        self._check(lib.hispmv_lanczos_status(self._ctx, C.c_void_p(work), C.c_void_p(stream), out))
        return {"steps": int(out[0]), "invariant": bool(out[1]), "breakdown": bool(out[2]), "products": int(out[3])}

    def eigsh_device(self, matrix_idx: int, k: int, d_v0: int, d_vecs: int, ld_vecs: int, ncv: int = 20, which: str = "LA", tol: float = 1e-5,
                     max_products: int = 1000, work: int = 0, work_bytes: int = 0, stream: int = 0) -> dict:
        """The k wanted eigenpairs of a symmetric handle by thick-restart Lanczos (hispmv_eigsh_device): d_v0 the start vector, d_vecs
        takes the vectors ld_vecs floats apart.  Returns {"status", "found", "products", "cycles", "scale", "vals", "residuals"} with
        the values and residual estimates as float64 arrays [found].  An unknown `which`, a bad k / ncv / tol / max_products or a short,
        missing or misaligned workspace raises ValueError, a call before load_matrices AssertionError."""
        if which not in _lib.EIGSH_WHICH:
            raise ValueError('which must be "LA", "SA" or "LM"')
        res = _lib.EigshResult()
        vals = np.full(max(int(k), 1), np.nan, np.float64)
        resid = np.full(max(int(k), 1), np.nan, np.float64)
        self._check(lib.hispmv_eigsh_device(self._ctx, int(matrix_idx), int(k), int(ncv), _lib.EIGSH_WHICH[which], float(tol), int(max_products),
                                            C.c_void_p(d_v0), C.c_void_p(d_vecs), int(ld_vecs), vals.ctypes.data_as(C.POINTER(C.c_double)),
                                            resid.ctypes.data_as(C.POINTER(C.c_double)), C.c_void_p(work), int(work_bytes), C.c_void_p(stream),
                                            C.byref(res)))
        return {"status": _lib.KRYLOV_STATUS[res.status], "found": int(res.found), "products": int(res.products), "cycles": int(res.cycles),
                "scale": float(res.scale), "vals": vals[:res.found].copy(), "residuals": resid[:res.found].copy()}

    # -- thick-restart Golub-Kahan (hispmv_gk_abi.cpp; hispmv_amd.solvers.svds wraps these) --------------------------------------------
    def gk_info(self, matrix_idx: int, ncv: int = 20) -> dict:
        """{"accepted", "work_bytes", "v_offset", "v_stride", "u_offset", "u_stride", "gc_offset", "yt_offset"} of a Golub-Kahan run with
        ncv basis vectors on a handle (hispmv_gk_info): the workspace, where it keeps V and U, Gc (the alphas and the betas lie right
        behind its 64 columns of 66 doubles) and the coefficients of the last rotation; zeros for a handle that is not loaded or that
        spmv_device_t refuses."""
        return self._basis_info(lib.hispmv_gk_info, matrix_idx, ncv, _lib.HISPMV_GK_MAX_NCV,
                                ("accepted", "work_bytes", "v_offset", "v_stride", "u_offset", "u_stride", "gc_offset", "yt_offset"))

    def gk_steps_device(self, matrix_idx: int, ncv: int, j0: int, j1: int, first: bool, d_v0: int, work: int, work_bytes: int, stream: int = 0) -> None:
        """Enqueues the open (first: from the start vector d_v0, cols floats) and the Golub-Kahan steps j0 .. j1 - 1 <= ncv - 1 of a run
        whose workspace is gk_info(matrix_idx, ncv)'s, with no host look (hispmv_gk_steps_device); gk_status reads the outcome.
        Exceptions as svds_device."""
        self._check(lib.hispmv_gk_steps_device(self._ctx, int(matrix_idx), int(ncv), int(j0), int(j1), int(bool(first)), C.c_void_p(d_v0),
                                               C.c_void_p(work), int(work_bytes), C.c_void_p(stream)))

    def gk_status(self, work: int, stream: int = 0) -> dict:
        """Waits for `stream` and reads {"steps", "invariant", "closed_u", "breakdown", "products"} of the Golub-Kahan run with
        workspace `work`."""
        out = (C.c_int64 * 5)()
        self._check(lib.hispmv_gk_status(self._ctx, C.c_void_p(work), C.c_void_p(stream), out))
        return {"steps": int(out[0]), "invariant": bool(out[1]), "closed_u": bool(out[2]), "breakdown": bool(out[3]), "products": int(out[4])}

    def svds_device(self, matrix_idx: int, k: int, d_v0: int, d_u: int, ld_u: int, d_v: int, ld_v: int, ncv: int = 20, tol: float = 1e-5,
                    max_products: int = 1000, work: int = 0, work_bytes: int = 0, stream: int = 0, vectors: bool = True) -> dict:
        """The k largest singular values of a handle of any shape by thick-restart Golub-Kahan (hispmv_svds_device): d_v0 the start
        vector (cols floats), d_u takes the left vectors ld_u floats apart, d_v the right vectors ld_v floats apart (vectors=False:
        neither is looked at).  Returns {"status", "found", "products", "cycles", "scale", "s", "residuals"} with the values and
        residual estimates as float64 arrays [found].  A bad k / ncv / tol / max_products, a NULL or misaligned pointer or a short,
        missing or misaligned workspace raises ValueError, a call before load_matrices AssertionError, a handle spmv_device_t refuses
        its NotImplementedError."""
        res = _lib.EigshResult()
        s = np.full(max(int(k), 1), np.nan, np.float64)
        resid = np.full(max(int(k), 1), np.nan, np.float64)
        dp = C.POINTER(C.c_double)
        self._check(lib.hispmv_svds_device(self._ctx, int(matrix_idx), int(k), int(ncv), float(tol), int(max_products), C.c_void_p(d_v0),
                                           int(bool(vectors)), C.c_void_p(d_u), int(ld_u), C.c_void_p(d_v), int(ld_v), s.ctypes.data_as(dp),
                                           resid.ctypes.data_as(dp), C.c_void_p(work), int(work_bytes), C.c_void_p(stream), C.byref(res)))
        return {"status": _lib.KRYLOV_STATUS[res.status], "found": int(res.found), "products": int(res.products), "cycles": int(res.cycles),
                "scale": float(res.scale), "s": s[:res.found].copy(), "residuals": resid[:res.found].copy()}

    # -- block-Jacobi preconditioner (hispmv_block_jacobi_abi.cpp; hispmv_amd.solvers.block_jacobi wraps these) ------------------------
    def block_jacobi_info(self, matrix_idx: int, block_size: int = 8) -> dict:
        """{"accepted", "n_blocks", "pre_bytes", "setup_launches", "cg_work_bytes", "gmres_work_bytes", "gmres_step_bytes", "n"} of a
        block-Jacobi preconditioner of block_size (4, 8, 16, 32) on a handle (hispmv_block_jacobi_info): the blocks and bytes of the
        caller's buffer, the launches of a setup, the workspace of cg_bj_device and of gmres_bj_device with restart 1 plus what every
        further step of restart adds; zeros for a handle that is not loaded, not square or a tile stream."""
        out = (C.c_int64 * 8)()
        rc = lib.hispmv_block_jacobi_info(self._ctx, int(matrix_idx), int(block_size), out)
        if rc != _lib.HISPMV_OK:
            if 0 <= int(matrix_idx) < self.num_matrices():
                raise ValueError("block_size must be 4, 8, 16 or 32")
            raise IndexError("Matrix idx out of range")
        keys = ("accepted", "n_blocks", "pre_bytes", "setup_launches", "cg_work_bytes", "gmres_work_bytes", "gmres_step_bytes", "n")
        d = dict(zip(keys, (int(x) for x in out)))
        d["accepted"] = bool(d["accepted"])
        return d

    def block_jacobi_extract_device(self, matrix_idx: int, block_size: int, d_pre: int, pre_bytes: int, stream: int = 0) -> None:
        """The padded diagonal blocks of the loaded matrix, not inverted, into the block area of the buffer at d_pre
        (hispmv_block_jacobi_extract_device; the layout is prep.block_jacobi's).  Asynchronous on `stream`.  A tile-stream handle
        raises NotImplementedError; a handle that is not square, a bad block_size or a short, missing or misaligned buffer ValueError."""
        self._check(lib.hispmv_block_jacobi_extract_device(self._ctx, int(matrix_idx), int(block_size), C.c_void_p(d_pre), int(pre_bytes), C.c_void_p(stream)))

    def block_invert_device(self, d_pre: int, n_blocks: int, block_size: int, stream: int = 0) -> None:
        """Inverts the n_blocks blocks of block_size x block_size floats at d_pre in place and writes their int32 flags behind them
        (hispmv_block_invert_device): Gauss-Jordan with partial pivoting, bit for bit the rule of include/hispmv.h; a block that
        cannot be inverted becomes the identity, flag 1.  Asynchronous on `stream`."""
        self._check(lib.hispmv_block_invert_device(self._ctx, C.c_void_p(d_pre), int(n_blocks), int(block_size), C.c_void_p(stream)))

    def block_jacobi_setup_device(self, matrix_idx: int, block_size: int, d_pre: int, pre_bytes: int, stream: int = 0) -> None:
        """Extraction followed by inversion (hispmv_block_jacobi_setup_device); exceptions as block_jacobi_extract_device."""
        self._check(lib.hispmv_block_jacobi_setup_device(self._ctx, int(matrix_idx), int(block_size), C.c_void_p(d_pre), int(pre_bytes), C.c_void_p(stream)))

    def block_jacobi_status(self, d_pre: int, n: int, block_size: int, stream: int = 0) -> int:
        """Waits for `stream` and returns the number of blocks of the buffer that were replaced by the identity (hispmv_block_jacobi_status)."""
        out = C.c_int64(0)
        self._check(lib.hispmv_block_jacobi_status(self._ctx, C.c_void_p(d_pre), int(n), int(block_size), C.c_void_p(stream), C.byref(out)))
        return int(out.value)

    def block_jacobi_apply_device(self, d_pre: int, n: int, block_size: int, d_r: int, d_z: int, stream: int = 0) -> None:
        """d_z = M^-1 d_r over n float32 elements with the inverted blocks at d_pre (hispmv_block_jacobi_apply_device).  Asynchronous on
        `stream`; d_r and d_z need 4-byte alignment only."""
        self._check(lib.hispmv_block_jacobi_apply_device(self._ctx, C.c_void_p(d_pre), int(n), int(block_size), C.c_void_p(d_r), C.c_void_p(d_z),
                                                         C.c_void_p(stream)))

    def cg_bj_device(self, matrix_idx: int, d_b: int, d_x: int, d_pre: int, block_size: int, rtol: float = 1e-6, max_iters: int = 1000,
                     check_every: int = 8, work: int = 0, work_bytes: int = 0, stream: int = 0) -> dict:
        """cg_device with the block-Jacobi buffer (d_pre, block_size) in place of d_minv (hispmv_cg_bj_device); workspace, result and
        exceptions as cg_device."""
        res = _lib.KrylovResult()
        self._check(lib.hispmv_cg_bj_device(self._ctx, int(matrix_idx), C.c_void_p(d_b), C.c_void_p(d_x), C.c_void_p(d_pre), int(block_size), float(rtol),
                                            int(max_iters), int(check_every), C.c_void_p(work), int(work_bytes), C.c_void_p(stream), C.byref(res)))
        return self._krylov_result(res)

    def gmres_bj_device(self, matrix_idx: int, d_b: int, d_x: int, d_pre: int, block_size: int, restart: int = 30, rtol: float = 1e-6,
                        max_iters: int = 1000, check_every: int = 8, work: int = 0, work_bytes: int = 0, stream: int = 0) -> dict:
        """gmres_device with the block-Jacobi buffer (d_pre, block_size) in place of d_minv, as a right preconditioner
        (hispmv_gmres_bj_device); the workspace is gmres_info(..., with_minv=True)'s; result and exceptions as gmres_device."""
        res = _lib.KrylovResult()
        self._check(lib.hispmv_gmres_bj_device(self._ctx, int(matrix_idx), C.c_void_p(d_b), C.c_void_p(d_x), C.c_void_p(d_pre), int(block_size), int(restart),
                                               float(rtol), int(max_iters), int(check_every), C.c_void_p(work), int(work_bytes), C.c_void_p(stream),
                                               C.byref(res)))
        return self._krylov_result(res)

    def set_arena_bytes(self, nbytes: int) -> None:
        self._check(lib.hispmv_set_arena_bytes(self._ctx, int(nbytes)))

    def arena_bytes_used(self) -> int:
        return int(lib.hispmv_arena_bytes_used(self._ctx))

    def num_matrices(self) -> int:
        return int(lib.hispmv_num_matrices(self._ctx))

    def matrix_info(self, matrix_idx: int) -> dict:
        info = _lib.MatrixInfo()
        rc = lib.hispmv_get_matrix_info(self._ctx, int(matrix_idx), C.byref(info))
        if rc != _lib.HISPMV_OK:
            raise IndexError("Matrix idx out of range")
        return {k: getattr(info, k) for k, _ in _lib.MatrixInfo._fields_}

    def spmv_device(self, matrix_idx: int, d_x: int, d_bias: int, d_y: int, alpha: float, beta: float,
                    stream: int = 0) -> None:
        """Asynchronous launch on device pointers (ints), e.g. torch tensors' ``data_ptr()``."""
        self._check(lib.hispmv_spmv_device(self._ctx, int(matrix_idx), C.c_void_p(d_x), C.c_void_p(d_bias),
                                           C.c_void_p(d_y), float(alpha), float(beta), C.c_void_p(stream)))

    def prepare_batch(self, matrix_idxs, d_xs, d_biases, d_ys):
        """Argument block for `spmv_device_batch` (host arrays of device pointers), built once and reused."""
        n = len(matrix_idxs)
        if not (len(d_xs) == len(d_ys) == n and (d_biases is None or len(d_biases) == n)):
            raise ValueError("prepare_batch: lists of different length")
        idx = (C.c_int32 * n)(*[int(i) for i in matrix_idxs])
        xs = (C.c_void_p * n)(*[int(p) for p in d_xs])
        bs = (C.c_void_p * n)(*[int(p) for p in d_biases]) if d_biases is not None else None
        ys = (C.c_void_p * n)(*[int(p) for p in d_ys])
        return (n, idx, xs, bs, ys)

    def spmv_device_batch(self, batch, alpha: float, beta: float, stream: int = 0) -> None:
        """n independent SpMVs in as few launches as possible (hispmv_spmv_device_batch): matrices with the same
        workgroup size share one grid.  `batch` comes from `prepare_batch`.  Asynchronous on `stream`."""
        n, idx, xs, bs, ys = batch
        self._check(lib.hispmv_spmv_device_batch(self._ctx, n, idx, xs, bs, ys, float(alpha), float(beta), C.c_void_p(stream)))

    def time_device(self, matrix_idx: int, d_x: int, d_bias: int, d_y: int, alpha: float, beta: float,
                    reps: int) -> float:
        ms = lib.hispmv_time_device(self._ctx, int(matrix_idx), C.c_void_p(d_x), C.c_void_p(d_bias),
                                    C.c_void_p(d_y), float(alpha), float(beta), int(reps))
        if ms < 0:
            raise RuntimeError(self._err() or "time_device failed")
        return float(ms)

    def boundary_pack(self, d_last: int, d_mask: int, d_send: int, n: int, stream: int = 0) -> None:
        """send[i] = mask[i] * *last[i] (hispmv_boundary_pack); `stream` 0 = the context's stream, as for spmv_device."""
        self._check(lib.hispmv_boundary_pack(self._ctx, C.c_void_p(d_last), C.c_void_p(d_mask), C.c_void_p(d_send), int(n), C.c_void_p(stream)))

    def boundary_apply(self, d_first: int, d_recv: int, d_weights: int, n: int, world: int, stream: int = 0) -> None:
        """*first[i] += sum_r recv[r*n + i] * weights[i*world + r] (hispmv_boundary_apply); `stream` 0 = the context's stream."""
        self._check(lib.hispmv_boundary_apply(self._ctx, C.c_void_p(d_first), C.c_void_p(d_recv), C.c_void_p(d_weights), int(n), int(world),
                                              C.c_void_p(stream)))

    def synchronize(self) -> None:
        self._check(lib.hispmv_synchronize(self._ctx))

    def last_kernel_ms(self) -> float:
        return float(lib.hispmv_last_kernel_ms(self._ctx))

    def batch_graph_stats(self) -> dict:
        """{"instantiations", "alpha_updates"} of the HIP-graph replay of spmv_device_batch (hispmv_batch_graph_stats)."""
        import ctypes as C
        out = (C.c_int64 * 2)()
        self._check(lib.hispmv_batch_graph_stats(self._ctx, out))
        return {"instantiations": int(out[0]), "alpha_updates": int(out[1])}

    def batch_call_info(self) -> dict:
        """How the last spmv_device_batch call was issued (hispmv_batch_call_info): launches, whether its slice groups and tiles
        ran as items of the step kernel's queue, the items, the HIP streams of the main launches."""
        import ctypes as C
        out = (C.c_int64 * 4)()
        self._check(lib.hispmv_batch_call_info(self._ctx, out))
        return {"launches": int(out[0]), "step_kernel": bool(out[1]), "items": int(out[2]), "streams": int(out[3])}

    def set_step_half(self, enable: bool) -> None:
        """Batch calls that hold a bf16 handle with half groups run through the step kernel too (hispmv_set_step_half; default off:
        such calls run as grids).  Calls issued from now on run under the new state; the result bits are those of the grids."""
        self._check(lib.hispmv_set_step_half(self._ctx, int(bool(enable))))
