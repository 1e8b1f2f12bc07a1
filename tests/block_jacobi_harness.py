"""What the GPU modules of the block-Jacobi preconditioner share (tests/test_gpu_block_jacobi.py, tests/test_gpu_block_jacobi_plans.py):
one context with matrices loaded, the device buffer taken apart, the bits of a float32 array.  No product code; not a test module and
not a conftest."""
import numpy as np

import block_jacobi_model as bj
import step_small_cases as S
from hispmv_amd import prep
from step_small_harness import HW, SHARED

f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


class Ctx:
    """One context with the given matrices (scipy COO, or a dense ndarray) loaded: the pattern of test_gpu_krylov.py.  updates: True
    or "any_storage" (set_value_updates); transposable: a state of set_transposable the handles are created under."""

    def __init__(self, torch, mats, env=S.SLICES, storage="fp32", updates=False, transposable=None):
        import pyhispmv
        self.torch, self.mats = torch, mats
        self.dev = torch.device("cuda", 0)
        with S.environment(dict(SHARED, **env)):
            self.h = pyhispmv.FpgaHandle(*HW)
            try:
                self.h.set_value_storage(storage)
                if updates:
                    self.h.set_value_updates(updates)
                if transposable is not None:
                    self.h.set_transposable(transposable)
                self.idx = []
                for A in mats:
                    if isinstance(A, np.ndarray):
                        self.idx.append(self.h.create_dense_handle(A.flatten(), *A.shape))
                    else:
                        A = A.tocoo()
                        self.idx.append(self.h.create_sparse_handle(A.row, A.col, A.data.astype(f32), *A.shape))
                    assert self.idx[-1] >= 0
                self.h.load_matrices()
            except BaseException:
                self.h.close()
                raise

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.torch.cuda.synchronize()
        self.h.close()

    def device(self, a, shift=0):
        """a on the device, `shift` floats off the 16-byte alignment of its allocation"""
        t = self.torch.empty(len(a) + shift + 4, dtype=self.torch.float32, device=self.dev)
        t[shift:shift + len(a)] = self.torch.from_numpy(np.ascontiguousarray(a, f32))
        return t[shift:shift + len(a)]

    def upload(self, raw):
        t = self.torch.from_numpy(np.ascontiguousarray(raw, np.uint8)).to(self.dev)
        assert t.data_ptr() % 16 == 0
        return t

    def products(self, k):
        """The model's callback over the library's own products on matrix k."""
        rows = self.mats[k].shape[0]

        def prod(x, bias, alpha, beta):
            dx = self.device(x)
            db = self.device(bias) if bias is not None else None
            dy = self.device(np.full(rows, np.nan, f32))
            self.torch.cuda.synchronize()          # the context's stream does not wait for torch's
            self.h.spmv_device(self.idx[k], dx.data_ptr(), db.data_ptr() if db is not None else 0, dy.data_ptr(), alpha, beta)
            self.h.synchronize()
            return dy.cpu().numpy()
        return prod, None

    def setup(self, k, bs, stream=0, only_extract=False):
        """A buffer of handle k set up (or only extracted into) by the device -> the tensor"""
        torch = self.torch
        info = self.h.block_jacobi_info(self.idx[k], bs)
        n = self.mats[k].shape[0]
        assert info["accepted"] and info["n"] == n and info["pre_bytes"] == prep.block_jacobi(n, bs)["pre_bytes"], info
        buf = torch.full((info["pre_bytes"],), 0xCD, dtype=torch.uint8, device=self.dev)
        torch.cuda.synchronize()
        call = self.h.block_jacobi_extract_device if only_extract else self.h.block_jacobi_setup_device
        call(self.idx[k], bs, buf.data_ptr(), info["pre_bytes"], stream)
        self.h.synchronize()
        torch.cuda.synchronize()
        return buf


def unpack(buf, n, bs):
    """(blocks [n_blocks, bs, bs] float32, flags int32) of a buffer tensor"""
    l = bj.layout(n, bs)
    raw = buf.cpu().numpy()
    blocks = raw[:l["n_blocks"] * bs * bs * 4].view(f32).reshape(l["n_blocks"], bs, bs)
    flags = raw[l["flags_offset"]:l["flags_offset"] + 4 * l["n_blocks"]].view(np.int32)
    return blocks, flags
