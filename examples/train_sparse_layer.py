"""A masked (pruned) linear layer trained on the device: the sparsity pattern lives in a loaded, updatable handle, the values in a
torch tensor.  Every step runs  y = sparse_linear(h, i, x, bias, values=v)  (the values are pushed into the handle, then the sparse
product), a mean-squared loss against the outputs of a teacher layer with the same pattern, backward (grad_x through the transposed
product, grad_v through the value gradient: a sampled dense-dense product restricted to the pattern, no rows x cols matrix anywhere)
and the SGD update  v -= lr * v.grad.  Prints the loss per step; it must fall.

--bf16 trains the same layer a second time on a handle that stores its values as bfloat16 (set_value_updates("any_storage")): v stays
the fp32 master copy, every forward pass pushes it and the handle keeps R(v), the gradient is taken at the stored values
(straight-through).  The final losses of the two runs are printed side by side; no threshold is applied to their difference.

--companion creates the layer under set_transposable("companion"): the handle stores its transpose as well, grad_x runs the forward
kernels over it (no atomics), and two runs print the same losses bit for bit.  companion_info says what the second copy costs.

--spmm routes the forward product and grad_x through the wide-batch entries (sparse_linear(..., spmm=True)): the activations are
transposed to feature-major, the lanes of a wavefront are the vectors of the batch and the matrix is read once per tile of up to 256
vectors.  It needs a slice-stream handle (without --companion the handle always is one; with it, grad_x runs over the stored
transpose when that is a slice stream and through the atomics otherwise).  The update pass and the value gradient are unchanged.

--wide-grad (implies --spmm) takes the value gradient through the wide-batch entry as well (sparse_linear(..., wide_grad=True)): the
feature-major copies of x and grad_y serve all three products of a step.

--bf16-activations (implies --spmm) keeps the activations bfloat16: x is drawn in fp32 and rounded once, y and grad_x are bf16
(sparse_linear(..., spmm=True) on a bfloat16 x: FpgaHandle.spmm_device_bf16 / spmm_device_t_bf16), the loss is taken in fp32 on the
widened y; bias and the values stay fp32, and the value gradient runs through the fp32 entries on widened copies.

--bf16-wide-grad (implies --bf16-activations) takes the value gradient on the bf16 activations as well (sparse_linear(...,
wide_grad="bf16"): FpgaHandle.spmm_value_grad_device_bf16): the bf16 feature-major copies of x and grad_y serve all three products of a
step and no fp32 copy of an activation is made; the gradient itself stays fp32.

    python examples/train_sparse_layer.py [--rows 2048] [--cols 1024] [--density 0.05] [--batch 64] [--steps 10] [--lr 0.1] [--bf16]
                                          [--companion] [--spmm] [--wide-grad] [--bf16-activations] [--bf16-wide-grad]
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def train(a, r, c, start, teacher, storage: str) -> list:
    """-> the loss of every step, on a handle with the given value storage"""
    import torch
    import pyhispmv
    from hispmv_amd.torch_ops import sparse_linear

    h = pyhispmv.FpgaHandle("train.xclbin", 0, 24, 1, 1, 2, 5, True, False, True)
    try:
        # the backward pass needs the slice stream -- or, --companion, runs over a stored transpose and keeps the loader's own format
        h.set_transposable("companion" if a.companion else True)
        h.set_value_storage(storage)
        h.set_value_updates("any_storage" if storage == "bf16" else True)         # ... and the value map
        i = h.create_sparse_handle(r, c, start, a.rows, a.cols)
        assert i >= 0
        h.load_matrices()
        if a.companion:
            print(f"[{storage}] companion_info: {h.companion_info(i)} (the handle: {h.matrix_info(i)['device_bytes']} device bytes in all)")
        dev = torch.device("cuda", 0)
        gen = torch.Generator(device=dev).manual_seed(0)
        x = torch.randn((a.batch, a.cols), dtype=torch.float32, device=dev, generator=gen)
        if a.bf16_activations:
            x = x.to(torch.bfloat16)
        bias = torch.zeros(a.rows, dtype=torch.float32, device=dev)
        teacher_d, v = torch.from_numpy(teacher).to(dev), torch.from_numpy(start).to(dev).requires_grad_(True)
        torch.cuda.synchronize()
        losses = []
        # A stream of its own: sparse_linear launches on torch's CURRENT stream, and torch's default stream has the handle 0, which the
        # library reads as "the context's own stream" -- torch's kernels and the library's would then run on two streams, which
        # sparse_linear(values=...) orders with two host waits per pass.  On one real stream nothing waits.
        with torch.cuda.stream(torch.cuda.Stream(device=dev)):
            with torch.no_grad():
                target = sparse_linear(h, i, x, bias, values=teacher_d, spmm=a.spmm, wide_grad=a.wide_grad)
            for step in range(a.steps):
                y = sparse_linear(h, i, x, bias, values=v, spmm=a.spmm, wide_grad=a.wide_grad)
                loss = ((y.float() - target.float()) ** 2).mean() * a.rows
                loss.backward()
                with torch.no_grad():
                    v -= a.lr * v.grad
                    v.grad = None
                losses.append(float(loss.detach()))
                print(f"[{storage}] step {step:2d}  loss {losses[-1]:.6f}")
        torch.cuda.synchronize()
        assert losses[-1] < losses[0], "the loss did not fall"
        print(f"[{storage}] {r.size} values trained on a {a.rows} x {a.cols} pattern: loss {losses[0]:.4f} -> {losses[-1]:.4f}")
        return losses
    finally:
        h.close()


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--cols", type=int, default=1024)
    ap.add_argument("--density", type=float, default=0.05)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--lr", type=float, default=0.1)
    ap.add_argument("--bf16", action="store_true", help="train a second time on a bf16 handle and print both final losses")
    ap.add_argument("--companion", action="store_true", help="store the transpose with the handle: a deterministic backward pass, for its bytes")
    ap.add_argument("--spmm", action="store_true", help="forward and grad_x through the wide-batch entries (feature-major operands, lanes across vectors)")
    ap.add_argument("--wide-grad", action="store_true", help="the value gradient through the wide-batch entry as well (implies --spmm)")
    ap.add_argument("--bf16-activations", action="store_true", help="bfloat16 x, y and grad_x through the bf16 wide-batch entries (implies --spmm)")
    ap.add_argument("--bf16-wide-grad", action="store_true", help="the value gradient on the bf16 activations too (implies --bf16-activations)")
    a = ap.parse_args()
    a.bf16_activations = a.bf16_activations or a.bf16_wide_grad
    a.spmm = a.spmm or a.wide_grad or a.bf16_activations
    if a.bf16_wide_grad:
        a.wide_grad = "bf16"

    rng = np.random.default_rng(0)
    r, c = np.nonzero(rng.random((a.rows, a.cols)) < a.density)
    r, c = r.astype(np.int32), c.astype(np.int32)
    scale = np.float32(1.0 / np.sqrt(a.density * a.cols))
    teacher = (rng.standard_normal(r.size).astype(np.float32)) * scale
    start = (rng.standard_normal(r.size).astype(np.float32)) * scale

    fp32 = train(a, r, c, start, teacher, "fp32")
    if a.bf16:
        bf16 = train(a, r, c, start, teacher, "bf16")
        print(f"final loss after {a.steps} steps: fp32 handle {fp32[-1]:.6f}, bf16 handle {bf16[-1]:.6f}")


if __name__ == "__main__":
    main()
