"""A sparse (or dense-overlay) layer on torch device tensors: ``y = sparse_linear(handle, idx, x, bias)`` runs forward through
FpgaHandle.linear_device and backward through FpgaHandle.linear_device_t, on torch's current stream, without the activations ever
leaving the device (FpgaHandle.linear takes host vectors: two PCIe crossings per layer and batch).

The matrix values are NOT differentiable here: no gradient flows to the handle.  The weight gradient is a sampled dense-dense product
(grad_y^T x restricted to the sparsity pattern), which this library does not compute; FpgaHandle.update_values_device is where its
result would go.  The backward pass is differentiable once (no double backward).  The autograd graph keeps a reference to the
handle, which keeps the object alive but not open: the handle must not be closed between forward and backward (a closed handle makes
backward raise, it does not launch).  torch is imported inside the functions, as in hispmv_amd/dist.py."""
from __future__ import annotations


def _check_tensor(torch, t, name: str, last: int, dims) -> None:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch tensor")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, not {t.dtype}")
    if not t.is_cuda:
        raise ValueError(f"{name} must be a device (cuda) tensor")
    if t.dim() not in dims or t.shape[-1] != last:
        raise ValueError(f"{name} must have shape {' or '.join('[B, %d]' % last if d == 2 else '[%d]' % last for d in dims)}, not {tuple(t.shape)}")


def _function(torch):
    fn = getattr(_function, "cached", None)
    if fn is not None:
        return fn

    class SparseLinear(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, bias, handle, idx, rows):
            ctx.handle, ctx.idx, ctx.has_bias = handle, idx, bias is not None
            stream = torch.cuda.current_stream(x.device).cuda_stream
            x = x.contiguous()
            y = torch.empty((x.shape[0], rows), dtype=torch.float32, device=x.device)
            b = bias.contiguous() if bias is not None else None
            handle.linear_device(idx, x.data_ptr(), x.shape[0], b.data_ptr() if b is not None else 0, y.data_ptr(), 1.0,
                                 1.0 if b is not None else 0.0, stream)
            ctx.cols = x.shape[1]
            return y

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, grad_y):
            grad_x = grad_bias = None
            if ctx.needs_input_grad[0]:
                g = grad_y.contiguous()
                stream = torch.cuda.current_stream(g.device).cuda_stream
                grad_x = torch.empty((g.shape[0], ctx.cols), dtype=torch.float32, device=g.device)
                ctx.handle.linear_device_t(ctx.idx, g.data_ptr(), g.shape[0], 0, grad_x.data_ptr(), 1.0, 0.0, 0, stream)
            if ctx.has_bias and ctx.needs_input_grad[1]:
                grad_bias = grad_y.sum(0)
            return grad_x, grad_bias, None, None, None

    _function.cached = SparseLinear
    return SparseLinear


def sparse_linear(handle, idx: int, x, bias=None):
    """y = A x (+ bias) for the loaded matrix `idx` of `handle` (an FpgaHandle): x is a float32 CUDA tensor [B, cols] or [cols] (made
    contiguous), the result [B, rows] (or [rows]); bias, if given, a float32 CUDA tensor [rows].  Differentiable in x and bias (grad_x =
    A^T grad_y through linear_device_t, grad_bias = grad_y.sum(0)); the matrix values are not differentiable.  Runs on torch's current
    stream.  A wrong dtype raises TypeError, a wrong device or shape ValueError, before any launch.  The backward pass needs a handle
    that linear_device_t accepts (a slice stream or a dense handle: FpgaHandle.set_transposable)."""
    import torch
    info = handle.matrix_info(idx)
    _check_tensor(torch, x, "x", info["cols"], (1, 2))
    if bias is not None:
        _check_tensor(torch, bias, "bias", info["rows"], (1,))
        if bias.device != x.device:
            raise ValueError("bias must be on the device of x")
    if x.dim() == 2 and x.shape[0] == 0:
        raise ValueError("x holds no vector")
    one = x.dim() == 1
    y = _function(torch).apply(x.unsqueeze(0) if one else x, bias, handle, int(idx), info["rows"])
    return y.squeeze(0) if one else y
