"""A sparse (or dense-overlay) layer on torch device tensors: ``y = sparse_linear(handle, idx, x, bias)`` runs forward through
FpgaHandle.linear_device and backward through FpgaHandle.linear_device_t, on torch's current stream, without the activations ever
leaving the device (FpgaHandle.linear takes host vectors: two PCIe crossings per layer and batch).

Without ``values`` the matrix values are NOT differentiable: no gradient flows to the handle.  With ``values=v`` -- a float32 CUDA
tensor of the handle's n values in the order of its creation input, on an updatable handle (FpgaHandle.set_value_updates) -- the layer
is trainable on the device: the forward pass first pushes v into the handle's layouts (FpgaHandle.update_values_device: one update
pass per forward) and then multiplies; the backward pass returns grad_values[k] = sum_b grad_y[b, row_k] * x[b, col_k] through
FpgaHandle.value_grad_device, a sampled dense-dense product restricted to the pattern, in the same order.  The handle holds ONE set of
values: grad_x is computed with the values the handle holds at backward time, so nothing else may push values into the handle between
a forward pass with ``values`` and its backward pass (another forward with other values, update_values).

Streams: the launches go to torch's current stream by its handle.  torch's DEFAULT stream has the handle 0, which the library reads as
"the context's own stream" (include/hispmv.h: the stream rule): the library's launches then run on a stream that is not ordered with
torch's kernels on the default stream.  With ``values`` the layer orders the two itself when torch's current stream is the default
stream: forward and backward each wait on the host for the default stream before their launches (``values`` was written there by the
optimiser step) and for the context's stream after them (FpgaHandle.synchronize), so the natural loop ``v -= lr * v.grad`` is correct
there, at the price of two host waits per pass.  Inside ``with torch.cuda.stream(torch.cuda.Stream()):`` everything is ordered on one
real stream and nothing waits (examples/train_sparse_layer.py).  Without ``values`` the layer adds no wait, as before: on the default
stream the caller synchronises between torch's operations and the layer.  One exception: a non-contiguous ``x`` or ``bias`` is copied
inside the forward pass, on torch's current stream, where no caller can stand between the copy and the launch; on the default stream
the forward pass waits for that copy itself, and for the launch that reads it before the copy is released.

``spmm=True`` routes the forward product and grad_x through the wide-batch entries (FpgaHandle.spmm_device / spmm_device_t) on
feature-major copies of the activations; ``wide_grad=True`` on top of it takes grad_values through the wide-batch value gradient
(FpgaHandle.spmm_value_grad_device) on the same copies.  With ``spmm=True`` a bfloat16 ``x`` stays bfloat16 through both products
(FpgaHandle.spmm_device_bf16 / spmm_device_t_bf16), and ``wide_grad="bf16"`` keeps the value gradient on the bf16 copies as well
(FpgaHandle.spmm_value_grad_device_bf16).  The default route is unchanged (see sparse_linear).

The backward pass is differentiable once (no double backward).  The autograd graph keeps a reference to the handle, which keeps the
object alive but not open: the handle must not be closed between forward and backward (a closed handle makes backward raise, it does
not launch).  torch is imported inside the functions, as in hispmv_amd/dist.py."""
from __future__ import annotations


def _check_tensor(torch, t, name: str, last: int, dims, dtype=None) -> None:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch tensor")
    dtype = torch.float32 if dtype is None else dtype
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {str(dtype).replace('torch.', '')}, not {t.dtype}")
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
            current = torch.cuda.current_stream(x.device)
            stream = current.cuda_stream
            copied = not x.is_contiguous() or (bias is not None and not bias.is_contiguous())
            x = x.contiguous()
            y = torch.empty((x.shape[0], rows), dtype=torch.float32, device=x.device)
            b = bias.contiguous() if bias is not None else None
            if copied and stream == 0:        # the copies above ran on torch's default stream, which the context's stream does not wait for
                current.synchronize()
            handle.linear_device(idx, x.data_ptr(), x.shape[0], b.data_ptr() if b is not None else 0, y.data_ptr(), 1.0,
                                 1.0 if b is not None else 0.0, stream)
            if copied and stream == 0:        # ... and the copies die with this frame: torch's allocator hands their memory to the next kernel
                handle.synchronize()          # on the default stream, which must not happen while the context's stream still reads them
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


def _function_values(torch):
    fn = getattr(_function_values, "cached", None)
    if fn is not None:
        return fn

    class SparseLinearValues(torch.autograd.Function):
        """sparse_linear with ``values``: update, multiply; backward adds grad_values (value_grad_device, alpha = 1, beta = 0)."""

        @staticmethod
        def forward(ctx, x, bias, values, handle, idx, rows):
            ctx.handle, ctx.idx, ctx.has_bias = handle, idx, bias is not None
            current = torch.cuda.current_stream(x.device)
            stream = current.cuda_stream
            x = x.contiguous()
            v = values.contiguous()
            if stream == 0:                   # the default stream: the launches run on the context's own stream (module docstring)
                current.synchronize()
            handle.update_values_device(idx, v.data_ptr(), v.numel(), stream)
            y = torch.empty((x.shape[0], rows), dtype=torch.float32, device=x.device)
            b = bias.contiguous() if bias is not None else None
            handle.linear_device(idx, x.data_ptr(), x.shape[0], b.data_ptr() if b is not None else 0, y.data_ptr(), 1.0,
                                 1.0 if b is not None else 0.0, stream)
            if stream == 0:
                handle.synchronize()
            ctx.cols, ctx.n = x.shape[1], v.numel()
            if values.requires_grad:          # x is kept for the value gradient only
                ctx.save_for_backward(x)
            return y

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, grad_y):
            grad_x = grad_bias = grad_values = None
            g = grad_y.contiguous()
            current = torch.cuda.current_stream(g.device)
            stream = current.cuda_stream
            if ctx.has_bias and ctx.needs_input_grad[1]:
                grad_bias = grad_y.sum(0)
            if stream == 0 and (ctx.needs_input_grad[0] or ctx.needs_input_grad[2]):          # as in forward
                current.synchronize()
            if ctx.needs_input_grad[0]:
                grad_x = torch.empty((g.shape[0], ctx.cols), dtype=torch.float32, device=g.device)
                ctx.handle.linear_device_t(ctx.idx, g.data_ptr(), g.shape[0], 0, grad_x.data_ptr(), 1.0, 0.0, 0, stream)
            if ctx.needs_input_grad[2]:
                (x,) = ctx.saved_tensors
                grad_values = torch.empty((ctx.n,), dtype=torch.float32, device=g.device)
                ctx.handle.value_grad_device(ctx.idx, g.data_ptr(), x.data_ptr(), g.shape[0], grad_values.data_ptr(), 1.0, 0.0, stream)
            if stream == 0 and (ctx.needs_input_grad[0] or ctx.needs_input_grad[2]):
                ctx.handle.synchronize()
            return grad_x, grad_bias, grad_values, None, None, None

    _function_values.cached = SparseLinearValues
    return SparseLinearValues


def _function_spmm(torch):
    fn = getattr(_function_spmm, "cached", None)
    if fn is not None:
        return fn

    def operands(a, n_out, work_bytes, ld):
        """torch's side of a wide call on a [B, n_in] tensor: -> (at [n_in, ld] with the batch in its first B columns, out [n_out, ld],
        the workspace).  ld is B rounded up to 4, so that every batch takes the lane widths its size allows; the pad columns of
        `at` are zeros and those of `out` are not written."""
        B = a.shape[0]
        if ld == B:
            at = a.t().contiguous()
        else:
            at = torch.zeros((a.shape[1], ld), dtype=torch.float32, device=a.device)
            at[:, :B] = a.t()
        out = torch.empty((n_out, ld), dtype=torch.float32, device=a.device)
        work = torch.empty((max(work_bytes, 4) + 3) // 4, dtype=torch.float32, device=a.device)
        return at, out, work

    class SparseLinearSpmm(torch.autograd.Function):
        """sparse_linear with spmm=True: forward through spmm_device, grad_x through spmm_device_t where the handle has a slice-stream
        companion (linear_device_t otherwise); `values` (or None), the update pass and the value gradient as in the other two functions.
        Every pass first lets torch build what the library reads (the transposed activations, contiguous bias and values, the result
        and the workspace) and only then launches.  On torch's default stream (handle 0 = the context's own stream, which is not
        ordered with torch's kernels) it waits on the host between the two, and again for the context's stream behind the launches;
        torch's temporaries stay referenced until that second wait is over."""

        @staticmethod
        def forward(ctx, x, bias, values, handle, idx, rows):
            ctx.handle, ctx.idx, ctx.has_bias, ctx.has_values = handle, idx, bias is not None, values is not None
            current = torch.cuda.current_stream(x.device)
            stream = current.cuda_stream
            B = x.shape[0]
            ld = (B + 3) & ~3
            info = handle.spmm_info(idx, B, ld)
            v = values.contiguous() if values is not None else None
            b = bias.contiguous() if bias is not None else None
            xt, yt, work = operands(x, rows, info["work_bytes"], ld)
            if stream == 0:
                current.synchronize()          # torch's kernels above are done before the context's stream reads their results
            if v is not None:
                handle.update_values_device(idx, v.data_ptr(), v.numel(), stream)
                ctx.n = v.numel()
            handle.spmm_device(idx, xt.data_ptr(), B, b.data_ptr() if b is not None else 0, yt.data_ptr(), 1.0, 1.0 if b is not None else 0.0,
                               ld_x=ld, ld_y=ld, work=work.data_ptr(), work_bytes=info["work_bytes"], stream=stream)
            if stream == 0:
                handle.synchronize()           # ... and xt, work, b, v are released only behind the launches that read them
            del xt, work, b, v
            ctx.cols = x.shape[1]
            if values is not None and values.requires_grad:          # x is kept for the value gradient only
                ctx.save_for_backward(x.contiguous())
            return yt[:, :B].t()

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, grad_y):
            grad_x = grad_bias = grad_values = None
            handle, idx = ctx.handle, ctx.idx
            current = torch.cuda.current_stream(grad_y.device)
            stream = current.cuda_stream
            B = grad_y.shape[0]
            ld = (B + 3) & ~3
            if ctx.has_bias and ctx.needs_input_grad[1]:
                grad_bias = grad_y.sum(0)
            want_x, want_v = ctx.needs_input_grad[0], ctx.has_values and ctx.needs_input_grad[2]
            # torch's side first: everything the launches below read or write
            info = handle.spmm_info(idx, B, ld) if want_x else None
            wide_t = want_x and info["accepted_t"]
            g = gt = gxt = work = x = None
            if wide_t:
                gt, gxt, work = operands(grad_y, ctx.cols, info["work_bytes_t"], ld)
            if want_v or (want_x and not wide_t):
                g = grad_y.contiguous()
            if want_x and not wide_t:
                grad_x = torch.empty((B, ctx.cols), dtype=torch.float32, device=grad_y.device)
            if want_v:
                (x,) = ctx.saved_tensors
                grad_values = torch.empty((ctx.n,), dtype=torch.float32, device=grad_y.device)
            if stream == 0 and (want_x or want_v):
                current.synchronize()
            if wide_t:
                handle.spmm_device_t(idx, gt.data_ptr(), B, 0, gxt.data_ptr(), 1.0, 0.0, ld_x=ld, ld_y=ld, work=work.data_ptr(),
                                     work_bytes=info["work_bytes_t"], stream=stream)
                grad_x = gxt[:, :B].t()
            elif want_x:
                handle.linear_device_t(idx, g.data_ptr(), B, 0, grad_x.data_ptr(), 1.0, 0.0, 0, stream)
            if want_v:
                handle.value_grad_device(idx, g.data_ptr(), x.data_ptr(), B, grad_values.data_ptr(), 1.0, 0.0, stream)
            if stream == 0 and (want_x or want_v):
                handle.synchronize()
            del g, gt, work
            return grad_x, grad_bias, grad_values, None, None, None

    _function_spmm.cached = SparseLinearSpmm
    return SparseLinearSpmm


def _function_spmm_wide(torch):
    fn = getattr(_function_spmm_wide, "cached", None)
    if fn is not None:
        return fn

    def feature_major(a, ld):
        """[B, n] -> [n, ld] with the batch in the first B columns and zeros in the pad columns"""
        B = a.shape[0]
        if ld == B:
            return a.t().contiguous()
        at = torch.zeros((a.shape[1], ld), dtype=torch.float32, device=a.device)
        at[:, :B] = a.t()
        return at

    def workspace(work_bytes, device):
        return torch.empty((max(work_bytes, 4) + 3) // 4, dtype=torch.float32, device=device)

    class SparseLinearSpmmWide(torch.autograd.Function):
        """sparse_linear with spmm=True, wide_grad=True and values: SparseLinearSpmm with the value gradient through
        spmm_value_grad_device.  The forward pass keeps the feature-major xt it built for spmm_device (not x); the backward pass builds
        the feature-major grad_y once, for spmm_device_t and for the value gradient.  Stream ordering as in SparseLinearSpmm: on torch's
        default stream a host wait between torch's side and the launches and another behind them, torch's temporaries referenced
        until the second is over."""

        @staticmethod
        def forward(ctx, x, bias, values, handle, idx, rows):
            ctx.handle, ctx.idx, ctx.has_bias = handle, idx, bias is not None
            current = torch.cuda.current_stream(x.device)
            stream = current.cuda_stream
            B = x.shape[0]
            ld = (B + 3) & ~3
            info = handle.spmm_info(idx, B, ld)
            v = values.contiguous()
            b = bias.contiguous() if bias is not None else None
            xt = feature_major(x, ld)
            yt = torch.empty((rows, ld), dtype=torch.float32, device=x.device)
            work = workspace(info["work_bytes"], x.device)
            if stream == 0:
                current.synchronize()
            handle.update_values_device(idx, v.data_ptr(), v.numel(), stream)
            handle.spmm_device(idx, xt.data_ptr(), B, b.data_ptr() if b is not None else 0, yt.data_ptr(), 1.0, 1.0 if b is not None else 0.0,
                               ld_x=ld, ld_y=ld, work=work.data_ptr(), work_bytes=info["work_bytes"], stream=stream)
            if stream == 0:
                handle.synchronize()
            ctx.cols, ctx.n = x.shape[1], v.numel()
            if values.requires_grad:          # the feature-major copy is kept for the value gradient only
                ctx.save_for_backward(xt)
            del xt, work, b, v
            return yt[:, :B].t()

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, grad_y):
            grad_x = grad_bias = grad_values = None
            handle, idx = ctx.handle, ctx.idx
            current = torch.cuda.current_stream(grad_y.device)
            stream = current.cuda_stream
            B = grad_y.shape[0]
            ld = (B + 3) & ~3
            if ctx.has_bias and ctx.needs_input_grad[1]:
                grad_bias = grad_y.sum(0)
            want_x, want_v = ctx.needs_input_grad[0], ctx.needs_input_grad[2]
            # torch's side first: everything the launches below read or write
            info = handle.spmm_info(idx, B, ld) if want_x else None
            wide_t = want_x and info["accepted_t"]
            g = gt = gxt = work = xt = None
            if wide_t or want_v:
                gt = feature_major(grad_y, ld)          # ONE copy, for both products
            if wide_t:
                gxt = torch.empty((ctx.cols, ld), dtype=torch.float32, device=grad_y.device)
                work = workspace(info["work_bytes_t"], grad_y.device)
            elif want_x:
                g = grad_y.contiguous()
                grad_x = torch.empty((B, ctx.cols), dtype=torch.float32, device=grad_y.device)
            if want_v:
                (xt,) = ctx.saved_tensors
                grad_values = torch.empty((ctx.n,), dtype=torch.float32, device=grad_y.device)
            if stream == 0 and (want_x or want_v):
                current.synchronize()
            if wide_t:
                handle.spmm_device_t(idx, gt.data_ptr(), B, 0, gxt.data_ptr(), 1.0, 0.0, ld_x=ld, ld_y=ld, work=work.data_ptr(),
                                     work_bytes=info["work_bytes_t"], stream=stream)
                grad_x = gxt[:, :B].t()
            elif want_x:
                handle.linear_device_t(idx, g.data_ptr(), B, 0, grad_x.data_ptr(), 1.0, 0.0, 0, stream)
            if want_v:
                handle.spmm_value_grad_device(idx, gt.data_ptr(), xt.data_ptr(), B, grad_values.data_ptr(), 1.0, 0.0, ld_gy=ld, ld_x=ld, stream=stream)
            if stream == 0 and (want_x or want_v):
                handle.synchronize()
            del g, gt, work, xt
            return grad_x, grad_bias, grad_values, None, None, None

    _function_spmm_wide.cached = SparseLinearSpmmWide
    return SparseLinearSpmmWide


def _function_spmm_bf16(torch):
    fn = getattr(_function_spmm_bf16, "cached", None)
    if fn is not None:
        return fn

    def feature_major(a, ld, dtype):
        """[B, n] -> [n, ld] of `dtype` with the batch in the first B columns and zeros in the pad columns"""
        B = a.shape[0]
        if ld == B:
            return a.t().to(dtype).contiguous()
        at = torch.zeros((a.shape[1], ld), dtype=dtype, device=a.device)
        at[:, :B] = a.t()
        return at

    def workspace(work_bytes, device):
        return torch.empty((max(work_bytes, 4) + 3) // 4, dtype=torch.float32, device=device)

    class SparseLinearSpmmBf16(torch.autograd.Function):
        """sparse_linear with spmm=True and a bfloat16 x: forward through spmm_device_bf16 on a feature-major bf16 copy (ld = B rounded up
        to 8), y bf16; grad_x bf16 through spmm_device_t_bf16 where the handle has a slice-stream companion, otherwise linear_device_t on
        the widened grad_y, narrowed by torch.  bias is fp32, grad_bias = grad_y.float().sum(0).  `values` is the fp32 master copy:
        its gradient goes through the unchanged fp32 entries on torch-widened copies of the saved activations and of grad_y --
        spmm_value_grad_device on feature-major copies (ld = B rounded up to 4, as SparseLinearSpmmWide builds them) when `wide`,
        value_grad_device otherwise -- so it has the bits of the fp32-activation call on the widened inputs.  `wide` == "bf16": the value
        gradient stays on 2-byte operands too (spmm_value_grad_device_bf16): forward saves the bf16 feature-major xt it built anyway (not
        x), backward builds the bf16 feature-major grad_y once, for spmm_device_t_bf16 (where accepted) and for the value gradient, and no
        fp32 copy of an activation is made.  Stream ordering as in SparseLinearSpmm."""

        @staticmethod
        def forward(ctx, x, bias, values, handle, idx, rows, wide):
            ctx.handle, ctx.idx, ctx.has_bias, ctx.has_values, ctx.wide = handle, idx, bias is not None, values is not None, wide
            current = torch.cuda.current_stream(x.device)
            stream = current.cuda_stream
            B = x.shape[0]
            ld = (B + 7) & ~7
            info = handle.spmm_bf16_info(idx, B, ld)
            v = values.contiguous() if values is not None else None
            b = bias.contiguous() if bias is not None else None
            xt = feature_major(x, ld, torch.bfloat16)
            yt = torch.empty((rows, ld), dtype=torch.bfloat16, device=x.device)
            work = workspace(info["work_bytes"], x.device)
            if stream == 0:
                current.synchronize()
            if v is not None:
                handle.update_values_device(idx, v.data_ptr(), v.numel(), stream)
                ctx.n = v.numel()
            handle.spmm_device_bf16(idx, xt.data_ptr(), B, b.data_ptr() if b is not None else 0, yt.data_ptr(), 1.0, 1.0 if b is not None else 0.0,
                                    ld_x=ld, ld_y=ld, work=work.data_ptr(), work_bytes=info["work_bytes"], stream=stream)
            if stream == 0:
                handle.synchronize()
            ctx.cols = x.shape[1]
            if values is not None and values.requires_grad:          # x (or, "bf16", the feature-major copy) is kept for the value gradient only
                ctx.save_for_backward(xt if wide == "bf16" else x.contiguous())
            del xt, work, b, v
            return yt[:, :B].t()

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, grad_y):
            grad_x = grad_bias = grad_values = None
            handle, idx = ctx.handle, ctx.idx
            current = torch.cuda.current_stream(grad_y.device)
            stream = current.cuda_stream
            B = grad_y.shape[0]
            ld, ld4 = (B + 7) & ~7, (B + 3) & ~3
            if ctx.has_bias and ctx.needs_input_grad[1]:
                grad_bias = grad_y.float().sum(0)
            want_x, want_v = ctx.needs_input_grad[0], ctx.has_values and ctx.needs_input_grad[2]
            # torch's side first: everything the launches below read or write
            info = handle.spmm_bf16_info(idx, B, ld) if want_x else None
            wide_t = want_x and info["accepted_t"]
            half_v = want_v and ctx.wide == "bf16"
            g = gt = gxt = gx32 = work = g32 = x32 = xt = None
            if wide_t or half_v:
                gt = feature_major(grad_y, ld, torch.bfloat16)          # ONE copy, for both products
            if wide_t:
                gxt = torch.empty((ctx.cols, ld), dtype=torch.bfloat16, device=grad_y.device)
                work = workspace(info["work_bytes_t"], grad_y.device)
            elif want_x:
                g = grad_y.float().contiguous()
                gx32 = torch.empty((B, ctx.cols), dtype=torch.float32, device=grad_y.device)
            if half_v:
                (xt,) = ctx.saved_tensors
                grad_values = torch.empty((ctx.n,), dtype=torch.float32, device=grad_y.device)
            elif want_v:
                (x,) = ctx.saved_tensors
                if ctx.wide:
                    g32, x32 = feature_major(grad_y, ld4, torch.float32), feature_major(x, ld4, torch.float32)
                else:
                    g32, x32 = (g if g is not None else grad_y.float().contiguous()), x.float()
                grad_values = torch.empty((ctx.n,), dtype=torch.float32, device=grad_y.device)
            if stream == 0 and (want_x or want_v):
                current.synchronize()
            if wide_t:
                handle.spmm_device_t_bf16(idx, gt.data_ptr(), B, 0, gxt.data_ptr(), 1.0, 0.0, ld_x=ld, ld_y=ld, work=work.data_ptr(),
                                          work_bytes=info["work_bytes_t"], stream=stream)
                grad_x = gxt[:, :B].t()
            elif want_x:
                handle.linear_device_t(idx, g.data_ptr(), B, 0, gx32.data_ptr(), 1.0, 0.0, 0, stream)
            if half_v:
                handle.spmm_value_grad_device_bf16(idx, gt.data_ptr(), xt.data_ptr(), B, grad_values.data_ptr(), 1.0, 0.0, ld_gy=ld, ld_x=ld, stream=stream)
            elif want_v and ctx.wide:
                handle.spmm_value_grad_device(idx, g32.data_ptr(), x32.data_ptr(), B, grad_values.data_ptr(), 1.0, 0.0, ld_gy=ld4, ld_x=ld4, stream=stream)
            elif want_v:
                handle.value_grad_device(idx, g32.data_ptr(), x32.data_ptr(), B, grad_values.data_ptr(), 1.0, 0.0, stream)
            if stream == 0 and (want_x or want_v):
                handle.synchronize()
            if gx32 is not None:
                grad_x = gx32.to(torch.bfloat16)              # (on the default stream behind the wait above: gx32 is written)
            del g, gt, work, g32, x32, xt
            return grad_x, grad_bias, grad_values, None, None, None, None

    _function_spmm_bf16.cached = SparseLinearSpmmBf16
    return SparseLinearSpmmBf16


def sparse_linear(handle, idx: int, x, bias=None, values=None, spmm: bool = False, wide_grad: bool = False):
    """y = A x (+ bias) for the loaded matrix `idx` of `handle` (an FpgaHandle): x is a float32 CUDA tensor [B, cols] or [cols] (made
    contiguous), the result [B, rows] (or [rows]); bias, if given, a float32 CUDA tensor [rows].  Differentiable in x and bias (grad_x =
    A^T grad_y through linear_device_t, grad_bias = grad_y.sum(0)).  Runs on torch's current stream.  A wrong dtype raises TypeError, a
    wrong device or shape ValueError, before any launch.  The backward pass needs a handle that linear_device_t accepts: a dense handle, a slice
    stream (FpgaHandle.set_transposable(True) keeps it one) or a tile stream created under FpgaHandle.set_transposable("keep_format");
    the same holds for grad_values.  For a deterministic backward create the handle under FpgaHandle.set_transposable("companion"):
    grad_x then runs the forward kernels over the handle's stored transpose and has the same bits from run to run, like y and
    grad_values.  That costs the device bytes and creation time of a second copy of the matrix (FpgaHandle.companion_info), and every
    value update writes both.

    values=None: the matrix values are those the handle holds and are not differentiable; launches and autograd graph are those of a
    call without the parameter.

    values: a float32 CUDA tensor [n] on the device of x, n = handle.value_update_info(idx)["n"], in the order of the handle's creation
    input (COO arrays, CSR values before the per-row sort, W row-major).  The handle must be updatable (created after
    FpgaHandle.set_value_updates(True)); otherwise ValueError, before any launch; a wrong dtype TypeError, a wrong length or device
    ValueError.  The forward pass pushes `values` into the handle (update_values_device on torch's current stream: one update pass per
    forward) and multiplies.  If values.requires_grad, backward returns grad_values[k] = sum_b grad_y[b, row_k] * x[b, col_k] through
    value_grad_device (alpha = 1, beta = 0: deterministic, no atomics), and x is saved for backward (only then).  grad_x uses the values
    the handle holds at backward time: nothing else may push values into the handle between this forward and its backward.

    bf16 handles (value storage "bf16", created under FpgaHandle.set_value_updates("any_storage")): `values` is the fp32 MASTER COPY.
    The forward pass pushes it and the update rounds on the device, so the handle stores R(values) (nearest bfloat16, ties to even)
    and y, grad_x are computed with R(values).  grad_values is the gradient AT THE STORED VALUES, handed to the master copy as if
    the rounding were the identity (straight-through): it does not depend on the values at all, and equals bit for bit what the
    fp32 handle of the same input returns.  The optimiser steps the fp32 copy; steps smaller than half a bf16 ulp accumulate there.

    Streams, with values: on torch's DEFAULT stream (handle 0, which the library reads as the context's own stream) forward and
    backward each wait on the host for the default stream before their launches and for the context's stream after them, so
    ``v -= lr * v.grad`` followed by the next forward is ordered; on any other current stream nothing waits.  A loop that should not
    wait on the host runs inside ``with torch.cuda.stream(torch.cuda.Stream()):``.

    spmm=False (default): nothing changes -- the launches and the autograd graph of a call without the parameter.  spmm=True routes the
    products through the wide-batch entries (FpgaHandle.spmm_device): forward transposes x to feature-major ([cols, B], contiguous),
    allocates the result and the workspace with torch.empty on the current stream, multiplies with the shared bias and returns the
    transposed view [B, rows] of the result; grad_x does the same through spmm_device_t when the handle owns a slice-stream companion
    (FpgaHandle.set_transposable("companion"): deterministic), and falls back to linear_device_t otherwise.  The matrix is then read
    once per tile of up to 256 vectors instead of once per 4.  y and grad_x are deterministic but are not the bits of spmm=False (the
    row sums are sequential, not a segmented scan).  A handle spmm_device does not accept (a tile stream, a dense handle) raises
    NotImplementedError before any launch.  With `values`, the update pass and value_grad_device stay as they are.  The feature-major
    copies have a leading dimension of B rounded up to 4 (pad columns zero), so that an odd batch still takes the lane widths its size
    allows.  On torch's default stream every pass waits on the host after torch has built those copies and again behind the library's
    launches (the context's stream is not ordered with torch's kernels).

    spmm=True with a bfloat16 x (CUDA, [B, cols] or [cols]): the activations stay bf16.  Forward builds a feature-major bf16 copy (leading
    dimension B rounded up to 8, so that every batch takes the lane widths its size allows), multiplies through
    FpgaHandle.spmm_device_bf16 and returns a bf16 [B, rows]: per element the fp32 value of the float32 route on x.float(), rounded once.
    grad_x is bf16: through spmm_device_t_bf16 where the handle has a slice-stream companion, otherwise linear_device_t on the widened
    grad_y, narrowed by torch.  bias stays a float32 [rows] tensor and grad_bias = grad_y.float().sum(0); `values` stays the float32
    master copy, and its gradient goes through the unchanged fp32 gradient entries (wide_grad or not) on torch-widened copies of x and
    grad_y: bit for bit the gradient of the float32 route on the widened tensors.  With spmm=False a bfloat16 x raises TypeError.

    wide_grad=False (default): nothing changes.  wide_grad=True needs spmm=True and `values` (otherwise ValueError, before any launch)
    and takes grad_values through FpgaHandle.spmm_value_grad_device: the forward pass saves the feature-major copy of x it built
    anyway (instead of x), the backward pass builds the feature-major grad_y once and uses it for spmm_device_t (where the handle has
    a slice-stream companion) and for the value gradient, which then reads the slice stream once per tile of up to 256 vectors
    instead of once per 4.  y and grad_x keep the bits of spmm=True; grad_values is deterministic, but its bits are not those of
    value_grad_device and depend on the batch size (the sums go lane by lane, then over the lanes as a pairwise tree).

    wide_grad="bf16": a third state, for a bfloat16 x (it needs one, spmm=True and `values`; otherwise, or for any state other than
    False, True and "bf16", ValueError before any launch).  y and grad_x are those of wide_grad=True; grad_values goes through
    FpgaHandle.spmm_value_grad_device_bf16 on the bf16 feature-major copies: forward saves the copy of x it built anyway (leading
    dimension B rounded up to 8), backward builds the copy of grad_y once, for spmm_device_t_bf16 and for the value gradient, and no
    float32 copy of an activation is made.  grad_values is float32 and deterministic; a lane owns up to 8 vectors, so its bits are
    those of wide_grad=True only where both entries take the same lane width and tiles."""
    import torch
    if not (isinstance(wide_grad, bool) or (isinstance(wide_grad, str) and wide_grad == "bf16")):
        raise ValueError('wide_grad must be False, True or "bf16"')
    if wide_grad and not spmm:
        raise ValueError("wide_grad=True needs spmm=True")
    if wide_grad and values is None:
        raise ValueError("wide_grad=True needs values")
    if wide_grad == "bf16" and not (isinstance(x, torch.Tensor) and x.dtype == torch.bfloat16):
        raise ValueError('wide_grad="bf16" needs a bfloat16 x')
    info = handle.matrix_info(idx)
    bf16 = spmm and isinstance(x, torch.Tensor) and x.dtype == torch.bfloat16
    _check_tensor(torch, x, "x", info["cols"], (1, 2), torch.bfloat16 if bf16 else torch.float32)
    if bias is not None:
        _check_tensor(torch, bias, "bias", info["rows"], (1,))
        if bias.device != x.device:
            raise ValueError("bias must be on the device of x")
    if x.dim() == 2 and x.shape[0] == 0:
        raise ValueError("x holds no vector")
    one = x.dim() == 1
    if spmm and not handle.spmm_info(idx, 1)["accepted"]:
        raise NotImplementedError("sparse_linear(spmm=True) needs a loaded slice-stream handle (FpgaHandle.set_transposable(True) keeps a sparse "
                                  "handle one); tile-stream and dense handles have no wide-batch kernel")
    if values is None and bf16:
        y = _function_spmm_bf16(torch).apply(x.unsqueeze(0) if one else x, bias, None, handle, int(idx), info["rows"], False)
        return y.squeeze(0) if one else y
    if values is None and spmm:
        y = _function_spmm(torch).apply(x.unsqueeze(0) if one else x, bias, None, handle, int(idx), info["rows"])
        return y.squeeze(0) if one else y
    if values is None:
        y = _function(torch).apply(x.unsqueeze(0) if one else x, bias, handle, int(idx), info["rows"])
        return y.squeeze(0) if one else y
    upd = handle.value_update_info(idx)
    if not upd["updatable"]:
        raise ValueError("values needs an updatable handle: create it after FpgaHandle.set_value_updates(True)")
    _check_tensor(torch, values, "values", upd["n"], (1,))
    if values.device != x.device:
        raise ValueError("values must be on the device of x")
    if bf16:
        y = _function_spmm_bf16(torch).apply(x.unsqueeze(0) if one else x, bias, values, handle, int(idx), info["rows"], wide_grad)
        return y.squeeze(0) if one else y
    if spmm:
        fn = _function_spmm_wide(torch) if wide_grad else _function_spmm(torch)
        y = fn.apply(x.unsqueeze(0) if one else x, bias, values, handle, int(idx), info["rows"])
        return y.squeeze(0) if one else y
    y = _function_values(torch).apply(x.unsqueeze(0) if one else x, bias, values, handle, int(idx), info["rows"])
    return y.squeeze(0) if one else y
