"""The voxel encoder stem's 3x3x3 convolutions as direct HIP kernels (csrc/mgs_conv3d.hip; SURVEY.md 2: helpers/network_utils.py:234-306).

    conv3d(x, weight, stride=1)
        F.conv3d(x, weight, None, stride, padding=1): x [B,Cin,D,H,W], weight [Cout,Cin,3,3,3], stride 1 or 2, 1..64 channels.
    conv_transpose3d(x, weight, output_padding=0)
        F.conv_transpose3d(x, weight, None, stride=2, padding=1, output_padding=output_padding): x [B,Cin,D,H,W],
        weight [Cin,Cout,3,3,3], output_padding 0 or 1 (the same in the three dimensions): [B,Cout,2D-1+op,2H-1+op,2W-1+op].

Both are autograd functions over the library's three passes (forward, backward-data, backward-weight): the transposed convolution's
forward is the convolution's backward-data, its input gradient the convolution's forward, its weight gradient the convolution's with
the two volumes exchanged.  float32 tensors on a HIP device; there is no CPU path.  A non-contiguous or misaligned tensor takes one
contiguous copy.  The backward keeps x and weight, nothing else of the volume's size, and computes only the gradients that are asked
for.  No atomics: the same bits from run to run; the weight gradient is the same bits for every `split` of its partial sums over
workgroups.  No host read, no allocation beyond the outputs and the device's shared workspace: capturable into a HIP graph.
"""
import torch

from . import _conv, _lib, _ops

MAX_C = 64


def _forward(x, w, y, B, cin, cout, ext, stride):
    _ops.call("mgs_conv3d_forward", x.device, B, cin, cout, *ext, stride, x.data_ptr(), w.data_ptr(), y.data_ptr())


def _backward_data(g, w, dx, B, cin, cout, ext, stride):
    _ops.call("mgs_conv3d_backward_data", g.device, B, cin, cout, *ext, stride, g.data_ptr(), w.data_ptr(), dx.data_ptr())


def _backward_weight(x, g, dw, B, cin, cout, ext, stride, split):
    # the partial records: written by the first launch before the second reads them
    ws = _ops.workspace(x.device, _lib.lib().mgs_conv3d_workspace_bytes(B, cin, cout, *ext, stride))
    _ops.call("mgs_conv3d_backward_weight", x.device, B, cin, cout, *ext, stride, x.data_ptr(), g.data_ptr(), dw.data_ptr(),
              ws.data_ptr(), ws.numel(), split)


def _out_extent(i, stride):
    return (i - 1) // stride + 1


class _Conv3d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, stride, split):
        x, weight = _ops.readable(x), _ops.readable(weight)
        B, cin = x.shape[:2]
        cout = weight.size(0)
        ext = tuple(x.shape[2:])
        y = torch.empty((B, cout) + tuple(_out_extent(i, stride) for i in ext), dtype=torch.float32, device=x.device)
        _forward(x, weight, y, B, cin, cout, ext, stride)
        ctx.save_for_backward(x, weight)
        ctx.stride, ctx.split = stride, split
        return y

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        B, cin = x.shape[:2]
        cout = weight.size(0)
        ext = tuple(x.shape[2:])
        dx = dw = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            g = _ops.readable(g)
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            _backward_data(g, weight, dx, B, cin, cout, ext, ctx.stride)
        if ctx.needs_input_grad[1]:
            dw = torch.empty_like(weight)
            _backward_weight(x, g, dw, B, cin, cout, ext, ctx.stride, ctx.split)
        return dx, dw, None, None


class _ConvTranspose3d(torch.autograd.Function):
    """The convolution it transposes has Cin = this op's output channels, Cout = its input channels, stride 2, and this op's OUTPUT
    as its input side."""

    @staticmethod
    def forward(ctx, x, weight, output_padding, split):
        x, weight = _ops.readable(x), _ops.readable(weight)
        B, cout = x.shape[:2]
        cin = weight.size(1)
        ext = tuple(2 * i - 1 + output_padding for i in x.shape[2:])
        y = torch.empty((B, cin) + ext, dtype=torch.float32, device=x.device)
        _backward_data(x, weight, y, B, cin, cout, ext, 2)
        ctx.save_for_backward(x, weight)
        ctx.ext, ctx.split = ext, split
        return y

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        B, cout = x.shape[:2]
        cin = weight.size(1)
        dx = dw = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            g = _ops.readable(g)
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            _forward(g, weight, dx, B, cin, cout, ctx.ext, 2)
        if ctx.needs_input_grad[1]:
            dw = torch.empty_like(weight)
            _backward_weight(g, x, dw, B, cin, cout, ctx.ext, 2, ctx.split)
        return dx, dw, None, None


def _check(op, x, weight, channel_dim):
    _ops.need_float32(op, x=x, weight=weight)
    _conv.check_shapes(x, weight, (3,), channel_dim)
    if not (1 <= weight.size(0) <= MAX_C and 1 <= weight.size(1) <= MAX_C):
        raise ValueError(f"weight {tuple(weight.shape)}: 1 to {MAX_C} channels on either side")
    _conv.check_rows(x)


def _conv3d(x, weight, stride=1, split=0):
    """conv3d with `split`: 0 = the library's split of the weight gradient's partial sums over workgroups, 1..64 = that many (a
    test aid)."""
    _check("conv3d", x, weight, 1)
    if stride not in (1, 2):
        raise ValueError(f"stride = {stride!r}: 1 or 2 (the same in the three dimensions)")
    return _Conv3d.apply(x, weight, int(stride), int(split))


def _conv_transpose3d(x, weight, output_padding=0, split=0):
    _check("conv_transpose3d", x, weight, 0)
    if output_padding not in (0, 1):
        raise ValueError(f"output_padding = {output_padding!r}: 0 or 1 (the same in the three dimensions)")
    ext = [2 * i - 1 + output_padding for i in x.shape[2:]]
    if ext[0] * ext[1] * ext[2] >= 2 ** 31:
        raise ValueError(f"x {tuple(x.shape)}: the output's (batch, channel) rows must hold fewer than 2^31 elements")
    return _ConvTranspose3d.apply(x, weight, int(output_padding), int(split))


def conv3d(x, weight, stride=1):
    """F.conv3d(x, weight, None, stride, padding=1) for a 3x3x3 weight [Cout,Cin,3,3,3]; x [B,Cin,D,H,W] fp32 on a HIP device."""
    return _conv3d(x, weight, stride)


def conv_transpose3d(x, weight, output_padding=0):
    """F.conv_transpose3d(x, weight, None, stride=2, padding=1, output_padding=output_padding) for a 3x3x3 weight [Cin,Cout,3,3,3];
    x [B,Cin,D,H,W] fp32 on a HIP device."""
    return _conv_transpose3d(x, weight, output_padding)
