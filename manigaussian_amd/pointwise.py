"""The voxel encoder stem's 1x1x1 convolution with bias as HIP kernels (csrc/mgs_pointwise.hip; SURVEY.md 2:
helpers/network_utils.py:248-306, conv_out).

    pointwise_conv3d(x, weight, bias=None)
        F.conv3d(x, weight, bias): x [B,Cin,D,H,W], weight [Cout,Cin,1,1,1], bias [Cout] or None, 1..64 channels on either side.

An autograd function over the library's two calls.  float32 tensors on a HIP device; there is no CPU path.  A non-contiguous or
misaligned tensor takes one contiguous copy.  The backward keeps x and weight, nothing else of the volume's size, and computes only the
gradients that are asked for: the input gradient alone is one launch; with the weight's or the bias's gradient the incoming gradient
is read once for all three (up to 16 input channels).  No atomics: the same bits from run to run; dw and db are the same bits for
every `split` of their partial sums over workgroups.  No host read, no allocation beyond the outputs and the device's shared
workspace: capturable into a HIP graph.
"""
import torch

from . import _conv, _lib, _ops

MAX_C = 64


class _Pointwise(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, split):
        x, weight = _ops.readable(x), _ops.readable(weight)
        bias = None if bias is None else _ops.readable(bias)
        B, cin = x.shape[:2]
        cout = weight.size(0)
        n = x[0, 0].numel()
        y = torch.empty((B, cout) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
        _ops.call("mgs_pointwise_forward", x.device, B, cin, cout, n, x.data_ptr(), weight.data_ptr(), _ops.ptr(bias), y.data_ptr())
        ctx.save_for_backward(x, weight)
        ctx.split, ctx.has_bias = split, bias is not None
        return y

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        begun = _conv.backward_begin(ctx, x, weight, g)
        if begun is None:
            return None, None, None, None
        g, dx, dw, db = begun
        dev = x.device
        B, cin = x.shape[:2]
        cout = weight.size(0)
        n = x[0, 0].numel()
        ws = None
        if dw is not None or db is not None:
            # the partial records: written by the first launch before the second reads them
            ws = _ops.workspace(dev, _lib.lib().mgs_pointwise_workspace_bytes(B, cin, cout, n))
        _ops.call("mgs_pointwise_backward", dev, B, cin, cout, n, x.data_ptr(), g.data_ptr(), weight.data_ptr(), _ops.ptr(dx),
                  _ops.ptr(dw), _ops.ptr(db), _ops.ptr(ws), ws.numel() if ws is not None else 0, ctx.split)
        return dx, dw, db, None


def _pointwise_conv3d(x, weight, bias=None, split=0):
    """pointwise_conv3d with `split`: 0 = the library's split of the partial sums of dw and db over workgroups, 1..64 = that many (a
    test aid)."""
    _ops.need_float32("pointwise_conv3d", ("bias",), x=x, weight=weight, bias=bias)
    _conv.check_shapes(x, weight, (1,))
    if not (1 <= weight.size(0) <= MAX_C and 1 <= weight.size(1) <= MAX_C):
        raise ValueError(f"weight {tuple(weight.shape)}: 1 to {MAX_C} channels on either side")
    _conv.check_bias(x, weight, bias)
    _conv.check_rows(x)
    return _Pointwise.apply(x, weight, bias, int(split))


def pointwise_conv3d(x, weight, bias=None):
    """F.conv3d(x, weight, bias) for a 1x1x1 weight [Cout,Cin,1,1,1] and a bias [Cout] or None; x [B,Cin,D,H,W] fp32 on a HIP device."""
    return _pointwise_conv3d(x, weight, bias)
