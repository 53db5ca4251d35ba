"""The Perceiver decoder's dense 3x3x3 / 5x5x5 convolutions with their bias and leaky ReLU as HIP kernels on the exact-f32 MFMA
(csrc/mgs_dense.hip; SURVEY.md 2: agents/manigaussian_bc/perceiver_lang_io.py, up0 = Conv3DUpsampleBlock(256, 128, 5) and final =
Conv3DBlock(256, 128, 3)).

    dense_conv3d(x, weight, bias=None, negative_slope=None)
        act(F.conv3d(x, weight, bias)): stride 1, no padding, dilation 1, groups 1; x [B,Cin,Di,Hi,Wi], weight [Cout,Cin,k,k,k] with
        k 3 or 5, bias [Cout] or None; Cin a multiple of 8 in 8..256, Cout a multiple of 32 in 32..256, every extent at least k.
        act is the identity for negative_slope None, else F.leaky_relu(., negative_slope) for a float >= 0 (0.0: ReLU).

An autograd function over the library's two calls.  float32 tensors on a HIP device; there is no CPU path.  A non-contiguous or
misaligned tensor takes one contiguous copy.  The backward keeps x, weight and y -- not the pre-activation: the incoming gradient is
scaled by y > 0 ? 1 : negative_slope, which is torch's rule since y > 0 exactly when the pre-activation is -- and computes only the
gradients that are asked for.  No atomics: the same bits from run to run; dw and db are the same bits for every `split` of their
partial sums over workgroups.  No host read; allocation is the results, one temporary of the padded output gradient's size (only when
dx is asked for) and the device's shared workspace: capturable into a HIP graph.
"""
import math

import torch

from . import _conv, _lib, _ops

KERNELS = (3, 5)
MIN_CIN, CIN_STEP, MIN_COUT, COUT_STEP, MAX_CHANNELS = 8, 8, 32, 32, 256


def _workspace(dev, B, cin, cout, k, ext):
    return _ops.workspace(dev, _lib.lib().mgs_dense_conv3d_workspace_bytes(B, cin, cout, k, *ext))


class _Dense(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, slope, split):
        x, weight = _ops.readable(x), _ops.readable(weight)
        bias = None if bias is None else _ops.readable(bias)
        B, cin = x.shape[:2]
        cout, k = weight.size(0), weight.size(2)
        ext = tuple(x.shape[2:])
        y = torch.empty((B, cout) + tuple(e - k + 1 for e in ext), dtype=torch.float32, device=x.device)
        ws = _workspace(x.device, B, cin, cout, k, ext)   # the rearranged weights: written by the first launch before the second reads them
        _ops.call("mgs_dense_conv3d_forward", x.device, B, cin, cout, k, *ext, slope, x.data_ptr(), weight.data_ptr(), _ops.ptr(bias),
                  y.data_ptr(), ws.data_ptr(), ws.numel())
        ctx.save_for_backward(x, weight, y)
        ctx.slope, ctx.split, ctx.has_bias = slope, split, bias is not None
        return y

    @staticmethod
    def backward(ctx, g):
        x, weight, y = ctx.saved_tensors
        begun = _conv.backward_begin(ctx, x, weight, g)
        if begun is None:
            return None, None, None, None, None
        g, dx, dw, db = begun
        dev = x.device
        B, cin = x.shape[:2]
        cout, k = weight.size(0), weight.size(2)
        ext = tuple(x.shape[2:])
        # the masked output gradient, zero-padded by k - 1 on every side: what the forward's kernel turns into dx
        scratch = torch.empty((B, cout) + tuple(e + k - 1 for e in ext), dtype=torch.float32, device=dev) if dx is not None else None
        ws = _workspace(dev, B, cin, cout, k, ext)   # the rearranged weights and the partial records, written before they are read
        _ops.call("mgs_dense_conv3d_backward", dev, B, cin, cout, k, *ext, ctx.slope, x.data_ptr(), y.data_ptr(), g.data_ptr(),
                  weight.data_ptr(), _ops.ptr(dx), _ops.ptr(dw), _ops.ptr(db), _ops.ptr(scratch), ws.data_ptr(), ws.numel(), ctx.split)
        return dx, dw, db, None, None


def eligible(cin, cout, kernel, ext):
    """Whether the kernels take [., cin, *ext] -> cout with a kernel^3 weight."""
    return (kernel in KERNELS and MIN_CIN <= cin <= MAX_CHANNELS and cin % CIN_STEP == 0 and MIN_COUT <= cout <= MAX_CHANNELS
            and cout % COUT_STEP == 0 and len(ext) == 3 and min(ext) >= kernel and math.prod(e + kernel - 1 for e in ext) < 2 ** 31)


def _dense_conv3d(x, weight, bias=None, negative_slope=None, split=0):
    """dense_conv3d with `split`: 0 = the library's split of the partial sums of dw and db over workgroups, 1..64 = that many (a
    test aid)."""
    _ops.need_float32("dense_conv3d", ("bias",), x=x, weight=weight, bias=bias)
    if negative_slope is not None and not (isinstance(negative_slope, (int, float)) and negative_slope >= 0):
        raise ValueError(f"negative_slope = {negative_slope!r}: None (no activation) or a number >= 0")
    _conv.check_shapes(x, weight, KERNELS)
    cout, cin, k = weight.shape[:3]
    if not (MIN_CIN <= cin <= MAX_CHANNELS and cin % CIN_STEP == 0 and MIN_COUT <= cout <= MAX_CHANNELS and cout % COUT_STEP == 0):
        raise ValueError(f"weight {tuple(weight.shape)}: a multiple of {COUT_STEP} in {MIN_COUT}..{MAX_CHANNELS} output and a multiple of "
                         f"{CIN_STEP} in {MIN_CIN}..{MAX_CHANNELS} input channels")
    _conv.check_bias(x, weight, bias)
    if min(x.shape[2:]) < k:
        raise ValueError(f"x {tuple(x.shape)}: every extent must be at least the kernel's {k}")
    if math.prod(e + k - 1 for e in x.shape[2:]) >= 2 ** 31:
        raise ValueError(f"x {tuple(x.shape)}: a (batch, channel) row, padded by {k - 1}, must hold fewer than 2^31 elements")
    if x.size(0) > 65535:
        raise ValueError(f"x {tuple(x.shape)}: at most 65535 batch entries")
    return _Dense.apply(x, weight, bias, -1.0 if negative_slope is None else float(negative_slope), int(split))


def dense_conv3d(x, weight, bias=None, negative_slope=None):
    """act(F.conv3d(x, weight, bias)) for a weight [Cout, Cin, k, k, k], k 3 or 5, Cin a multiple of 8 up to 256, Cout a multiple of 32
    up to 256, and a bias [Cout] or None; x [B,Cin,Di,Hi,Wi] fp32 on a HIP device; negative_slope None (no activation) or the leaky
    ReLU's slope >= 0."""
    return _dense_conv3d(x, weight, bias, negative_slope)
