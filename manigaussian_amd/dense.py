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

from . import _lib, _ops
from .conv3d import _readable

KERNELS = (3, 5)
MIN_CIN, CIN_STEP, MIN_COUT, COUT_STEP, MAX_CHANNELS = 8, 8, 32, 32, 256


def _workspace(dev, B, cin, cout, k, ext):
    return _ops.workspace(dev, _lib.lib().mgs_dense_conv3d_workspace_bytes(B, cin, cout, k, *ext))


class _Dense(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, slope, split):
        x, weight = _readable(x), _readable(weight)
        bias = None if bias is None else _readable(bias)
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
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_b = ctx.has_bias and ctx.needs_input_grad[2]
        if not (need_x or need_w or need_b):
            return None, None, None, None, None
        dev = x.device
        B, cin = x.shape[:2]
        cout, k = weight.size(0), weight.size(2)
        ext = tuple(x.shape[2:])
        g = _readable(g)
        dx = torch.empty_like(x) if need_x else None
        dw = torch.empty_like(weight) if need_w else None
        db = torch.empty(cout, dtype=torch.float32, device=dev) if need_b else None
        # the masked output gradient, zero-padded by k - 1 on every side: what the forward's kernel turns into dx
        scratch = torch.empty((B, cout) + tuple(e + k - 1 for e in ext), dtype=torch.float32, device=dev) if need_x else None
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
    for name, t in (("x", x), ("weight", weight), ("bias", bias)):
        if t is None and name == "bias":
            continue
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
            raise RuntimeError(f"dense_conv3d needs float32 tensors on a HIP device ({name} is "
                               f"{getattr(t, 'dtype', type(t))} on {getattr(t, 'device', 'the host')}); there is no CPU path")
    if negative_slope is not None and not (isinstance(negative_slope, (int, float)) and negative_slope >= 0):
        raise ValueError(f"negative_slope = {negative_slope!r}: None (no activation) or a number >= 0")
    if x.dim() != 5 or x.numel() == 0:
        raise ValueError(f"expected x [B,C,D,H,W] with no empty dimension, got {tuple(x.shape)}")
    if weight.dim() != 5 or weight.size(2) not in KERNELS or len(set(weight.shape[2:])) != 1 or weight.size(1) != x.size(1):
        raise ValueError(f"weight {tuple(weight.shape)} is not a 3x3x3 or 5x5x5 kernel over the {x.size(1)} channels of x")
    if weight.device != x.device:
        raise ValueError(f"weight must be on {x.device}")
    cout, cin, k = weight.shape[:3]
    if not (MIN_CIN <= cin <= MAX_CHANNELS and cin % CIN_STEP == 0 and MIN_COUT <= cout <= MAX_CHANNELS and cout % COUT_STEP == 0):
        raise ValueError(f"weight {tuple(weight.shape)}: a multiple of {COUT_STEP} in {MIN_COUT}..{MAX_CHANNELS} output and a multiple of "
                         f"{CIN_STEP} in {MIN_CIN}..{MAX_CHANNELS} input channels")
    if bias is not None and (tuple(bias.shape) != (cout,) or bias.device != x.device):
        raise ValueError(f"bias must be a [{cout}] tensor on {x.device}, got {tuple(bias.shape)} on {bias.device}")
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
