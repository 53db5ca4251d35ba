"""The voxel encoder stem's 1x1x1 convolution with bias as HIP kernels (csrc/mgs_pointwise.hip; SURVEY.md 2:
helpers/network_utils.py:248-306, conv_out).

    pointwise_conv3d(x, weight, bias=None)
        F.conv3d(x, weight, bias): x [B,Cin,D,H,W], weight [Cout,Cin,1,1,1], bias [Cout] or None, 1..64 channels on either side.
    wide_pointwise_conv3d(x, weight, bias=None)
        the same for 1..16 input and 65..256 output channels (conv_out at final_dim = 128: 8 -> 128), over mgs_pointwise_wide_*.

One autograd function over a family's two calls (the entry points' prefix says which).  float32 tensors on a HIP device; there is no CPU path.  A non-contiguous or
misaligned tensor takes one contiguous copy.  The backward keeps x and weight, nothing else of the volume's size, and computes only the
gradients that are asked for: the input gradient alone is one launch; with the weight's or the bias's gradient the incoming gradient
is read once for all three (up to 16 input channels; the wide op walks its output channels in blocks of 64 inside that one launch,
and its dx is the same bits whether or not the other two are asked for, as the narrow op's is).  No atomics: the same bits from run to run; dw and db are the same bits for
every `split` of their partial sums over workgroups.  No host read, no allocation beyond the outputs and the device's shared
workspace: capturable into a HIP graph.
"""
import torch

from . import _conv, _lib, _ops

MAX_C = 64
WIDE_MAX_CIN, WIDE_MIN_COUT, WIDE_MAX_COUT = 16, 65, 256
NARROW, WIDE = "mgs_pointwise_", "mgs_pointwise_wide_"   # the two families' entry points


class _Pointwise(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, split, prefix):
        x, weight = _ops.readable(x), _ops.readable(weight)
        bias = None if bias is None else _ops.readable(bias)
        B, cin = x.shape[:2]
        cout = weight.size(0)
        n = x[0, 0].numel()
        y = torch.empty((B, cout) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
        _ops.call(prefix + "forward", x.device, B, cin, cout, n, x.data_ptr(), weight.data_ptr(), _ops.ptr(bias), y.data_ptr())
        ctx.save_for_backward(x, weight)
        ctx.split, ctx.has_bias, ctx.prefix = split, bias is not None, prefix
        return y

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        begun = _conv.backward_begin(ctx, x, weight, g)
        if begun is None:
            return None, None, None, None, None
        g, dx, dw, db = begun
        dev = x.device
        B, cin = x.shape[:2]
        cout = weight.size(0)
        n = x[0, 0].numel()
        ws = None
        if dw is not None or db is not None:
            # the partial records: written by the first launch before the second reads them
            ws = _ops.workspace(dev, getattr(_lib.lib(), ctx.prefix + "workspace_bytes")(B, cin, cout, n))
        _ops.call(ctx.prefix + "backward", dev, B, cin, cout, n, x.data_ptr(), g.data_ptr(), weight.data_ptr(), _ops.ptr(dx),
                  _ops.ptr(dw), _ops.ptr(db), _ops.ptr(ws), ws.numel() if ws is not None else 0, ctx.split)
        return dx, dw, db, None, None


def _checked(name, x, weight, bias, channels_ok, channels):
    """The checks of either op; channels_ok(cout, cin): its channel ranges, `channels` their wording."""
    _ops.need_float32(name, ("bias",), x=x, weight=weight, bias=bias)
    _conv.check_shapes(x, weight, (1,))
    if not channels_ok(weight.size(0), weight.size(1)):
        raise ValueError(f"weight {tuple(weight.shape)}: {channels}")
    _conv.check_bias(x, weight, bias)
    _conv.check_rows(x)


def _pointwise_conv3d(x, weight, bias=None, split=0):
    """pointwise_conv3d with `split`: 0 = the library's split of the partial sums of dw and db over workgroups, 1..64 = that many (a
    test aid)."""
    _checked("pointwise_conv3d", x, weight, bias, lambda cout, cin: 1 <= cout <= MAX_C and 1 <= cin <= MAX_C,
             f"1 to {MAX_C} channels on either side")
    return _Pointwise.apply(x, weight, bias, int(split), NARROW)


def pointwise_conv3d(x, weight, bias=None):
    """F.conv3d(x, weight, bias) for a 1x1x1 weight [Cout,Cin,1,1,1] and a bias [Cout] or None; x [B,Cin,D,H,W] fp32 on a HIP device."""
    return _pointwise_conv3d(x, weight, bias)


def _wide_pointwise_conv3d(x, weight, bias=None, split=0):
    """wide_pointwise_conv3d with `split`, as _pointwise_conv3d."""
    _checked("wide_pointwise_conv3d", x, weight, bias,
             lambda cout, cin: WIDE_MIN_COUT <= cout <= WIDE_MAX_COUT and 1 <= cin <= WIDE_MAX_CIN,
             f"1 to {WIDE_MAX_CIN} input and {WIDE_MIN_COUT} to {WIDE_MAX_COUT} output channels (pointwise_conv3d takes 1 to {MAX_C})")
    return _Pointwise.apply(x, weight, bias, int(split), WIDE)


def wide_pointwise_conv3d(x, weight, bias=None):
    """F.conv3d(x, weight, bias) for a 1x1x1 weight [Cout,Cin,1,1,1] with Cin 1..16 and Cout 65..256, and a bias [Cout] or None;
    x [B,Cin,D,H,W] fp32 on a HIP device."""
    return _wide_pointwise_conv3d(x, weight, bias)
