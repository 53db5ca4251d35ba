"""The Perceiver decoder's narrow-output 3x3x3 convolution with its pad folded into the addressing, as HIP kernels
(csrc/mgs_narrow.hip; SURVEY.md 2: agents/manigaussian_bc/perceiver_lang_io.py:322, trans_decoder = Conv3DBlock(128, 1, 3)).

    narrow_conv3d(x, weight, bias=None, padding_mode="replicate")
        F.conv3d(F.pad(x, (1,) * 6, mode='replicate' | 'constant'), weight, bias): x [B,Cin,D,H,W], weight [Cout,Cin,3,3,3], bias [Cout]
        or None; Cout 1..4, Cin 1..256; padding_mode "replicate" or "zeros".  The padded volume is never written.

An autograd function over the library's two calls.  float32 tensors on a HIP device; there is no CPU path.  A non-contiguous or
misaligned tensor takes one contiguous copy.  The backward keeps x and weight, nothing else of the volume's size, and computes only the
gradients that are asked for: the input gradient alone is one launch without a workspace and does not read x.  No atomics: the same
bits from run to run; dw and db are the same bits for every `split` of their partial sums over workgroups.  No host read, no
allocation beyond the outputs and the device's shared workspace: capturable into a HIP graph.
"""
import torch

from . import _conv, _lib, _ops

MAX_CIN, MAX_COUT = 256, 4
PADDING_MODES = ("replicate", "zeros")


class _Narrow(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, zeros, split):
        x, weight = _ops.readable(x), _ops.readable(weight)
        bias = None if bias is None else _ops.readable(bias)
        B, cin = x.shape[:2]
        cout = weight.size(0)
        ext = tuple(x.shape[2:])
        y = torch.empty((B, cout) + ext, dtype=torch.float32, device=x.device)
        _ops.call("mgs_narrow_conv3d_forward", x.device, B, cin, cout, *ext, zeros, x.data_ptr(), weight.data_ptr(), _ops.ptr(bias),
                  y.data_ptr())
        ctx.save_for_backward(x, weight)
        ctx.zeros, ctx.split, ctx.has_bias = zeros, split, bias is not None
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
        ext = tuple(x.shape[2:])
        ws = None
        if dw is not None or db is not None:
            # the partial records: written by the first launch before the second reads them
            ws = _ops.workspace(dev, _lib.lib().mgs_narrow_conv3d_workspace_bytes(B, cin, cout, *ext))
        _ops.call("mgs_narrow_conv3d_backward", dev, B, cin, cout, *ext, ctx.zeros, x.data_ptr(), g.data_ptr(), weight.data_ptr(),
                  _ops.ptr(dx), _ops.ptr(dw), _ops.ptr(db), _ops.ptr(ws), ws.numel() if ws is not None else 0, ctx.split)
        return dx, dw, db, None, None


def _narrow_conv3d(x, weight, bias=None, padding_mode="replicate", split=0):
    """narrow_conv3d with `split`: 0 = the library's split of the partial sums of dw and db over workgroups, 1..64 = that many (a
    test aid)."""
    _ops.need_float32("narrow_conv3d", ("bias",), x=x, weight=weight, bias=bias)
    if padding_mode not in PADDING_MODES:
        raise ValueError(f"padding_mode = {padding_mode!r}: 'replicate' or 'zeros'")
    _conv.check_shapes(x, weight, (3,))
    if not (1 <= weight.size(0) <= MAX_COUT and 1 <= weight.size(1) <= MAX_CIN):
        raise ValueError(f"weight {tuple(weight.shape)}: 1 to {MAX_COUT} output and 1 to {MAX_CIN} input channels")
    _conv.check_bias(x, weight, bias)
    _conv.check_rows(x)
    return _Narrow.apply(x, weight, bias, int(padding_mode == "zeros"), int(split))


def narrow_conv3d(x, weight, bias=None, padding_mode="replicate"):
    """F.conv3d(F.pad(x, (1,) * 6, mode), weight, bias) for a 3x3x3 weight [Cout <= 4, Cin <= 256, 3, 3, 3] and a bias [Cout] or None;
    x [B,Cin,D,H,W] fp32 on a HIP device; padding_mode "replicate" or "zeros"."""
    return _narrow_conv3d(x, weight, bias, padding_mode)
