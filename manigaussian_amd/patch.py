"""The Perceiver's patch embedding -- a Conv3d whose stride is its kernel -- with its pad folded into the addressing and its bias and
ReLU / leaky ReLU in the epilogue, as HIP kernels on the exact-f32 MFMA (csrc/mgs_patch.hip; SURVEY.md 2:
agents/manigaussian_bc/perceiver_lang_io.py:235, patchify = Conv3DBlock(128, 128, kernel_sizes=5, strides=5, activation='relu')).

    patch_conv3d(x, weight, bias=None, padding=0, padding_mode="replicate", negative_slope=None)
        act(F.conv3d(F.pad(x, (padding,) * 6, mode='replicate' | 'constant'), weight, bias, stride=k)): x [B,Cin,D,H,W], weight
        [Cout,Cin,k,k,k] with k 2..5, bias [Cout] or None; padding 0..k-1; Cin a multiple of 8 in 8..256, Cout a multiple of 32 in
        32..256.  act is the identity for negative_slope None, else F.leaky_relu(., negative_slope) for a float >= 0 (0.0: ReLU).  The
        padded volume is never written.

An autograd function over the library's two calls.  float32 tensors on a HIP device; there is no CPU path.  A non-contiguous or
misaligned tensor takes one contiguous copy.  The backward keeps x, weight and -- with an activation -- y, nothing else of the
volume's size: the incoming gradient is scaled by y > 0 ? 1 : negative_slope, which is torch's rule since y > 0 exactly when the
pre-activation is.  Only the gradients that are asked for are computed; the input gradient alone is one launch without a workspace.
A voxel past the last patch belongs to no output: its gradient is zero, written by the same launch.  No atomics: the same bits from
run to run; dw and db are the same bits for every `split` of their partial sums over workgroups.  No host read, no allocation beyond
the results and the device's shared workspace: capturable into a HIP graph.
"""
import torch

from . import _conv, _lib, _ops

KERNELS = (2, 3, 4, 5)
MIN_CIN, CIN_STEP, MIN_COUT, COUT_STEP, MAX_CHANNELS = 8, 8, 32, 32, 256
PADDING_MODES = ("replicate", "zeros")


def out_extents(ext, k, pad):
    return tuple((e + 2 * pad - k) // k + 1 for e in ext)


class _Patch(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, pad, zeros, slope, split):
        x, weight = _ops.readable(x), _ops.readable(weight)
        bias = None if bias is None else _ops.readable(bias)
        B, cin = x.shape[:2]
        cout, k = weight.size(0), weight.size(2)
        ext = tuple(x.shape[2:])
        y = torch.empty((B, cout) + out_extents(ext, k, pad), dtype=torch.float32, device=x.device)
        # the rearranged weights: written by the first launch before the second reads them
        ws = _ops.workspace(x.device, _lib.lib().mgs_patch_conv3d_workspace_bytes(B, cin, cout, k, pad, *ext))
        _ops.call("mgs_patch_conv3d_forward", x.device, B, cin, cout, k, pad, *ext, zeros, slope, x.data_ptr(), weight.data_ptr(),
                  _ops.ptr(bias), y.data_ptr(), ws.data_ptr(), ws.numel())
        if slope >= 0:
            ctx.save_for_backward(x, weight, y)
        else:
            ctx.save_for_backward(x, weight)
        ctx.pad, ctx.zeros, ctx.slope, ctx.split, ctx.has_bias = pad, zeros, slope, split, bias is not None
        return y

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors[:2]
        y = ctx.saved_tensors[2] if ctx.slope >= 0 else None
        begun = _conv.backward_begin(ctx, x, weight, g)
        if begun is None:
            return (None,) * 7
        g, dx, dw, db = begun
        dev = x.device
        B, cin = x.shape[:2]
        cout, k = weight.size(0), weight.size(2)
        ext = tuple(x.shape[2:])
        ws = None
        if dw is not None or db is not None:
            # the partial records: written by the first launch before the second reads them
            ws = _ops.workspace(dev, _lib.lib().mgs_patch_conv3d_workspace_bytes(B, cin, cout, k, ctx.pad, *ext))
        _ops.call("mgs_patch_conv3d_backward", dev, B, cin, cout, k, ctx.pad, *ext, ctx.zeros, ctx.slope, x.data_ptr(), _ops.ptr(y),
                  g.data_ptr(), weight.data_ptr(), _ops.ptr(dx), _ops.ptr(dw), _ops.ptr(db), _ops.ptr(ws),
                  ws.numel() if ws is not None else 0, ctx.split)
        return dx, dw, db, None, None, None, None


def eligible(cin, cout, kernel, pad, ext, batch=1):
    """Whether the kernels take [batch, cin, *ext] -> cout with a kernel^3 weight at stride kernel and this pad."""
    if not (kernel in KERNELS and isinstance(pad, int) and 0 <= pad < kernel and MIN_CIN <= cin <= MAX_CHANNELS and cin % CIN_STEP == 0
            and MIN_COUT <= cout <= MAX_CHANNELS and cout % COUT_STEP == 0 and len(ext) == 3 and 1 <= batch <= 65535):
        return False
    if min(ext) < 1 or min(ext) + 2 * pad < kernel or ext[0] * ext[1] * ext[2] >= 2 ** 31:
        return False
    out = out_extents(ext, kernel, pad)
    return batch * out[0] * out[1] * out[2] < 2 ** 31


def _patch_conv3d(x, weight, bias=None, padding=0, padding_mode="replicate", negative_slope=None, split=0):
    """patch_conv3d with `split`: 0 = the library's split of the partial sums of dw and db over workgroups, 1..64 = that many (a
    test aid)."""
    _ops.need_float32("patch_conv3d", ("bias",), x=x, weight=weight, bias=bias)
    if padding_mode not in PADDING_MODES:
        raise ValueError(f"padding_mode = {padding_mode!r}: 'replicate' or 'zeros'")
    if negative_slope is not None and not (isinstance(negative_slope, (int, float)) and negative_slope >= 0):
        raise ValueError(f"negative_slope = {negative_slope!r}: None (no activation) or a number >= 0")
    _conv.check_shapes(x, weight, KERNELS)
    cout, cin, k = weight.shape[:3]
    if not (isinstance(padding, int) and not isinstance(padding, bool) and 0 <= padding < k):
        raise ValueError(f"padding = {padding!r}: an integer in 0..{k - 1}, the same on every side")
    if not (MIN_CIN <= cin <= MAX_CHANNELS and cin % CIN_STEP == 0 and MIN_COUT <= cout <= MAX_CHANNELS and cout % COUT_STEP == 0):
        raise ValueError(f"weight {tuple(weight.shape)}: a multiple of {COUT_STEP} in {MIN_COUT}..{MAX_CHANNELS} output and a multiple of "
                         f"{CIN_STEP} in {MIN_CIN}..{MAX_CHANNELS} input channels")
    _conv.check_bias(x, weight, bias)
    _conv.check_rows(x)
    if min(x.shape[2:]) + 2 * padding < k:
        raise ValueError(f"x {tuple(x.shape)}: every extent, padded by {padding} on both sides, must be at least the kernel's {k}")
    if x.size(0) > 65535:
        raise ValueError(f"x {tuple(x.shape)}: at most 65535 batch entries")
    out = out_extents(tuple(x.shape[2:]), k, padding)
    if x.size(0) * out[0] * out[1] * out[2] >= 2 ** 31:
        raise ValueError(f"x {tuple(x.shape)}: the patches of all batch entries must number fewer than 2^31")
    return _Patch.apply(x, weight, bias, int(padding), int(padding_mode == "zeros"), -1.0 if negative_slope is None else float(negative_slope),
                        int(split))


def patch_conv3d(x, weight, bias=None, padding=0, padding_mode="replicate", negative_slope=None):
    """act(F.conv3d(F.pad(x, (padding,) * 6, mode), weight, bias, stride=k)) for a weight [Cout, Cin, k, k, k], k 2..5, Cin a multiple of
    8 up to 256, Cout a multiple of 32 up to 256, and a bias [Cout] or None; x [B,Cin,D,H,W] fp32 on a HIP device; padding 0..k-1;
    padding_mode "replicate" or "zeros"; negative_slope None (no activation) or the leaky ReLU's slope >= 0."""
    return _patch_conv3d(x, weight, bias, padding, padding_mode, negative_slope)
