"""The photometric loss of Gaussian splatting, fused: L1 + L2 + D-SSIM on the rendered image, forward and backward.

Reference: agents/manigaussian_bc/loss.py:9-13 (l1_loss, l2_loss) and :25-68 (gaussian, create_window, ssim, _ssim: an 11 x 11
Gaussian window of sigma 1.5 with zero padding), conf/method/ManiGaussian_BC.yaml:97-98 (lambda_l1, lambda_ssim) and the
commented line of neural_rendering.py:299-307.  In torch that is five grouped conv2d calls and a dozen elementwise kernels
forward, and their backward.  Here: three launches forward, one backward, no host synchronisation, deterministic
(csrc/mgs_photometric.hip).  The forward already writes d loss / d color; the backward only scales it by the upstream gradient,
read on the device.
"""
import ctypes

import torch

from . import _lib, _ops
from .losses import _round4

MAX_C = 64
WINDOW_SIZE = 11
# loss.gaussian(11, 1.5) as float32, bit for bit (the library's MGS_SSIM_WINDOW; tests compare both with the reference's)
WINDOW = (0.001028380123898387, 0.0075987582094967365, 0.036000773310661316, 0.10936068743467331, 0.21300552785396576,
          0.26601171493530273, 0.21300552785396576, 0.10936068743467331, 0.036000773310661316, 0.0075987582094967365,
          0.001028380123898387)


def _images(t, name, fn):
    """[C,H,W] or [V,C,H,W] -> [V,C,H,W], contiguous (the rasterizer's outputs already are)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{fn}: {name} must be a tensor, got {type(t).__name__}")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{fn}: {name} must be float32, got {t.dtype}")
    if t.dim() not in (3, 4):
        raise RuntimeError(f"{fn}: {name} must be [C,H,W] or [V,C,H,W], got {tuple(t.shape)}")
    v = t if t.dim() == 4 else t.unsqueeze(0)
    if not 1 <= v.size(0) <= _lib.MAX_VIEWS:
        raise RuntimeError(f"{fn}: V = {v.size(0)} views (1 .. {_lib.MAX_VIEWS})")
    if not 1 <= v.size(1) <= MAX_C:
        raise RuntimeError(f"{fn}: C = {v.size(1)} channels (1 .. {MAX_C})")
    if v.size(2) < 1 or v.size(3) < 1:
        raise RuntimeError(f"{fn}: {name} {tuple(t.shape)} is empty")
    return v.contiguous()


def _target(t, name, fn, V, C, H, W, channel_first=False):
    """A constant target, channel-first [V,C,H,W] or (unless channel_first) channel-last [V,H,W,C]; V = 1: the leading
    dimension may be missing.  Returns the element strides (view, channel, row, column) of the tensor itself, never a copy."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{fn}: {name} must be a tensor, got {type(t).__name__}")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{fn}: {name} must be float32, got {t.dtype}")
    if t.requires_grad:
        raise RuntimeError(f"{fn}: {name} is a target (a constant) and must not require grad; detach it")
    shape, st = tuple(t.shape), tuple(t.stride())
    if t.dim() == 3:
        if V != 1:
            raise RuntimeError(f"{fn}: {name} {shape} has no view dimension, the rendered images have V = {V}")
        shape, st = (1,) + shape, (0,) + st
    forms = f"[{V},{C},{H},{W}]" if channel_first else f"[{V},{H},{W},{C}] or [{V},{C},{H},{W}]"
    if len(shape) != 4:
        raise RuntimeError(f"{fn}: {name} must be {forms}, got {tuple(t.shape)}")
    if shape[0] != V and (shape[1:] == (C, H, W) or (not channel_first and shape[1:] == (H, W, C))):
        raise RuntimeError(f"{fn}: {name} holds {shape[0]} views, the rendered images V = {V}")
    if shape == (V, C, H, W):
        return st
    if not channel_first and shape == (V, H, W, C):
        return (st[0], st[3], st[1], st[2])
    raise RuntimeError(f"{fn}: {name} must be {forms}, got {tuple(t.shape)}")


def _weights(weights, V, dev, fn):
    """-> (host floats [3V] or None, device tensor [V,3] or None)"""
    if weights is None:
        return [1.0] * (3 * V), None
    if isinstance(weights, torch.Tensor):
        if tuple(weights.shape) != (V, 3):
            raise RuntimeError(f"{fn}: weights must be [V,3] = [{V},3], got {tuple(weights.shape)}")
        if not weights.is_cuda:
            return [float(x) for x in weights.reshape(-1).tolist()], None
        if weights.dtype != torch.float32 or weights.device != dev or not weights.is_contiguous():
            raise RuntimeError(f"{fn}: device weights must be a contiguous float32 [V,3] tensor on the images' device")
        if weights.requires_grad:
            raise RuntimeError(f"{fn}: weights are constants and must not require grad")
        return None, weights
    rows = [tuple(r) for r in weights]
    if len(rows) != V or any(len(r) != 3 for r in rows):
        raise RuntimeError(f"{fn}: weights must be {V} triples (w_l1, w_l2, w_ssim), one per view; got {weights!r}")
    return [float(x) for r in rows for x in r], None


class _Photometric(torch.autograd.Function):
    """per_view False: -> (loss, terms [V,4]); True: -> (ssim [V], None), differentiable per view (the caller passes the
    weights (0, 0, -1), so the unit gradient of view v is d ssim[v] / d color[v])."""

    @staticmethod
    def forward(ctx, color, target, strides, w_host, w_dev, per_view):
        L = _lib.lib()
        dev = color.device
        V, C, H, W = color.shape
        need = ctx.needs_input_grad[0]
        # one allocation: unit gradient | workspace | terms | loss
        n_u = _round4(V * C * H * W) if need else 0
        ws_bytes = L.mgs_photometric_workspace_bytes(V, C, W, H)
        n_ws = _round4((ws_bytes + 3) // 4)
        buf = torch.empty(n_u + n_ws + 4 * V + 1, dtype=torch.float32, device=dev)
        unit = buf[:n_u] if need else None
        ws = buf[n_u:n_u + n_ws]
        terms = buf[n_u + n_ws:n_u + n_ws + 4 * V].view(V, 4)
        loss = buf[n_u + n_ws + 4 * V:].view(())
        wh = (ctypes.c_float * (3 * V))(*w_host) if w_host is not None else None
        _ops.call("mgs_photometric_forward", dev, V, C, W, H, color.data_ptr(), target.data_ptr(),
                  (ctypes.c_int64 * 4)(*strides), wh, _ops.ptr(w_dev), _ops.ptr(unit), terms.data_ptr(), loss.data_ptr(),
                  ws.data_ptr(), ws_bytes)
        ctx.unit = unit
        ctx.shape = (V, C, W, H)
        ctx.per_view = per_view
        ctx.set_materialize_grads(False)
        if per_view:
            return terms[:, 2], None
        ctx.mark_non_differentiable(terms)
        return loss, terms

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _g_terms):
        if g is None or ctx.unit is None:
            return (None,) * 6
        V, C, W, H = ctx.shape
        dev = g.device
        g_up = g if g.dtype == torch.float32 else g.float()
        if ctx.per_view:
            g_up = g_up.contiguous()
        out = torch.empty((V, C, H, W), dtype=torch.float32, device=dev)
        _ops.call("mgs_photometric_backward", dev, V, C, W, H, g_up.data_ptr(), 1 if ctx.per_view else 0,
                  ctx.unit.data_ptr(), out.data_ptr())
        return (out,) + (None,) * 5


def _apply(fn, name, color, target, weights, per_view, channel_first):
    """weights: as photometric_loss takes them, or a function of the view count."""
    c = _images(color, name, fn)
    V, C, H, W = c.shape
    strides = _target(target, "target", fn, V, C, H, W, channel_first)
    w_host, w_dev = _weights(weights(V) if callable(weights) else weights, V, c.device, fn)
    # (shapes first, devices last: a wrong shape is reported as such wherever the tensors live)
    for what, t in ((name, c), ("target", target)):
        if not t.is_cuda:
            raise RuntimeError(f"{fn} needs tensors on a HIP device; there is no CPU path ({what} is on {t.device})")
        if t.device != c.device:
            raise RuntimeError(f"{fn}: {what} is on {t.device}, {name} on {c.device}")
    return _Photometric.apply(c, target, strides, w_host, w_dev, per_view)


def _window(window_size, fn):
    if window_size != WINDOW_SIZE:
        raise RuntimeError(f"{fn}: window_size = {window_size} is not implemented (the fused kernels hold loss.py's default "
                           f"window: {WINDOW_SIZE} taps, sigma 1.5)")


def photometric_loss(color, target, *, weights=None, window_size=WINDOW_SIZE):
    """L1 + L2 + D-SSIM between rendered images and their targets for V views in one fused pass -> (loss, terms).

    color [V,C,H,W] (C <= 64; [C,H,W] for one view) is the rasterizer's output; target is a constant, channel-last [V,H,W,C]
    or channel-first [V,C,H,W], read through its strides without a copy.
      loss  = 0 + sum_v (w_l1[v] * l1[v] + w_l2[v] * l2[v] + w_ssim[v] * (1 - ssim[v])), a 0-dim tensor with a grad_fn;
              l1 = mean |x - y|, l2 = mean (x - y)^2, ssim = loss.py's ssim(x, y) (11 x 11 window, sigma 1.5, zero padding).
      terms = {"l1": [V], "l2": [V], "ssim": [V], "psnr": [V]}: detached device tensors; nothing is read back to the host
              (PSNR = 20 log10(1 / sqrt(l2)), 100 where l2 is exactly 0, decided on the device).
    weights: None (all ones), V triples (w_l1, w_l2, w_ssim) of Python floats (passed by value: a captured HIP graph keeps the
    values it was captured with), or a float32 device tensor [V,3] (read by the kernels: a captured graph follows in-place
    updates).  A zero weight still reports its term and gives an exactly zero gradient share.
    The standard splatting loss (1 - lambda) L1 + lambda D-SSIM is weights=[(1 - lam, 0, lam)] per view.
    Only color receives a gradient.  float32, HIP tensors only; window_size other than 11 is refused."""
    _window(window_size, "photometric_loss")
    loss, terms = _apply("photometric_loss", "color", color, target, weights, False, False)
    return loss, {"l1": terms[:, 0], "l2": terms[:, 1], "ssim": terms[:, 2], "psnr": terms[:, 3]}


def ssim(img1, img2, window_size=WINDOW_SIZE, size_average=True):
    """Drop-in for loss.py's ssim on channel-first images [V,C,H,W] (or [C,H,W]): differentiable with respect to img1, img2
    is a constant.  size_average=False returns the [V] per-image means."""
    _window(window_size, "ssim")
    per_view, _ = _apply("ssim", "img1", img1, img2, lambda V: [(0.0, 0.0, -1.0)] * V, True, True)
    return per_view.mean() if size_average else per_view  # (the mean over the views and its backward are torch's)


def l1_loss(network_output, gt):
    """loss.py's l1_loss (mean |network_output - gt| over everything) through the fused pass; gt is a constant."""
    loss, _ = _apply("l1_loss", "network_output", network_output, gt, lambda V: [(1.0 / V, 0.0, 0.0)] * V, False, False)
    return loss
