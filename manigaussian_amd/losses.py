"""ManiGaussian's rendering losses, fused: the block between the rasterizer's forward and its backward.

Reference: agents/manigaussian_bc/neural_rendering.py:299-329 (l2 on the rendered colour, PSNR, the embedding loss, l2 on the
next frame's colour, the weighted sum), :90-106 (_embed_loss_fn: cosine / l2 / l2_norm), :22-27 (PSNR_torch) and loss.py:12-23.
There it is a few dozen small torch kernels forward + backward, and PSNR_torch's `if mse == 0` reads the device in every
step.  Here: two launches forward (three for "l2_norm"), one backward, no host synchronisation, deterministic (csrc/mgs_loss.hip).
The forward already writes d loss / d image; the backward only scales it by the upstream gradient, read on the device.
"""
import ctypes

import torch

from . import _lib, _ops

EMBED_FNS = {"cosine": 0, "l2": 1, "l2_norm": 2}
MAX_F = 64


def _images(t, name, channels=None):
    """[C,H,W] or [V,C,H,W] -> [V,C,H,W], contiguous (the rasterizer's outputs already are)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"rendering_loss: {name} must be a tensor, got {type(t).__name__}")
    if t.dtype != torch.float32:
        raise RuntimeError(f"rendering_loss: {name} must be float32, got {t.dtype}")
    if t.dim() not in (3, 4):
        raise RuntimeError(f"rendering_loss: {name} must be [C,H,W] or [V,C,H,W], got {tuple(t.shape)}")
    v = t if t.dim() == 4 else t.unsqueeze(0)
    if channels is not None and v.size(1) != channels:
        raise RuntimeError(f"rendering_loss: {name} must have {channels} channels ([V,{channels},H,W]), got {tuple(t.shape)}")
    return v.contiguous()


def _target(t, name, V, C, H, W):
    """A constant target, channel-last [V,H,W,C] or channel-first [V,C,H,W] (V = 1: the leading dimension may be missing):
    returns (tensor, element strides (view, channel, row, column)) -- the tensor itself, never a copy."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"rendering_loss: {name} must be a tensor, got {type(t).__name__}")
    if t.dtype != torch.float32:
        raise RuntimeError(f"rendering_loss: {name} must be float32, got {t.dtype}")
    if t.requires_grad:
        raise RuntimeError(f"rendering_loss: {name} is a target (a constant) and must not require grad; detach it")
    shape, st = tuple(t.shape), t.stride()
    if t.dim() == 3:
        if V != 1:
            raise RuntimeError(f"rendering_loss: {name} {shape} has no view dimension, the rendered images have V = {V}")
        shape, st = (1,) + shape, (0,) + tuple(st)
    if len(shape) != 4:
        raise RuntimeError(f"rendering_loss: {name} must be [V,H,W,{C}] or [V,{C},H,W], got {tuple(t.shape)}")
    if shape[0] != V and shape[1:] in ((C, H, W), (H, W, C)):
        raise RuntimeError(f"rendering_loss: {name} holds {shape[0]} views, the rendered images V = {V}")
    if shape == (V, C, H, W):
        return t, (st[0], st[1], st[2], st[3])
    if shape == (V, H, W, C):
        return t, (st[0], st[3], st[1], st[2])
    raise RuntimeError(f"rendering_loss: {name} must be [{V},{H},{W},{C}] or [{V},{C},{H},{W}], got {tuple(t.shape)}")


_ZERO = {}


def _zero(dev):
    """The constant 0 of a device (loss_reg, and loss_dyna of a static step): made once, not once per step."""
    z = _ZERO.get(dev)
    if z is None:
        z = _ZERO[dev] = torch.zeros((), dtype=torch.float32, device=dev)
    return z


def _round4(n):
    return (n + 3) & ~3


class _RenderingLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, color, feature, gt_rgb, rgb_st, gt_embed, emb_st, embed_fn, w_host, w_dev):
        L = _lib.lib()
        dev = color.device
        V, _, H, W = color.shape
        N = H * W
        has_embed = feature is not None
        F = feature.size(1) if has_embed else 0
        need_c = ctx.needs_input_grad[0]
        need_f = has_embed and ctx.needs_input_grad[1]
        # one allocation: unit gradients | workspace | terms | loss
        n_c, n_f = _round4(V * 3 * N), _round4(V * F * N)
        ws_bytes = L.mgs_render_loss_workspace_bytes(V, W, H)
        n_ws = _round4((ws_bytes + 3) // 4)
        buf = torch.empty(n_c + n_f + n_ws + 3 * V + 1, dtype=torch.float32, device=dev)
        g_color, g_feature = buf[:n_c], buf[n_c:n_c + n_f]
        ws = buf[n_c + n_f:n_c + n_f + n_ws]
        terms = buf[n_c + n_f + n_ws:n_c + n_f + n_ws + 3 * V].view(V, 3)
        loss = buf[n_c + n_f + n_ws + 3 * V:].view(())
        i64x4 = ctypes.c_int64 * 4
        wh = (ctypes.c_float * (2 * V))(*w_host) if w_host is not None else None
        _ops.call("mgs_render_loss_forward", dev,
                  V, F, W, H, color.data_ptr(), gt_rgb.data_ptr(), i64x4(*rgb_st),
                  feature.data_ptr() if has_embed else None, gt_embed.data_ptr() if has_embed else None,
                  i64x4(*emb_st) if has_embed else None, embed_fn, wh, _ops.ptr(w_dev),
                  g_color.data_ptr() if need_c else None, g_feature.data_ptr() if need_f else None, terms.data_ptr(),
                  loss.data_ptr(), ws.data_ptr(), ws_bytes)
        ctx.unit = (g_color if need_c else None, g_feature if need_f else None)
        ctx.shape = (V, F, W, H)
        ctx.mark_non_differentiable(terms)
        ctx.set_materialize_grads(False)
        return loss, terms

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss, _g_terms):
        if g_loss is None:
            return (None,) * 9
        V, F, W, H = ctx.shape
        unit_c, unit_f = ctx.unit
        dev = g_loss.device
        g_up = g_loss if g_loss.dtype == torch.float32 else g_loss.float()
        out_c = torch.empty((V, 3, H, W), dtype=torch.float32, device=dev) if unit_c is not None else None
        out_f = torch.empty((V, F, H, W), dtype=torch.float32, device=dev) if unit_f is not None else None
        if out_c is not None or out_f is not None:
            p = _ops.ptr
            _ops.call("mgs_render_loss_backward", dev, V, F, W, H, g_up.data_ptr(), p(unit_c), p(unit_f), p(out_c), p(out_f))
        return (out_c, out_f) + (None,) * 7


def _weights(weights, V, dev):
    """-> (host floats [2V] or None, device tensor [V,2] or None)"""
    if weights is None:
        return [1.0] * (2 * V), None
    if isinstance(weights, torch.Tensor):
        if tuple(weights.shape) != (V, 2):
            raise RuntimeError(f"rendering_loss: weights must be [V,2] = [{V},2], got {tuple(weights.shape)}")
        if not weights.is_cuda:
            return [float(x) for x in weights.reshape(-1).tolist()], None
        if weights.dtype != torch.float32 or weights.device != dev or not weights.is_contiguous():
            raise RuntimeError("rendering_loss: device weights must be a contiguous float32 [V,2] tensor on the images' device")
        if weights.requires_grad:
            raise RuntimeError("rendering_loss: weights are constants and must not require grad")
        return None, weights
    rows = [tuple(r) for r in weights]
    if len(rows) != V or any(len(r) != 2 for r in rows):
        raise RuntimeError(f"rendering_loss: weights must be {V} pairs (w_rgb, w_embed), one per view; got {weights!r}")
    return [float(x) for r in rows for x in r], None


def rendering_loss(color, gt_rgb, feature=None, gt_embed=None, *, weights=None, embed_loss_fn="cosine"):
    """ManiGaussian's rendering losses for V views in one fused pass -> (loss, terms).

    color [V,3,H,W] and feature [V,F,H,W] (F <= 64) are the rasterizer's outputs ([3,H,W] / [F,H,W] for one view); gt_rgb and
    gt_embed are constants, channel-last [V,H,W,C] or channel-first [V,C,H,W], read through their strides without a copy.
      loss  = 0 + sum_v (w_rgb[v] * l2(color[v], gt_rgb[v]) + w_embed[v] * embed_loss(feature[v], gt_embed[v])), a 0-dim
              tensor with a grad_fn; embed_loss is "cosine" (1 - mean cosine similarity, torch's F.cosine_similarity
              including its gradient at zero-norm pixels), "l2" or "l2_norm"; 0 without feature / gt_embed.
      terms = {"loss_rgb": [V], "loss_embed": [V], "psnr": [V]}: detached device tensors; nothing is read back to the host,
              `.item()` is the caller's choice (PSNR is 100 where the mse is exactly 0, decided on the device).
    weights: None (all ones), V pairs of Python floats (passed by value: a captured HIP graph keeps the values it was captured
    with), or a float32 device tensor [V,2] (read by the kernels: a captured graph follows in-place updates, e.g. lambda_dyna
    switching on after the warm-up).  A zero weight still reports its term and gives an exactly zero gradient.
    Only the inputs that require grad receive a gradient.  float32, HIP tensors only."""
    if embed_loss_fn not in EMBED_FNS:
        raise RuntimeError(f"rendering_loss: embed_loss_fn {embed_loss_fn!r} is not implemented (one of {sorted(EMBED_FNS)})")
    c = _images(color, "color", 3)
    V, _, H, W = c.shape
    t_rgb, rgb_st = _target(gt_rgb, "gt_rgb", V, 3, H, W)
    f = t_emb = emb_st = None
    if feature is not None and gt_embed is not None:
        f = _images(feature, "feature")
        if f.size(0) != V or tuple(f.shape[2:]) != (H, W):
            raise RuntimeError(f"rendering_loss: feature {tuple(feature.shape)} does not match color {tuple(color.shape)} "
                               "in views or image size")
        if not 1 <= f.size(1) <= MAX_F:
            raise RuntimeError(f"rendering_loss: F = {f.size(1)} feature channels (1 .. {MAX_F})")
        t_emb, emb_st = _target(gt_embed, "gt_embed", V, f.size(1), H, W)
    # (shapes first, devices last: a wrong shape is reported as such wherever the tensors live)
    for name, t in (("color", c), ("gt_rgb", t_rgb), ("feature", f), ("gt_embed", t_emb)):
        if t is not None and not t.is_cuda:
            raise RuntimeError(f"rendering_loss needs tensors on a HIP device; there is no CPU path ({name} is on {t.device})")
        if t is not None and t.device != c.device:
            raise RuntimeError(f"rendering_loss: {name} is on {t.device}, color on {c.device}")
    w_host, w_dev = _weights(weights, V, c.device)
    loss, terms = _RenderingLoss.apply(c, f, t_rgb, rgb_st, t_emb, emb_st, EMBED_FNS[embed_loss_fn], w_host, w_dev)
    return loss, {"loss_rgb": terms[:, 0], "loss_embed": terms[:, 1], "psnr": terms[:, 2]}


def manigaussian_losses(cur, nxt, gt_rgb, gt_embed, next_gt_rgb, *, lambda_embed, lambda_dyna, embed_loss_fn="cosine",
                        stacked=None, weights=None):
    """The loss block of NeuralRenderer.forward (neural_rendering.py:299-352) -> (loss, loss_dict).

    cur / nxt: what render() returned for the current frame and for the deformed next frame ("render", "render_embed");
    nxt = None is the static step.  loss = l2(rgb) + lambda_embed * embed_loss + lambda_dyna * l2(next rgb), in the reference's
    order; pass lambda_dyna = 0 before the warm-up (the term is still reported).  gt_embed = None: no embedding term.
    loss_dict has the reference's keys (loss_rgb, loss_embed, loss_dyna, loss_reg, l1, psnr) as DEVICE scalars: the reference
    calls .item() on each, six host synchronisations per step; here that is the caller's choice.

    stacked: the batch dict of render_sets_stacked() (row 0 the current frame, row 1 the next one).  Both frames then go
    through ONE fused pass on the batch tensors, and autograd hands the batch gradient straight to the set-batch backward (a
    loss on the per-view slices would rebuild it with zero-fills and adds).  gt_rgb may then already be the [2,H,W,3] stack of
    both targets (next_gt_rgb = None), which saves the torch.stack here.
    weights: optional float32 device tensor [2,2] = [[1, lambda_embed], [lambda_dyna, 0]] replacing the two lambdas (a captured
    graph follows in-place updates of it); stacked form only."""
    dyn = nxt is not None or (stacked is not None and stacked["render"].size(0) == 2)
    if stacked is not None:
        color, feat = stacked["render"], stacked["render_embed"]
        V = color.size(0)
        if V not in (1, 2):
            raise RuntimeError(f"manigaussian_losses: the stacked batch holds {V} views (the current frame and, optionally, the next)")
        if gt_embed is None or feat.dim() != 4:
            feat = None
        if V == 2:
            if next_gt_rgb is not None:
                a = gt_rgb if gt_rgb.dim() == 3 else gt_rgb[0]
                b = next_gt_rgb if next_gt_rgb.dim() == 3 else next_gt_rgb[0]
                gt = torch.stack([a, b])
            else:
                gt = gt_rgb
            ge = None
            if feat is not None:  # the next frame has no embedding term: weight 0 on the current frame's target (view stride 0)
                e1 = gt_embed if gt_embed.dim() == 4 else gt_embed.unsqueeze(0)
                ge = e1.expand(2, *e1.shape[1:])
            w = weights if weights is not None else [(1.0, float(lambda_embed)), (float(lambda_dyna), 0.0)]
        else:
            gt, ge = gt_rgb, gt_embed if feat is not None else None
            w = weights if weights is not None else [(1.0, float(lambda_embed))]
        loss, t = rendering_loss(color, gt, feat, ge, weights=w, embed_loss_fn=embed_loss_fn)
        l_rgb, l_emb, psnr = t["loss_rgb"][0], t["loss_embed"][0], t["psnr"][0]
        l_dyna = t["loss_rgb"][1] if V == 2 else None
    else:
        if weights is not None:
            raise RuntimeError("manigaussian_losses: device weights need the stacked form")
        feat = cur.get("render_embed") if gt_embed is not None else None
        if feat is not None and feat.dim() < 3:  # render() without language features returns a [1] placeholder
            feat = None
        loss, t = rendering_loss(cur["render"], gt_rgb, feat, gt_embed if feat is not None else None,
                                 weights=[(1.0, float(lambda_embed))], embed_loss_fn=embed_loss_fn)
        l_rgb, l_emb, psnr = t["loss_rgb"][0], t["loss_embed"][0], t["psnr"][0]
        l_dyna = None
        if dyn:
            if next_gt_rgb is None:
                raise RuntimeError("manigaussian_losses: a next frame without next_gt_rgb")
            loss_n, tn = rendering_loss(nxt["render"], next_gt_rgb, weights=[(float(lambda_dyna), 0.0)])
            loss = loss + loss_n
            l_dyna = tn["loss_rgb"][0]
    zero = _zero(loss.device)
    return loss, {"loss": loss, "loss_rgb": l_rgb, "loss_embed": l_emb, "loss_dyna": zero if l_dyna is None else l_dyna,
                  "loss_reg": zero, "l1": l_rgb, "psnr": psnr}
