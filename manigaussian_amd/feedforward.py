"""What a Perceiver transformer block does beside its attention and its GEMMs (agents/manigaussian_bc/perceiver_lang_io.py:56-99:
PreNorm's nn.LayerNorm, FeedForward's Linear -> GEGLU -> Linear), fused (csrc/mgs_feedforward.hip).

    layer_norm(x, weight, bias, eps)   F.layer_norm over the last dimension: one launch forward; backward one launch for dx plus one
                                       for dweight / dbias (none when both are frozen).  Keeps x, weight and two floats per row.
    bias_geglu(h, bias)                a, gates = (h + bias).chunk(2, -1); a * F.gelu(gates): one launch forward; backward one launch
                                       that writes both halves of dh in place, plus one for dbias.  Keeps h and bias, nothing of
                                       gelu's size.

No atomics: the same bits from run to run; capturable into a HIP graph.  A float32 tensor on a HIP device within the kernels' limits
takes them; anything else (a CPU tensor, another dtype, a last dimension above 1024, a layer norm without weight or bias) takes
torch's own composition, so the drop-ins work wherever the reference's classes do.

`PreNorm`, `GEGLU` and `FeedForward` have the reference's constructors, sub-module names and initialisation: a reference state_dict
loads with strict=True and the other way round.  Which of the two ops a drop-in sends through the kernels follows the measured
medians (scripts/bench_feedforward.py): ROUTE below -- at present neither, see there.
"""
import functools

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib, _ops

MAX_D = 1024        # the widest layer norm row one wave holds
MAX_ELEMS = 2 ** 31 - 1

# Which ops the drop-in classes send through the kernels (the functions layer_norm / bias_geglu always do, for eligible tensors):
# an op stays on torch's side unless its measured median, forward AND forward + backward, is below torch's at every measured use.
# As measured (profiles/feedforward_bench.json) neither is yet: called one at a time, both ops are bound by the host's
# enqueue path, where this module's Python autograd functions cost more than torch's compiled ones, although the kernels take less
# device time.  layer_norm loses at both shapes; bias_geglu wins forward (23.5 against 35.0 us) and loses forward + backward
# (115 against 108 us).  So the drop-ins run torch's composition until the numbers say otherwise.
ROUTE = {"layer_norm": False, "bias_geglu": False}


def _by_rows(t, width, zero_ok=False):
    """(tensor, row stride in elements) of a [..., width] tensor read as [rows, width]: the tensor itself when its last dimension
    has unit stride and its leading dimensions collapse to one uniform row stride (at least the width, or 0 with zero_ok: one
    row expanded over all), else one contiguous copy."""
    if t.is_contiguous():
        return t, width
    lead = [(n, s) for n, s in zip(t.shape[:-1], t.stride()[:-1]) if n != 1]
    ok = width == 1 or t.stride(-1) == 1
    stride = width
    if ok and lead:
        stride = lead[-1][1]
        ok = all(s0 == s1 * n1 for (_, s0), (n1, s1) in zip(lead[:-1], lead[1:]))
        ok = ok and (stride >= width or (zero_ok and stride == 0))
    if not ok:
        return t.contiguous(), width
    return t, stride


@functools.lru_cache(maxsize=None)
def _workspace_bytes(cols):
    return _lib.lib().mgs_feedforward_workspace_bytes(1, cols)   # (64 slabs of two sums: the same for any number of rows)


def _workspace(dev, cols):
    # the slabs' partial column sums: written before they are read in every call
    return _ops.workspace(dev, _workspace_bytes(cols))


def _fp32(g):
    return g if g.dtype == torch.float32 else g.to(torch.float32)


class _LayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps, row_split):
        D = x.shape[-1]
        x, xs = _by_rows(x, D)
        weight, bias = weight.contiguous(), bias.contiguous()
        dev, rows = x.device, x.numel() // D
        y = torch.empty(x.shape, dtype=torch.float32, device=dev)
        stats = torch.empty(rows, 2, dtype=torch.float32, device=dev)
        _ops.call("mgs_layernorm_forward", dev, rows, D, x.data_ptr(), xs, weight.data_ptr(), bias.data_ptr(), eps, y.data_ptr(),
                  stats.data_ptr())
        ctx.save_for_backward(x, weight, stats)
        ctx.xs, ctx.row_split = xs, row_split
        return y

    @staticmethod
    def backward(ctx, g):
        x, weight, stats = ctx.saved_tensors
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        if not (need_x or need_w or need_b):
            return None, None, None, None, None
        D = x.shape[-1]
        dev, rows = x.device, x.numel() // D
        g, gs = _by_rows(_fp32(g), D, zero_ok=True)
        dx = torch.empty(x.shape, dtype=torch.float32, device=dev)
        dw = torch.empty(D, dtype=torch.float32, device=dev) if need_w else None
        db = torch.empty(D, dtype=torch.float32, device=dev) if need_b else None
        ws = _workspace(dev, D) if (need_w or need_b) else None
        _ops.call("mgs_layernorm_backward", dev, rows, D, x.data_ptr(), ctx.xs, weight.data_ptr(), stats.data_ptr(), g.data_ptr(), gs,
                  dx.data_ptr(), _ops.ptr(dw), _ops.ptr(db), _ops.ptr(ws), ws.numel() if ws is not None else 0, ctx.row_split)
        return (dx if need_x else None), dw, db, None, None


class _BiasGeglu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, bias, row_split):
        M = h.shape[-1] // 2
        h, hs = _by_rows(h, 2 * M)
        bias = None if bias is None else bias.contiguous()
        dev, rows = h.device, h.numel() // (2 * M)
        out = torch.empty(h.shape[:-1] + (M,), dtype=torch.float32, device=dev)
        _ops.call("mgs_bias_geglu_forward", dev, rows, M, h.data_ptr(), hs, _ops.ptr(bias), out.data_ptr())
        ctx.save_for_backward(h, bias)
        ctx.hs, ctx.row_split = hs, row_split
        return out

    @staticmethod
    def backward(ctx, g):
        h, bias = ctx.saved_tensors
        need_h, need_b = ctx.needs_input_grad[:2]
        if not (need_h or need_b):
            return None, None, None
        M = h.shape[-1] // 2
        dev, rows = h.device, h.numel() // (2 * M)
        g, gs = _by_rows(_fp32(g), M, zero_ok=True)
        dh = torch.empty(h.shape, dtype=torch.float32, device=dev)
        db = torch.empty(2 * M, dtype=torch.float32, device=dev) if (need_b and bias is not None) else None
        ws = _workspace(dev, M) if db is not None else None
        _ops.call("mgs_bias_geglu_backward", dev, rows, M, h.data_ptr(), ctx.hs, _ops.ptr(bias), g.data_ptr(), gs, dh.data_ptr(),
                  _ops.ptr(db), _ops.ptr(ws), ws.numel() if ws is not None else 0, ctx.row_split)
        return (dh if need_h else None), db, None


def _on_device_fp32(*tensors):
    return all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 for t in tensors)


def layer_norm(x, weight, bias, eps=1e-5, row_split=0):
    """F.layer_norm(x, x.shape[-1:], weight, bias, eps).  float32 on a HIP device with 1 <= x.shape[-1] <= 1024, weight and bias
    given: the fused kernels; anything else: torch's.  row_split: the number of slabs of the backward's column sums (0: the
    library's choice, 1..64: a test aid)."""
    D = x.shape[-1] if x.dim() else 0
    if (weight is None or bias is None or not _on_device_fp32(x, weight, bias) or not 1 <= D <= MAX_D
            or not 0 < x.numel() <= MAX_ELEMS or weight.shape != (D,) or bias.shape != (D,)):
        return F.layer_norm(x, (D,), weight, bias, eps)
    return _LayerNorm.apply(x, weight, bias, float(eps), int(row_split))


def geglu_composition(h, bias=None):
    """The op in torch's own calls: the reference's GEGLU.forward behind the bias add."""
    if bias is not None:
        h = h + bias
    a, gates = h.chunk(2, dim=-1)
    return a * F.gelu(gates)


def bias_geglu(h, bias=None, row_split=0):
    """a, gates = (h + bias).chunk(2, -1); a * F.gelu(gates)  (the exact, erf GELU), h [..., 2 M], bias [2 M] or None.  float32 on a
    HIP device: the fused kernels; anything else: torch's composition."""
    W = h.shape[-1] if h.dim() else 0
    tensors = (h,) if bias is None else (h, bias)
    if (not _on_device_fp32(*tensors) or W < 2 or W % 2 or not 0 < h.numel() <= MAX_ELEMS
            or (bias is not None and bias.shape != (W,))):
        return geglu_composition(h, bias)
    return _BiasGeglu.apply(h, bias, int(row_split))


def _norm(x, ln):
    """nn.LayerNorm `ln` applied to x: through layer_norm when the route and the module allow it."""
    if ROUTE["layer_norm"] and len(ln.normalized_shape) == 1:
        return layer_norm(x, ln.weight, ln.bias, ln.eps)
    return ln(x)


class PreNorm(nn.Module):
    """perceiver_lang_io.py:56's PreNorm; self.norm / self.norm_context hold the parameters as nn.LayerNorm."""

    def __init__(self, dim, fn, context_dim=None):
        super().__init__()
        self.fn = fn
        self.norm = nn.LayerNorm(dim)
        self.norm_context = nn.LayerNorm(context_dim) if context_dim is not None else None

    def _normed(self, x, kwargs):
        x = _norm(x, self.norm)
        if self.norm_context is not None:
            kwargs.update(context=_norm(kwargs["context"], self.norm_context))
        return x

    def forward(self, x, **kwargs):
        x = self._normed(x, kwargs)
        return self.fn(x, **kwargs)

    def get_attention_matrix(self, x, **kwargs):
        x = self._normed(x, kwargs)
        kwargs["return_attention_weights"] = True
        return self.fn(x, **kwargs)


class GEGLU(nn.Module):
    """perceiver_lang_io.py:83's GEGLU."""

    def forward(self, x):
        return bias_geglu(x, None) if ROUTE["bias_geglu"] else geglu_composition(x)


class FeedForward(nn.Module):
    """perceiver_lang_io.py:89's FeedForward: the first linear's bias is added inside the GEGLU, so its bias gradient comes out of
    the GEGLU's backward and the biased [rows, 2 M] tensor is never written."""

    def __init__(self, dim, mult=4):
        super().__init__()
        self.net = nn.Sequential(nn.Linear(dim, dim * mult * 2), GEGLU(), nn.Linear(dim * mult, dim))

    def forward(self, x):
        if not ROUTE["bias_geglu"]:
            return self.net(x)
        first, _, last = self.net
        return last(bias_geglu(F.linear(x, first.weight), first.bias))
