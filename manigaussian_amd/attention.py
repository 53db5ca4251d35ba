"""The Perceiver's attention (agents/manigaussian_bc/perceiver_lang_io.py:102-145, class Attention), fused.

`Attention` has the reference's constructor, parameter names (to_q.weight, to_kv.weight, to_out.weight, to_out.bias) and
forward; a reference state_dict loads with strict=True and the other way round.  The three linear layers stay torch GEMMs;
what lies between them -- rearrange, q k^T * scale, key mask at -finfo.max, softmax, dropout, . v, rearrange back -- is one
HIP kernel forward and three backward (csrc/mgs_attention.hip): fp32 throughout, nothing of size Nq x Nk is ever stored, q, k
and v are read where the linear layers left them (k and v as the halves of the to_kv output, by stride), and the backward
hands to_kv ONE contiguous gradient.  Deterministic (no atomics) and capturable.

Dropout draws from the library's own counter-based stream (DESIGN.md "Attention": Philox4x32-10 of (seed, offset, b H + h, i,
j)), not from torch's generator: the same seed gives other masks than the reference's run, as any two dropout
implementations do.  Seed and offset live in a device buffer of the module (`rng_state`, int64 [2], not in state_dict()); every
training forward with dropout advances the offset by an in-place device add, so a replayed graph draws a fresh mask.

There is no CPU path.
"""
import ctypes

import torch
from torch import nn

from . import _lib, _ops

DIM_HEAD = 64  # the only head dimension the library compiles


def _copy(t):
    """A freshly allocated row-major copy (`.contiguous()` would hand back a tensor whose size-1 dimensions carry odd strides)."""
    return t.clone(memory_format=torch.contiguous_format)


def _by_stride(t):
    """The tensor itself when the library reads it in place -- what attn_check_qkv and bad_stride of mgs_attention.hip accept:
    unit-stride last dimension, 16-byte aligned base, row stride at least the row, row and batch strides multiples of 4 floats
    (a batch stride of 0, an `expand` over the batch, is one) -- else a row-major copy.  The halves of a to_kv output, a
    16-byte aligned column slice and every nn.Linear output are read in place; a column slice at an odd offset, a buffer of odd
    width and a row-expanded gradient (what `out.sum(1)` sends back) are copied."""
    sb, sn, s1 = t.stride()
    if s1 == 1 and t.data_ptr() % 16 == 0 and sn >= t.size(2) and sn % 4 == 0 and sb >= 0 and sb % 4 == 0:
        return t
    return _copy(t)


def _fill(a, q, k, v, heads, mask, dropout_p, rng):
    a.B, a.Nq, a.H, a.Nk, a.D = q.size(0), q.size(1), heads, k.size(1), q.size(2) // heads
    a.dropout_p = dropout_p
    a.q, a.k, a.v = q.data_ptr(), k.data_ptr(), v.data_ptr()
    a.q_stride_b, a.q_stride_n = q.stride(0), q.stride(1)
    a.k_stride_b, a.k_stride_n = k.stride(0), k.stride(1)
    a.v_stride_b, a.v_stride_n = v.stride(0), v.stride(1)
    if mask is not None:
        a.mask, a.mask_stride_b = mask.data_ptr(), mask.stride(0)
    a.rng_state = rng.data_ptr() if rng is not None else None


class _FusedAttention(torch.autograd.Function):
    """inputs (q, kv, None, None): k and v are the halves of kv [B,Nk,2 H 64] and kv gets one gradient;
    inputs (q, None, k, v): k and v are tensors of their own."""

    @staticmethod
    def forward(ctx, q, kv, k, v, heads, mask, dropout_p, rng):
        packed = kv is not None
        if packed:
            kv = _by_stride(kv)
            k, v = kv.chunk(2, dim=-1)
        else:
            k, v = _by_stride(k), _by_stride(v)
        q = _by_stride(q)
        dev = q.device
        B, Nq, HD = q.shape
        out = torch.empty(B, Nq, HD, dtype=torch.float32, device=dev)
        lse = torch.empty(B, heads, Nq, dtype=torch.float32, device=dev)
        a = _lib.MgsAttentionArgs()
        _fill(a, q, k, v, heads, mask, dropout_p, rng)
        a.out_stride_b, a.out_stride_n = out.stride(0), out.stride(1)
        _ops.call("mgs_attention_forward", dev, ctypes.byref(a), out.data_ptr(), lse.data_ptr())
        ctx.save_for_backward(q, kv if packed else k, v if not packed else None, mask, rng, out, lse)
        ctx.packed, ctx.heads, ctx.dropout_p = packed, heads, dropout_p
        return out

    @staticmethod
    def backward(ctx, d_out):
        q, kk, v, mask, rng, out, lse = ctx.saved_tensors
        k, v = kk.chunk(2, dim=-1) if ctx.packed else (kk, v)
        d_out = _by_stride(d_out)
        dev = q.device
        B, Nq, HD = q.shape
        Nk = k.size(1)
        dq = torch.empty(B, Nq, HD, dtype=torch.float32, device=dev)
        dkv = torch.empty(B, Nk, 2 * HD, dtype=torch.float32, device=dev)
        # D_i of the backward: written before it is read in every call
        ws = _ops.workspace(dev, _lib.lib().mgs_attention_workspace_bytes(B, ctx.heads, Nq, Nk))
        a = _lib.MgsAttentionArgs()
        _fill(a, q, k, v, ctx.heads, mask, ctx.dropout_p, rng)
        a.out_stride_b, a.out_stride_n = out.stride(0), out.stride(1)
        a.dout_stride_b, a.dout_stride_n = d_out.stride(0), d_out.stride(1)
        a.dq_stride_b, a.dq_stride_n = dq.stride(0), dq.stride(1)
        a.dkv_stride_b, a.dkv_stride_n = dkv.stride(0), dkv.stride(1)
        _ops.call("mgs_attention_backward", dev, ctypes.byref(a), out.data_ptr(), lse.data_ptr(), d_out.data_ptr(),
                  dq.data_ptr(), dkv.data_ptr(), ws.data_ptr(), ws.numel())
        if ctx.packed:
            return dq, dkv, None, None, None, None, None, None
        dk, dv = dkv.chunk(2, dim=-1)
        return dq, None, dk, dv, None, None, None, None


def _check(q, k, v, heads, mask, dropout_p, rng_state):
    for name, t in (("q", q), ("k", k), ("v", v)):
        if not t.is_cuda or t.dtype != torch.float32:
            raise RuntimeError(f"fused_attention needs float32 tensors on a HIP device ({name} is {t.dtype} on {t.device}); "
                               "there is no CPU path")
    heads = int(heads)
    if q.dim() != 3 or k.dim() != 3 or v.dim() != 3 or heads < 1:
        raise ValueError(f"expected q [B,Nq,H*64], k and v [B,Nk,H*64], got {tuple(q.shape)}, {tuple(k.shape)}, {tuple(v.shape)}")
    if q.size(2) != heads * DIM_HEAD or k.size(2) != q.size(2) or v.size(2) != q.size(2):
        raise ValueError(f"width mismatch: q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)} for {heads} heads of "
                         f"{DIM_HEAD} (the only head dimension compiled)")
    if k.size(0) != q.size(0) or v.shape != k.shape:
        raise ValueError(f"batch or length mismatch: q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)}")
    if q.size(1) < 1 or k.size(1) < 1:
        raise ValueError(f"empty sequence: q {tuple(q.shape)}, k {tuple(k.shape)}")
    if not 0.0 <= float(dropout_p) < 1.0:
        raise ValueError(f"dropout_p = {dropout_p} outside [0, 1)")
    if mask is not None:
        mask = mask.reshape(mask.size(0), -1)
        if mask.shape != (q.size(0), k.size(1)) or mask.device != q.device:
            raise ValueError(f"mask {tuple(mask.shape)} on {mask.device} for keys {tuple(k.shape)} on {q.device}")
        mask = mask.to(torch.uint8) if mask.dtype == torch.bool else (mask != 0).to(torch.uint8)
        mask = mask.contiguous()
    if float(dropout_p) > 0.0:
        if rng_state is None or rng_state.dtype != torch.int64 or rng_state.numel() != 2 or rng_state.device != q.device \
                or not rng_state.is_contiguous():
            raise ValueError("dropout_p > 0 needs rng_state: a contiguous int64 tensor (seed, offset) on the device of q")
    else:
        rng_state = None
    return heads, mask, float(dropout_p), rng_state


def fused_attention(q, k, v, heads, mask=None, dropout_p=0.0, rng_state=None):
    """q [B,Nq,H*64], k and v [B,Nk,H*64] (any layout: read in place where the library can, e.g. the chunk views of a to_kv output,
    copied otherwise, see _by_stride), mask [B,Nk] or [B,1,Nk] of any type (False / 0: the key's score is -finfo.max)
    -> [B,Nq,H*64].  rng_state: int64 device tensor (seed, offset), read by the kernels."""
    heads, mask, dropout_p, rng_state = _check(q, k, v, heads, mask, dropout_p, rng_state)
    return _FusedAttention.apply(q, None, k, v, heads, mask, dropout_p, rng_state)


def fused_attention_kv(q, kv, heads, mask=None, dropout_p=0.0, rng_state=None):
    """The same with k and v as the two halves of kv [B,Nk,2*H*64]; kv receives one contiguous gradient."""
    if kv.dim() != 3 or kv.size(2) % 2:
        raise ValueError(f"expected kv [B,Nk,2*H*64], got {tuple(kv.shape)}")
    k, v = kv.chunk(2, dim=-1)
    heads, mask, dropout_p, rng_state = _check(q, k, v, heads, mask, dropout_p, rng_state)
    return _FusedAttention.apply(q, kv, None, None, heads, mask, dropout_p, rng_state)


def dropout_keep_mask(B, heads, Nq, Nk, dropout_p, rng_state):
    """The keep decisions the kernels take for this (seed, offset): uint8 [B*heads, Nq, Nk] (a test and debug aid)."""
    dev = rng_state.device
    keep = torch.empty(B * heads, Nq, Nk, dtype=torch.uint8, device=dev)
    a = _lib.MgsAttentionArgs()
    a.B, a.H, a.Nq, a.Nk, a.D, a.dropout_p = B, heads, Nq, Nk, DIM_HEAD, float(dropout_p)
    a.rng_state = rng_state.data_ptr()
    _ops.call("mgs_attention_dropout_mask", dev, ctypes.byref(a), keep.data_ptr())
    return keep


def _as_int64(v):
    v = int(v) & 0xFFFFFFFFFFFFFFFF
    return v - (1 << 64) if v >= (1 << 63) else v


class Attention(nn.Module):
    """perceiver_lang_io.py:102's Attention.  dim_head must be 64."""

    def __init__(self, query_dim, context_dim=None, heads=8, dim_head=64, dropout=0.0):
        super().__init__()
        if dim_head != DIM_HEAD:
            raise ValueError(f"dim_head = {dim_head}: only {DIM_HEAD} is compiled")
        if not 0.0 <= float(dropout) < 1.0:
            raise ValueError(f"dropout = {dropout} outside [0, 1)")
        inner_dim = dim_head * heads
        context_dim = query_dim if context_dim is None else context_dim
        self.scale = dim_head ** -0.5
        self.heads = heads
        self.to_q = nn.Linear(query_dim, inner_dim, bias=False)
        self.to_kv = nn.Linear(context_dim, inner_dim * 2, bias=False)
        self.to_out = nn.Linear(inner_dim, query_dim)
        self.dropout_p = float(dropout)
        self.register_buffer("rng_state", torch.zeros(2, dtype=torch.int64), persistent=False)
        self._seeded = False

    def manual_seed(self, seed, offset=0):
        """Restart the module's dropout stream at (seed, offset)."""
        self.rng_state.copy_(torch.tensor([_as_int64(seed), _as_int64(offset)], dtype=torch.int64))
        self._seeded = True
        return self

    def forward(self, x, context=None, mask=None, return_attention_weights=False):
        context = x if context is None else context
        for name, t in (("x", x), ("context", context)):
            if not t.is_cuda or t.dtype != torch.float32:
                raise RuntimeError(f"Attention needs float32 tensors on a HIP device ({name} is {t.dtype} on {t.device}); "
                                   "there is no CPU path")
        if x.dim() != 3 or context.dim() != 3 or x.size(0) != context.size(0):
            raise ValueError(f"expected x [B,Nq,{self.to_q.in_features}] and context [B,Nk,{self.to_kv.in_features}], got "
                             f"{tuple(x.shape)} and {tuple(context.shape)}")
        if x.size(2) != self.to_q.in_features or context.size(2) != self.to_kv.in_features:
            raise ValueError(f"width mismatch: x {tuple(x.shape)} for query_dim {self.to_q.in_features}, context "
                             f"{tuple(context.shape)} for context_dim {self.to_kv.in_features}")
        q = self.to_q(x)
        kv = self.to_kv(context)
        if return_attention_weights:
            return self._attention_weights(q, kv, mask)
        p = self.dropout_p if self.training else 0.0
        rng = None
        if p > 0.0:
            if not self._seeded:
                self.manual_seed(torch.initial_seed())
            rng = self.rng_state.clone()  # the state this forward and its backward see
            self.rng_state[1:].add_(1)
        out = fused_attention_kv(q, kv, self.heads, mask=mask, dropout_p=p, rng_state=rng)
        return self.to_out(out)

    def _attention_weights(self, q, kv, mask):
        """The visualisation path: the [B*H, Nq, Nk] softmax matrix is the request, so plain torch ops compute it."""
        h = self.heads
        k = kv.chunk(2, dim=-1)[0]
        B, Nq, Nk = q.size(0), q.size(1), k.size(1)
        q = q.reshape(B, Nq, h, DIM_HEAD).permute(0, 2, 1, 3).reshape(B * h, Nq, DIM_HEAD)
        k = k.reshape(B, Nk, h, DIM_HEAD).permute(0, 2, 1, 3).reshape(B * h, Nk, DIM_HEAD)
        sim = torch.einsum("bid,bjd->bij", q, k) * self.scale
        if mask is not None:
            m = mask.reshape(B, -1).bool()
            sim.masked_fill_(~m.repeat_interleave(h, dim=0)[:, None, :], -torch.finfo(sim.dtype).max)
        return sim.softmax(dim=-1)
