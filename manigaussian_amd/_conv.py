"""What the Conv3d families (conv3d.py, pointwise.py, narrow.py, dense.py) and their routing (encoder.py, volume.py) share: the
argument checks that differ only in the numbers they print, the opening of a bias-carrying backward, and the opening of a routing
predicate.  What is specific to a family -- channel ranges, padding_mode, negative_slope, stride, output_padding, the batch limit --
stays in that family's module.
"""
import torch

from . import _ops


def check_shapes(x, weight, kernels, channel_dim=1):
    """x is [B,C,D,H,W] and not empty; weight is a k x k x k kernel, k in `kernels`, over the channels of x (its dimension
    `channel_dim`), on the device of x."""
    if x.dim() != 5 or x.numel() == 0:
        raise ValueError(f"expected x [B,C,D,H,W] with no empty dimension, got {tuple(x.shape)}")
    if weight.dim() != 5 or tuple(weight.shape[2:]) not in [(k, k, k) for k in kernels] or weight.size(channel_dim) != x.size(1):
        sizes = " or ".join(f"{k}x{k}x{k}" for k in kernels)
        raise ValueError(f"weight {tuple(weight.shape)} is not a {sizes} kernel over the {x.size(1)} channels of x")
    if weight.device != x.device:
        raise ValueError(f"weight must be on {x.device}")


def check_bias(x, weight, bias):
    """bias is None or [Cout] on the device of x."""
    if bias is not None and (tuple(bias.shape) != (weight.size(0),) or bias.device != x.device):
        raise ValueError(f"bias must be a [{weight.size(0)}] tensor on {x.device}, got {tuple(bias.shape)} on {bias.device}")


def check_rows(x):
    """The kernels index inside a (batch, channel) row of x in 32 bits."""
    if x[0, 0].numel() >= 2 ** 31:
        raise ValueError(f"x {tuple(x.shape)}: a (batch, channel) row must hold fewer than 2^31 elements")


def backward_begin(ctx, x, weight, g):
    """The opening of a backward over (x, weight, bias, ...): None when no gradient is asked for, else (g made readable, dx, dw, db),
    each result allocated only where asked for."""
    need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    need_b = ctx.has_bias and ctx.needs_input_grad[2]
    if not (need_x or need_w or need_b):
        return None
    g = _ops.readable(g)
    dx = torch.empty_like(x) if need_x else None
    dw = torch.empty_like(weight) if need_w else None
    db = torch.empty(weight.size(0), dtype=torch.float32, device=x.device) if need_b else None
    return g, dx, dw, db


def routable(x, weight, bias=None):
    """The opening of a routing predicate: x is a float32 HIP tensor, 5-D and not empty, and the module's weight and optional bias
    are float32 on its device."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 5 or x.numel() == 0:
        return False
    if weight.dtype != torch.float32 or weight.device != x.device:
        return False
    return bias is None or (bias.dtype == torch.float32 and bias.device == x.device)
