"""What the Perceiver decoder does to its 100^3 volumes between the convolutions (agents/manigaussian_bc/perceiver_lang_io.py:
488-499; helpers/network_utils.py:129-171 Conv3DBlock, 374-391 Conv3DUpsampleBlock), fused.

    resample_pad(sources, scale, pad) = F.pad(F.interpolate(torch.cat(sources, 1), scale_factor=scale, mode='trilinear',
                                                            align_corners=False), (pad,) * 6, mode='replicate')

as ONE launch (csrc/mgs_volume.hip) that reads the sources where they lie -- a channel slice of a wider tensor is not copied --
and writes the padded volume once; neither the concatenation nor the unpadded upsampled volume ever exists.  The backward is a
gather (two launches for scale > 1, one for scale == 1): no atomics, no zero-fill, the same bits from run to run, capturable.
CPU tensors take the torch composition above.

`Conv3DBlock` and `Conv3DUpsampleBlock` have the reference's constructors, parameter names and initialisation; a reference
state_dict loads with strict=True and the other way round.  The convolutions stay MIOpen's and the activations torch's: a block
in replicate mode hands `F.conv3d(..., padding=0)` the volume this op padded, which is what nn.Conv3d computes in that mode.
The one exception is a 3x3x3 block with at most 4 output channels (trans_decoder, perceiver_lang_io.py:322): where narrow_site()
says so (NARROW overrides it) it goes through narrow_conv3d (narrow.py, csrc/mgs_narrow.hip), which folds the pad into its
addressing, so that the input is not padded first.  A dense 3x3x3 or 5x5x5 block at channel counts dense_conv3d takes (up0's two
blocks and final) runs its convolution, bias and ReLU / leaky ReLU as one op on the volume this module padded (dense.py,
csrc/mgs_dense.hip) where dense_site() says so (DENSE overrides it).  A block whose stride is its kernel (the Perceiver's patchify,
perceiver_lang_io.py:235) goes through patch_conv3d (patch.py, csrc/mgs_patch.hip) -- pad, convolution, bias and activation in one op on
the unpadded volume -- where patch_site() says so (PATCH overrides it).
"""
import ctypes

import torch
import torch.nn.functional as F
from torch import nn

from . import _conv, _lib, _ops
from . import dense as _dense
from . import patch as _patch
from .dense import dense_conv3d
from .narrow import MAX_CIN as NARROW_MAX_CIN, MAX_COUT as NARROW_MAX_COUT, narrow_conv3d

LRELU_SLOPE = 0.02
MAX_SOURCES, MAX_SCALE, MAX_PAD = _lib.VOLUME_MAX_SOURCES, 8, 8

# Whether a narrow-output 3x3x3 block goes through narrow_conv3d (csrc/mgs_narrow.hip).  NARROW: None = follow narrow_site();
# True / False = every eligible block / none (tests, scripts/bench_narrow.py).
NARROW = None
NARROW_CHANNELS = (128, 1)   # the channel counts that were measured (trans_decoder's)
NARROW_MIN_VOXELS = 25 ** 3  # D H W of the smallest measured winner, [1, 128 -> 1, 25^3] (None: no measured shape won all four pairs)


def narrow_site(cin, cout, voxels):
    """The routing rule of the narrow-output 3x3x3 block (voxels = D H W), from the measurement (scripts/bench_narrow.py ->
    profiles/narrow_conv_bench.json), by encoder.fused_site()'s criterion: a shape is routed only where the op's third
    quartile lay below the first quartile of the parent's path (resample_pad + F.conv3d(padding=0), at the faster of cudnn.benchmark
    off and on) for forward AND forward + backward, eager AND graph-replayed.  Nothing else was measured, so nothing else is routed:
    the threshold is the smallest winner's own size, at its own channel counts."""
    if NARROW_MIN_VOXELS is None:
        return False
    return (cin, cout) == NARROW_CHANNELS and voxels >= NARROW_MIN_VOXELS


def _narrow_routed(conv, x):
    """Whether `conv` (a 3x3x3 nn.Conv3d of trans_decoder's kind) on x goes through the kernels."""
    if NARROW is False or not _conv.routable(x, conv.weight, conv.bias):
        return False
    if conv.kernel_size != (3, 3, 3) or conv.stride != (1, 1, 1) or conv.padding != (1, 1, 1) or conv.dilation != (1, 1, 1):
        return False
    if conv.groups != 1 or conv.padding_mode not in ("replicate", "zeros") or x.size(1) != conv.in_channels:
        return False
    if conv.out_channels > NARROW_MAX_COUT or conv.in_channels > NARROW_MAX_CIN or x[0, 0].numel() >= 2 ** 31:
        return False
    return True if NARROW else narrow_site(conv.in_channels, conv.out_channels, x[0, 0].numel())


# Whether a dense 3x3x3 / 5x5x5 block's convolution (on the padded volume) goes through dense_conv3d (csrc/mgs_dense.hip).  DENSE:
# None = follow dense_site(); True / False = every eligible block / none (tests, scripts/bench_dense.py).
DENSE = None
# (cin, cout, k) -> output voxels of the smallest measured winner at these channel counts (scripts/bench_dense.py ->
# profiles/dense_conv_bench.json); a triple that was not measured, or that won nowhere, is not here
DENSE_MIN_VOXELS = {}


def dense_site(cin, cout, k, voxels):
    """The routing rule of the dense blocks (voxels = output D H W), from the measurement (scripts/bench_dense.py ->
    profiles/dense_conv_bench.json), by encoder.fused_site()'s criterion: a shape is routed only where the op's third
    quartile lay below the first quartile of torch's F.leaky_relu(F.conv3d(...)) (at the faster of cudnn.benchmark off and on) for
    forward AND forward + backward, eager AND graph-replayed.  Only measured (cin, cout, k) triples are routed, each from its
    smallest measured winner's size up."""
    least = DENSE_MIN_VOXELS.get((cin, cout, k))
    return least is not None and voxels >= least


def _dense_slope(activation):
    """(whether the op can fuse the block's activation, the slope it takes)"""
    if activation is None:
        return True, None
    if type(activation) is nn.LeakyReLU and activation.negative_slope >= 0:
        return True, float(activation.negative_slope)
    if type(activation) is nn.ReLU:
        return True, 0.0
    return False, None


def _dense_routed(conv, x):
    """Whether `conv` on x, the volume that already carries its padding, goes through the kernels."""
    if DENSE is False or not _conv.routable(x, conv.weight, conv.bias):
        return False
    k = conv.kernel_size
    if len(set(k)) != 1 or conv.stride != (1, 1, 1) or conv.dilation != (1, 1, 1) or conv.groups != 1 or x.size(1) != conv.in_channels:
        return False
    if x.size(0) > 65535 or not _dense.eligible(conv.in_channels, conv.out_channels, k[0], tuple(x.shape[2:])):
        return False
    if DENSE:
        return True
    return dense_site(conv.in_channels, conv.out_channels, k[0], (x.size(2) - k[0] + 1) * (x.size(3) - k[0] + 1) * (x.size(4) - k[0] + 1))


# Whether a block whose stride is its kernel goes through patch_conv3d (csrc/mgs_patch.hip).  PATCH: None = follow patch_site();
# True / False = every eligible block / none (tests, scripts/bench_patch.py).
PATCH = None
# (cin, cout, k) -> input voxels D H W of the smallest measured winner at these channel counts (scripts/bench_patch.py ->
# profiles/patch_conv_bench.json); a triple that was not measured, or that won nowhere, is not here
PATCH_MIN_VOXELS = {}


def patch_site(cin, cout, k, voxels):
    """The routing rule of the kernel = stride blocks (voxels = input D H W), from the measurement (scripts/bench_patch.py ->
    profiles/patch_conv_bench.json), by encoder.fused_site()'s criterion: a shape is routed only where the op's third
    quartile lay below the first quartile of the parent's path (resample_pad + F.conv3d(stride=k) + the activation, at the faster of
    cudnn.benchmark off and on) for forward AND forward + backward, eager AND graph-replayed.  Only measured (cin, cout, k) triples
    are routed, each from its smallest measured winner's size up."""
    least = PATCH_MIN_VOXELS.get((cin, cout, k))
    return least is not None and voxels >= least


def _patch_routed(conv, x, activation=None):
    """Whether `conv` (an nn.Conv3d whose stride is its cubic kernel) followed by `activation` goes through the kernels on x, the
    volume WITHOUT its padding."""
    if PATCH is False or not _conv.routable(x, conv.weight, conv.bias):
        return False
    k, p = conv.kernel_size, conv.padding
    if len(set(k)) != 1 or conv.stride != k or conv.dilation != (1, 1, 1) or conv.groups != 1 or x.size(1) != conv.in_channels:
        return False
    if conv.padding_mode not in _patch.PADDING_MODES or isinstance(p, str) or len(set(p)) != 1:
        return False
    if not _patch.eligible(conv.in_channels, conv.out_channels, k[0], p[0], tuple(x.shape[2:]), x.size(0)):
        return False
    if not _dense_slope(activation)[0]:
        return False
    return True if PATCH else patch_site(conv.in_channels, conv.out_channels, k[0], x[0, 0].numel())


def _in_place(t):
    """The tensor itself when the kernels can read it where it lies -- spatial dimensions contiguous, batch and channel strides
    whatever they are -- else a row-major copy."""
    _, _, D, H, W = t.shape
    sd, sh, sw = t.stride()[2:]
    if (W == 1 or sw == 1) and (H == 1 or sh == W) and (D == 1 or sd == H * W):
        return t
    return t.clone(memory_format=torch.contiguous_format)


def _args(shapes, scale, pad):
    """MgsVolumeArgs of sources of these shapes [B, C_k, D, H, W] (pointers and strides left empty)."""
    a = _lib.MgsVolumeArgs()
    a.B, _, a.D, a.H, a.W = shapes[0]
    a.scale, a.pad, a.nsrc = scale, pad, len(shapes)
    for k, s in enumerate(shapes):
        a.C[k] = s[1]
    return a


def composition(sources, scale=1, pad=0):
    """The op in torch's own calls: the CPU path, and what the fused op is compared with."""
    x = sources[0] if len(sources) == 1 else torch.cat(list(sources), 1)
    if scale > 1:
        x = F.interpolate(x, scale_factor=scale, mode="trilinear", align_corners=False)
    return F.pad(x, (pad,) * 6, mode="replicate") if pad > 0 else x


class _ResamplePad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scale, pad, *sources):
        sources = [_in_place(t) for t in sources]
        dev = sources[0].device
        shapes = [tuple(t.shape) for t in sources]
        B, _, D, H, W = shapes[0]
        a = _args(shapes, scale, pad)
        for k, t in enumerate(sources):
            a.src[k], a.stride_b[k], a.stride_c[k] = t.data_ptr(), t.stride(0), t.stride(1)
        out = torch.empty(B, sum(s[1] for s in shapes), scale * D + 2 * pad, scale * H + 2 * pad, scale * W + 2 * pad,
                          dtype=torch.float32, device=dev)
        _ops.call("mgs_volume_resample_pad_forward", dev, ctypes.byref(a), out.data_ptr())
        ctx.shapes, ctx.scale, ctx.pad = shapes, scale, pad  # (a linear op: its gradient needs no tensor of the forward)
        return out

    @staticmethod
    def backward(ctx, g_out):
        dev = g_out.device
        g_out = g_out.to(torch.float32).contiguous()
        a = _args(ctx.shapes, ctx.scale, ctx.pad)
        grads = [torch.empty(s, dtype=torch.float32, device=dev) for s in ctx.shapes]
        pointers = (_lib.c_fp * len(grads))(*[g.data_ptr() for g in grads])
        # the x y sums: written before they are read in every call
        ws = _ops.workspace(dev, _lib.lib().mgs_volume_workspace_bytes(ctypes.byref(a)))
        _ops.call("mgs_volume_resample_pad_backward", dev, ctypes.byref(a), g_out.data_ptr(), pointers, ws.data_ptr(), ws.numel())
        return (None, None) + tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad[2:]))


def resample_pad(sources, scale=1, pad=0):
    """sources: a tensor or a list / tuple of 1..4 tensors [B, C_k, D, H, W] of one batch size and spatial shape, fp32;
    scale 1..8 (trilinear, align_corners=False), pad 0..8 (replicate) -> [B, sum C_k, scale D + 2 pad, scale H + 2 pad,
    scale W + 2 pad].  Tensors on a HIP device take the fused kernels, CPU tensors torch's composition."""
    sources = [sources] if isinstance(sources, torch.Tensor) else list(sources)
    scale, pad = int(scale), int(pad)
    if not 1 <= len(sources) <= MAX_SOURCES:
        raise ValueError(f"resample_pad takes 1..{MAX_SOURCES} sources, got {len(sources)}")
    if not (1 <= scale <= MAX_SCALE and 0 <= pad <= MAX_PAD):
        raise ValueError(f"scale = {scale} (1..{MAX_SCALE}), pad = {pad} (0..{MAX_PAD})")
    first = sources[0]
    for t in sources:
        if not isinstance(t, torch.Tensor) or t.dim() != 5 or t.dtype != torch.float32:
            raise ValueError(f"expected float32 tensors [B,C,D,H,W], got {getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
        if t.shape[0] != first.shape[0] or t.shape[2:] != first.shape[2:] or t.device != first.device:
            raise ValueError(f"sources differ in batch, spatial shape or device: {tuple(first.shape)} on {first.device} and "
                             f"{tuple(t.shape)} on {t.device}")
        if t.shape[1] < 1 or min(t.shape[2:]) < 1:
            raise ValueError(f"a source of shape {tuple(t.shape)} has an empty channel or spatial dimension")
    if not first.is_cuda:
        return composition(sources, scale, pad)
    return _ResamplePad.apply(scale, pad, *sources)


def _activation(name):
    if name == "relu":
        return nn.ReLU()
    if name == "lrelu":
        return nn.LeakyReLU(LRELU_SLOPE)
    if name == "elu":
        return nn.ELU()
    if name == "tanh":
        return nn.Tanh()
    if name == "prelu":
        return nn.PReLU()
    raise ValueError("%s not recognized." % name)


class Conv3DBlock(nn.Module):
    """helpers/network_utils.py:129's Conv3DBlock.  forward takes a tensor, or a list / tuple of tensors to concatenate along
    the channels (`self.final([d0, latents])`): the concatenation is then never written."""

    def __init__(self, in_channels, out_channels, kernel_sizes=3, strides=1, norm=None, activation=None,
                 padding_mode="replicate", padding=None):
        super().__init__()
        padding = kernel_sizes // 2 if padding is None else padding
        self.conv3d = nn.Conv3d(in_channels, out_channels, kernel_sizes, strides, padding=padding, padding_mode=padding_mode)
        weight, bias = self.conv3d.weight, self.conv3d.bias
        if activation is None:
            nn.init.xavier_uniform_(weight, gain=nn.init.calculate_gain("linear"))
        elif activation == "tanh":
            nn.init.xavier_uniform_(weight, gain=nn.init.calculate_gain("tanh"))
        elif activation == "lrelu":
            nn.init.kaiming_uniform_(weight, a=LRELU_SLOPE, nonlinearity="leaky_relu")
        elif activation == "relu":
            nn.init.kaiming_uniform_(weight, nonlinearity="relu")
        else:
            raise ValueError()
        nn.init.zeros_(bias)
        if norm is not None:
            raise NotImplementedError("Norm not implemented.")
        self.norm = None
        self.activation = None if activation is None else _activation(activation)
        self.out_channels = out_channels

    def fused_pad(self):
        """The replicate pad this block's convolution asks for when resample_pad can provide it (one width on every side), else None."""
        c = self.conv3d
        p = c.padding
        if c.padding_mode == "replicate" and not isinstance(p, str) and len(set(p)) == 1 and 0 <= p[0] <= MAX_PAD:
            return p[0]
        return None

    def forward_padded(self, x):
        """The block on a volume that already carries its padding."""
        c = self.conv3d
        if _dense_routed(c, x):
            fused, slope = _dense_slope(self.activation)
            x = dense_conv3d(x, c.weight, c.bias, slope)
            return x if fused else self.activation(x)
        x = F.conv3d(x, c.weight, c.bias, c.stride, 0, c.dilation, c.groups)
        return self.activation(x) if self.activation is not None else x

    def forward(self, x):
        several = not isinstance(x, torch.Tensor)
        if not several and _narrow_routed(self.conv3d, x):
            c = self.conv3d
            x = narrow_conv3d(x, c.weight, c.bias, c.padding_mode)
            return self.activation(x) if self.activation is not None else x
        if not several and _patch_routed(self.conv3d, x, self.activation):
            c = self.conv3d
            return _patch.patch_conv3d(x, c.weight, c.bias, c.padding[0], c.padding_mode, _dense_slope(self.activation)[1])
        pad = self.fused_pad()
        if pad == 0 and not several and _dense_routed(self.conv3d, x):
            return self.forward_padded(x)
        if pad is None or (pad == 0 and not several):
            x = self.conv3d(torch.cat(list(x), 1) if several else x)
            return self.activation(x) if self.activation is not None else x
        return self.forward_padded(resample_pad(x, 1, pad))


class Conv3DUpsampleBlock(nn.Module):
    """helpers/network_utils.py:374's Conv3DUpsampleBlock, in the reference's nn.Sequential layout (the parameter-free
    nn.Upsample keeps its slot).  For strides > 1 the upsample and the second block's replicate pad are one resample_pad call."""

    def __init__(self, in_channels, out_channels, strides, kernel_sizes=3, norm=None, activation=None):
        super().__init__()
        layer = [Conv3DBlock(in_channels, out_channels, kernel_sizes, 1, norm, activation)]
        if strides > 1:
            layer.append(nn.Upsample(scale_factor=strides, mode="trilinear", align_corners=False))
        layer.append(Conv3DBlock(out_channels, out_channels, kernel_sizes, 1, norm, activation))
        self.conv_up = nn.Sequential(*layer)
        self.strides = strides

    def forward(self, x):
        if len(self.conv_up) == 2:
            return self.conv_up(x)
        first, _, last = self.conv_up
        pad = last.fused_pad()
        if pad is None or not (isinstance(self.strides, int) and 1 < self.strides <= MAX_SCALE):
            return self.conv_up(x)
        return last.forward_padded(resample_pad(first(x), self.strides, pad))
