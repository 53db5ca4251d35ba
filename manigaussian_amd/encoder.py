"""The Perceiver's 3-D conv stem (helpers/network_utils.py:219-306, classes InPlaceABN, ConvBnReLU3D and
MultiLayer3DEncoderShallow) with its ten normalisation sites fused (csrc/mgs_abn.hip).

    batch_norm_act(x, weight, bias, running_mean, running_var, num_batches_tracked, training=..., residual=...)
        residual + leaky_relu(batch_norm(x)) with nn.BatchNorm3d's semantics (biased variance to normalise, unbiased into
        running_var, both running buffers and the counter updated in place by the launch itself).  Training forward: two launches;
        eval: one; backward: two.  Keeps x and two floats per channel (mean, 1/std), nothing else of the volume's size: the backward
        recomputes the activation's argument with the forward's own expression.  The gradient towards `residual` is the incoming
        gradient itself.  No atomics: the same bits from run to run, whatever the split of a row over workgroups.  Capturable into
        a HIP graph.  There is no CPU path.

`InPlaceABN`, `ConvBnReLU3D` and `MultiLayer3DEncoderShallow` have the reference's constructors, attribute and parameter names and
initialisation (InPlaceABN keeps a real nn.BatchNorm3d as `bn`): the stem's 62 state_dict entries load with strict=True and the other
way round.  The 3x3x3 convolutions are nn.Conv3d / nn.ConvTranspose3d modules whose weights go through conv3d / conv_transpose3d
(conv3d.py, csrc/mgs_conv3d.hip) where conv_site() says so (CONV overrides it; a CPU tensor, another dtype, a bias or any other
kernel size, padding, dilation or groups stays torch's).  The 1x1x1 conv_out with bias goes through pointwise_conv3d (pointwise.py,
csrc/mgs_pointwise.hip) where pointwise_site() says so (POINTWISE overrides it), and with 65..256 output channels (out_channels = 128,
the reference's final_dim) through wide_pointwise_conv3d where wide_pointwise_site() says so.  The stem hands conv4 / conv2 / conv0 to its three
transposed-convolution sites as the skip tensor.  A site runs the reference's torch composition on a CPU tensor, for a dtype other than float32, for momentum=None, in
eval mode with gradients enabled -- and wherever fused_site() says the fused op was not measured faster (FORCE overrides it).
"""
import torch
from torch import nn

from . import _conv, _lib, _ops
from .conv3d import conv3d, conv_transpose3d
from .pointwise import WIDE_MAX_CIN, WIDE_MAX_COUT, WIDE_MIN_COUT, pointwise_conv3d, wide_pointwise_conv3d

MAX_C = 65536
MAX_CONV_C = 64

# Which sites the drop-in modules send through batch_norm_act (the function itself always takes the kernels).  FORCE: None = follow
# fused_site(); True / False = every eligible site fused / none (tests, scripts/bench_encoder.py).
FORCE = None


FUSED_MIN_ELEMENTS = 8_000_000   # B C D H W of the smallest volume measured faster in all four (pass, form) pairs: [1, 8, 100^3]


def fused_site(values_per_channel, channels):
    """The routing rule (values_per_channel = B D H W), from the measurement (scripts/bench_encoder.py ->
    profiles/encoder_bench.json): a site is fused only where the op was faster than torch's BatchNorm3d -> LeakyReLU
    (-> add) forward AND forward + backward, eager AND graph-replayed, by more than the run-to-run spread.  On an MI355X at B = 1
    that holds at [8, 100^3] (conv0, conv11: 25 against 315 us forward, 188 / 53 against 593 / 594 us forward + backward eager /
    graph-replayed).  At [16, 50^3] and below the kernels win graph-replayed (25 against 90 us at 50^3), but an eager forward +
    backward is bound by the host's enqueue path, where this module's Python autograd function is no faster than torch's nodes
    (75 against 70 to 86 us, or 185 to 215 against 130 to 170 us: the host has two speeds), so those eight sites stay on torch's
    composition; [16, 50^3] with the skip add won one run of three, inside that spread.  Between 2 and 8 million elements nothing
    was measured: not fused."""
    return values_per_channel * channels >= FUSED_MIN_ELEMENTS


# Which of the stem's 3x3x3 convolutions the drop-in modules send through conv3d / conv_transpose3d (csrc/mgs_conv3d.hip).  CONV: None =
# follow conv_site(); True / False = every eligible site / none (tests, scripts/bench_conv3d.py).  FORCE = False keeps them on torch too.
CONV = None
CONV_MIN_VOXELS = 50 ** 3          # the smallest measured winner's input volume (conv2: [16, 50^3] -> [16, 50^3], stride 1)
CONV_MIN_VOXELS_STRIDED = 100 ** 3   # ... and the smallest with stride 2, transposed or not (conv1, conv11: a 100^3 input side)


def conv_site(cin, cout, voxels, stride, transposed):
    """The routing rule of the convolutions (voxels = D H W of the convolution's input; for a transposed site, of its OUTPUT, the
    input side of the convolution it transposes), from the measurement (scripts/bench_conv3d.py -> profiles/conv3d_bench.json,
    DESIGN.md 7m), by fused_site()'s criterion: a site is routed only where the op's third quartile lay below torch's first quartile
    for forward AND forward + backward, eager AND graph-replayed, torch taken at the faster of cudnn.benchmark off and on.  On an
    MI355X at B = 1 that holds for conv0, conv1, conv2 and conv11 (forward 1.3 to 5.1 x, forward + backward 58 to 262 x: torch's
    weight gradient alone takes 18 to 147 ms there).  At a 50^3 input side with stride 2 (conv3) and at 25^3 (conv4) the op wins
    forward + backward 6.9 / 6.6 x but loses the forward alone (133 against 45 us, 116 against 75 us); conv9 (transposed, 50^3
    output) won its forward by 5 % in the committed run and lost it by 1 % in the run before: inside the spread between runs; at
    25^3 with stride 2 and at 13^3 (conv5, conv6, conv7) the op loses every pair: a few dozen workgroups on 256 CUs.  Those six
    stay torch's.  Nothing was measured between the sizes or at other channel counts: the thresholds are the winners' own volumes."""
    if stride == 1 and not transposed:
        return voxels >= CONV_MIN_VOXELS
    return voxels >= CONV_MIN_VOXELS_STRIDED


def _conv_routed(conv, x, transposed):
    """Whether `conv` (a bias-free 3x3x3 nn.Conv3d / stride-2 nn.ConvTranspose3d of the stem's kind) on x goes through the kernels."""
    w = conv.weight
    if CONV is False or FORCE is False or conv.bias is not None or not _conv.routable(x, w):
        return False
    if conv.kernel_size != (3, 3, 3) or conv.padding != (1, 1, 1) or conv.dilation != (1, 1, 1) or conv.groups != 1:
        return False
    if conv.padding_mode != "zeros" or max(w.shape[:2]) > MAX_CONV_C or x.size(1) != conv.in_channels:
        return False
    if transposed:
        op = conv.output_padding
        if conv.stride != (2, 2, 2) or op not in ((0, 0, 0), (1, 1, 1)):
            return False
        voxels = (2 * x.size(2) - 1 + op[0]) * (2 * x.size(3) - 1 + op[0]) * (2 * x.size(4) - 1 + op[0])
        cin, cout = conv.out_channels, conv.in_channels   # of the convolution it transposes
    else:
        if conv.stride not in ((1, 1, 1), (2, 2, 2)):
            return False
        voxels = x[0, 0].numel()
        cin, cout = conv.in_channels, conv.out_channels
    if voxels >= 2 ** 31:
        return False
    return True if CONV else conv_site(cin, cout, voxels, conv.stride[0], transposed)


# Whether the stem's 1x1x1 conv_out goes through pointwise_conv3d (csrc/mgs_pointwise.hip).  POINTWISE: None = follow pointwise_site();
# True / False = every eligible site / none (tests, scripts/bench_pointwise.py).  FORCE = False keeps it on torch too; FORCE = True
# and CONV = True do not switch it on.
POINTWISE = None
POINTWISE_CHANNELS = (8, 64)  # the channel counts that were measured (conv_out's)
POINTWISE_MIN_VALUES = 50 ** 3  # B D H W of the smallest measured winner, [1, 8 -> 64, 50^3] (None: no measured shape won all four pairs)


def pointwise_site(cin, cout, values_per_channel):
    """The routing rule of the 1x1x1 convolution (values_per_channel = B D H W), from the measurement (scripts/bench_pointwise.py ->
    profiles/pointwise_bench.json), by fused_site()'s criterion: a shape is routed only where the op's third quartile
    lay below torch's first quartile for forward AND forward + backward, eager AND graph-replayed, torch taken at the faster of
    cudnn.benchmark off and on.  Measured on an MI355X at 8 -> 64 channels, B = 1: at 100^3 (conv_out) the op wins the forward 5.7 x
    and forward + backward 400 x (0.33 against 132 ms: torch's weight and bias gradient alone takes 126 ms), at 50^3 2.3 x and 86 x;
    at 25^3 it wins forward + backward 16 x but loses the forward alone (31 against 22 us eager, 34 against 16 us graph-replayed), so
    25^3 is not routed.  Nothing else was measured, so nothing else is routed: the threshold is the smallest winner's own size, at
    its own channel counts."""
    if POINTWISE_MIN_VALUES is None:
        return False
    return (cin, cout) == POINTWISE_CHANNELS and values_per_channel >= POINTWISE_MIN_VALUES


def _pointwise_routed(conv, x):
    """Whether `conv` (a 1x1x1 nn.Conv3d of conv_out's kind, with or without a bias) on x goes through the kernels."""
    w = conv.weight
    if POINTWISE is False or FORCE is False or not _conv.routable(x, w, conv.bias):
        return False
    if conv.kernel_size != (1, 1, 1) or conv.stride != (1, 1, 1) or conv.padding != (0, 0, 0) or conv.dilation != (1, 1, 1):
        return False
    if conv.groups != 1 or conv.padding_mode != "zeros" or max(w.shape[:2]) > MAX_CONV_C or x.size(1) != conv.in_channels:
        return False
    if x[0, 0].numel() >= 2 ** 31:
        return False
    return True if POINTWISE else pointwise_site(conv.in_channels, conv.out_channels, x.numel() // x.size(1))


# The same conv_out with 65..256 output channels (out_channels = 128) through wide_pointwise_conv3d.  It follows the switches above:
# POINTWISE = None: wide_pointwise_site(); True / False: every eligible site / none.
WIDE_POINTWISE_CHANNELS = (8, 128)  # the channel counts that were measured (conv_out's at final_dim = 128)
WIDE_POINTWISE_MIN_VALUES = 100 ** 3  # B D H W of the smallest measured winner, [1, 8 -> 128, 100^3] (None: no shape won all four pairs)


def wide_pointwise_site(cin, cout, values_per_channel):
    """The routing rule of the 1x1x1 convolution with 65..256 output channels (values_per_channel = B D H W), from the measurement
    (scripts/bench_wide_pointwise.py -> profiles/wide_pointwise_bench.json), by fused_site()'s criterion, as
    pointwise_site().  Measured on an MI355X at 8 -> 128 channels, B = 1: at 100^3 the op wins the forward 2.2 x and forward +
    backward 198 x (0.67 against 132.5 ms: torch's weight and bias gradient alone takes 131.9 ms).  At 50^3 it wins forward + backward
    84 x but its forward ties torch's (44.6 against 43.9 us eager, 50.0 against 49.4 us graph-replayed), and at 25^3 the forward loses
    2.7 x: neither is routed, and POINTWISE = True is the caller's switch there.  Nothing is routed below the smallest measured
    winner's size or at channel counts nobody measured."""
    if WIDE_POINTWISE_MIN_VALUES is None:
        return False
    return (cin, cout) == WIDE_POINTWISE_CHANNELS and values_per_channel >= WIDE_POINTWISE_MIN_VALUES


def _wide_pointwise_routed(conv, x):
    """_pointwise_routed's questions for 1..16 input and 65..256 output channels."""
    w = conv.weight
    if POINTWISE is False or FORCE is False or not _conv.routable(x, w, conv.bias):
        return False
    if conv.kernel_size != (1, 1, 1) or conv.stride != (1, 1, 1) or conv.padding != (0, 0, 0) or conv.dilation != (1, 1, 1):
        return False
    if conv.groups != 1 or conv.padding_mode != "zeros" or x.size(1) != conv.in_channels:
        return False
    if not (1 <= w.size(1) <= WIDE_MAX_CIN and WIDE_MIN_COUT <= w.size(0) <= WIDE_MAX_COUT) or x[0, 0].numel() >= 2 ** 31:
        return False
    return True if POINTWISE else wide_pointwise_site(conv.in_channels, conv.out_channels, x.numel() // x.size(1))


class _BatchNormAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, residual, running_mean, running_var, num_batches_tracked, training, momentum, eps, slope,
                slices):
        x = _ops.readable(x)
        res = None if residual is None else _ops.readable(residual)
        dev = x.device
        B, C = x.shape[:2]
        n = x[0, 0].numel()
        weight, bias = weight.contiguous(), bias.contiguous()
        y = torch.empty(x.shape, dtype=torch.float32, device=dev)
        stats = ws = None
        if training:
            stats = torch.empty(C, 2, dtype=torch.float32, device=dev)
            # the sub-slice records: written by every forward (and backward) before it reads them
            ws = _ops.workspace(dev, _lib.lib().mgs_abn_workspace_bytes(B, C, n))
        _ops.call("mgs_abn_forward", dev, B, C, n, x.data_ptr(), _ops.ptr(res), weight.data_ptr(), bias.data_ptr(),
                  _ops.ptr(running_mean), _ops.ptr(running_var), _ops.ptr(num_batches_tracked), int(training), momentum, eps, slope,
                  y.data_ptr(), _ops.ptr(stats), _ops.ptr(ws), ws.numel() if ws is not None else 0, slices)
        if training:
            ctx.save_for_backward(x, weight, bias, stats)
        ctx.training, ctx.slope, ctx.slices = training, slope, slices
        return y

    @staticmethod
    def backward(ctx, g):
        if not ctx.training:
            raise RuntimeError("batch_norm_act has no backward in eval mode (training=False)")
        x, weight, bias, stats = ctx.saved_tensors
        dev = x.device
        B, C = x.shape[:2]
        n = x[0, 0].numel()
        gy = _ops.readable(g)
        dx = torch.empty_like(x)
        dwb = torch.empty(2, C, dtype=torch.float32, device=dev)
        ws = _ops.workspace(dev, _lib.lib().mgs_abn_workspace_bytes(B, C, n))
        _ops.call("mgs_abn_backward", dev, B, C, n, x.data_ptr(), gy.data_ptr(), weight.data_ptr(), bias.data_ptr(),
                  stats.data_ptr(), ctx.slope, dx.data_ptr(), dwb[0].data_ptr(), dwb[1].data_ptr(), ws.data_ptr(), ws.numel(),
                  ctx.slices)
        need = ctx.needs_input_grad
        return (dx if need[0] else None, dwb[0] if need[1] else None, dwb[1] if need[2] else None, g if need[3] else None,
                None, None, None, None, None, None, None, None)


def _batch_norm_act(x, weight, bias, running_mean, running_var, num_batches_tracked, training, momentum, eps, negative_slope,
                    residual, slices=0):
    """batch_norm_act with `slices`: 0 = the library's split of a row over workgroups, 1..64 = that many (a test aid)."""
    _ops.need_float32("batch_norm_act", ("residual",), x=x, residual=residual)
    if x.dim() != 5 or x.numel() == 0:
        raise ValueError(f"expected x [B,C,D,H,W] with no empty dimension, got {tuple(x.shape)}")
    if residual is not None and residual.shape != x.shape:
        raise ValueError(f"residual {tuple(residual.shape)} does not match x {tuple(x.shape)}")
    C = x.size(1)
    if C > MAX_C:
        raise ValueError(f"C = {C}: at most {MAX_C} channels")
    for name, t in (("weight", weight), ("bias", bias)):
        if not isinstance(t, torch.Tensor) or t.shape != (C,) or t.dtype != torch.float32 or t.device != x.device:
            raise ValueError(f"{name} must be a float32 [{C}] tensor on {x.device}")
    if (running_mean is None) != (running_var is None):
        raise ValueError("running_mean and running_var: both or neither")
    for name, t in (("running_mean", running_mean), ("running_var", running_var)):
        if t is not None and (t.shape != (C,) or t.dtype != torch.float32 or t.device != x.device or not t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous float32 [{C}] tensor on {x.device}")
    if num_batches_tracked is not None and (num_batches_tracked.dtype != torch.int64 or num_batches_tracked.numel() != 1
                                            or num_batches_tracked.device != x.device):
        raise ValueError(f"num_batches_tracked must be one int64 on {x.device}")
    training = bool(training)
    if training and x.numel() // C == 1:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {x.size()}")
    if not training and running_mean is None:
        raise ValueError("training=False needs running_mean and running_var")
    if momentum is None:
        raise ValueError("momentum=None (a cumulative average) is not supported; use torch's batch norm")
    return _BatchNormAct.apply(x, weight, bias, residual, running_mean, running_var, num_batches_tracked if training else None,
                               training, float(momentum), float(eps), float(negative_slope), int(slices))


def batch_norm_act(x, weight, bias, running_mean, running_var, num_batches_tracked=None, *, training, momentum=0.1, eps=1e-5,
                   negative_slope=0.01, residual=None):
    """y = residual + leaky_relu(batch_norm(x), negative_slope); x and residual [B,C,D,H,W] fp32 on a HIP device, the rest [C].
    training: batch statistics, and running_mean / running_var / num_batches_tracked (each may be None) updated in place;
    else the running buffers normalise and nothing is updated (forward only).  negative_slope = 0 is ReLU."""
    return _batch_norm_act(x, weight, bias, running_mean, running_var, num_batches_tracked, training, momentum, eps, negative_slope,
                           residual)


class InPlaceABN(nn.Module):
    """helpers/network_utils.py:219's InPlaceABN; forward takes the skip tensor of the add that follows three of its uses."""

    def __init__(self, out_channels, activation='leaky_relu'):
        super().__init__()
        acts = {'leaky_relu': nn.LeakyReLU, 'relu': nn.ReLU}
        if activation not in acts:
            raise ValueError()
        self.bn = nn.BatchNorm3d(out_channels)
        self.act = acts[activation](inplace=True)

    def _fused(self, x):
        bn = self.bn
        if FORCE is False or not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 5:
            return False
        if bn.momentum is None or not bn.affine or not bn.track_running_stats or bn.weight.dtype != torch.float32:
            return False
        if x.numel() == 0 or x.size(1) != bn.num_features or x.size(1) > MAX_C:
            return False
        if bn.training and x.numel() // x.size(1) == 1:
            return False  # (torch's own error, from torch's own call)
        if not bn.training and torch.is_grad_enabled():
            return False
        return True if FORCE else fused_site(x.numel() // x.size(1), x.size(1))

    def forward(self, x, residual=None):
        if self._fused(x) and (residual is None or (residual.is_cuda and residual.dtype == torch.float32
                                                    and residual.shape == x.shape)):
            bn = self.bn
            return batch_norm_act(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked,
                                  training=bn.training, momentum=bn.momentum, eps=bn.eps,
                                  negative_slope=getattr(self.act, "negative_slope", 0.0), residual=residual)
        x = self.act(self.bn(x))
        return x if residual is None else residual + x


class ConvBnReLU3D(nn.Module):
    """helpers/network_utils.py:234's ConvBnReLU3D: a bias-free nn.Conv3d (`conv`) and its norm_act (`bn`)."""

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, pad=1, norm_act=InPlaceABN):
        super().__init__()
        self.conv = nn.Conv3d(in_channels, out_channels, kernel_size, stride=stride, padding=pad, bias=False)
        self.bn = norm_act(out_channels)

    def forward(self, x):
        if _conv_routed(self.conv, x, False):
            return self.bn(conv3d(x, self.conv.weight, self.conv.stride[0]))
        return self.bn(self.conv(x))


def _up_site(cin, cout, output_padding, norm_act):
    """A stride-2 transposed convolution back up one level and its norm_act, as the Sequential the state_dict names (`.0`, `.1`)."""
    return nn.Sequential(nn.ConvTranspose3d(cin, cout, 3, padding=1, output_padding=output_padding, stride=2, bias=False),
                         norm_act(cout))


def _up(site, x, skip):
    """skip + site(x): the add goes into the norm_act when it is ours."""
    conv = site[0]
    if isinstance(conv, nn.ConvTranspose3d) and _conv_routed(conv, x, True):
        y = conv_transpose3d(x, conv.weight, conv.output_padding[0])
    else:
        y = conv(x)
    if len(site) == 2 and isinstance(site[1], InPlaceABN):
        return site[1](y, residual=skip)
    return skip + site[1:](y)


class MultiLayer3DEncoderShallow(nn.Module):
    """helpers/network_utils.py:248's MultiLayer3DEncoderShallow, the point-cloud voxel encoder: [B, in_channels, S, S, S] ->
    ([B, out_channels, S, S, S], [input, the 32-channel volume at S/4, the 16-channel volume at S/2]).  Three levels down
    (8 -> 16 -> 32 -> 64 channels, stride 2 each), three back up with skip adds, a 1x1x1 convolution out.  Sub-modules are created
    in the reference's order, so a seeded construction draws the same initial weights."""
    CHANNELS = (8, 16, 32, 64)

    def __init__(self, in_channels=10, out_channels=64, norm_act=InPlaceABN):
        super().__init__()
        self.out_channels = out_channels
        c0, c1, c2, c3 = self.CHANNELS
        self.conv0 = ConvBnReLU3D(in_channels, c0, norm_act=norm_act)
        self.conv1 = ConvBnReLU3D(c0, c1, stride=2, norm_act=norm_act)
        self.conv2 = ConvBnReLU3D(c1, c1, norm_act=norm_act)
        self.conv3 = ConvBnReLU3D(c1, c2, stride=2, norm_act=norm_act)
        self.conv4 = ConvBnReLU3D(c2, c2, norm_act=norm_act)
        self.conv5 = ConvBnReLU3D(c2, c3, stride=2, norm_act=norm_act)
        self.conv6 = ConvBnReLU3D(c3, c3, norm_act=norm_act)
        self.conv7 = _up_site(c3, c2, 0, norm_act)    # 13^3 -> 25^3: no output padding
        self.conv9 = _up_site(c2, c1, 1, norm_act)
        self.conv11 = _up_site(c1, c0, 1, norm_act)
        self.conv_out = nn.Conv3d(c0, out_channels, 1, stride=1, padding=0, bias=True)

    def forward(self, x):
        voxel_list = [x]                                   # the multi-scale features the decoder reads
        conv0 = self.conv0(x)
        conv2 = self.conv2(self.conv1(conv0))              # 16 channels at half size
        conv4 = self.conv4(self.conv3(conv2))              # 32 at a quarter
        x = self.conv6(self.conv5(conv4))                  # 64 at an eighth
        x = _up(self.conv7, x, conv4)
        del conv4
        voxel_list.append(x)
        x = _up(self.conv9, x, conv2)
        del conv2
        voxel_list.append(x)
        x = _up(self.conv11, x, conv0)
        del conv0
        if _pointwise_routed(self.conv_out, x):
            return pointwise_conv3d(x, self.conv_out.weight, self.conv_out.bias), voxel_list
        if _wide_pointwise_routed(self.conv_out, x):
            return wide_pointwise_conv3d(x, self.conv_out.weight, self.conv_out.bias), voxel_list
        return self.conv_out(x), voxel_list
