"""The Perceiver's aggregated features (helpers/network_utils.py:927-963, class SpatialSoftmax3D, and the
nn.AdaptiveMaxPool3d(1) the encoder applies to the same volume at agents/manigaussian_bc/perceiver_lang_io.py:384,485,504), fused.

`SpatialSoftmax3D` has the reference's constructor, its `temperature` attribute (0.01, read at every call) and its three
registered buffers pos_x / pos_y / pos_z, built the same way: a reference state_dict loads with strict=True and the other way
round.  The kernels (csrc/mgs_spatial_softmax.hip) compute the positions from the voxel index and do not read the buffers.

Forward reads the volume ONCE and yields the three expected coordinates per channel and, for free, the channel's global maximum
(`forward_with_max`: the [ss | maxp] pair the Perceiver concatenates, as two views of one [B, 4C] buffer).  Backward reads the
volume once more and writes its gradient; between the two only the input itself and six floats per (batch, channel) are kept --
nothing of the volume's size.  No atomics: the same bits from run to run, whatever the split of a row over workgroups.
Capturable into a HIP graph.

There is no CPU path.
"""
import numpy as np
import torch
from torch import nn

from . import _lib, _ops

STATS = 6  # floats per (batch, channel): max, sum, E_x, E_y, E_z, argmax (the bits of a uint32)


def _rows_by_stride(t):
    """A [B, n] upstream gradient the kernels read by row stride."""
    return t if t.stride(1) == 1 and t.stride(0) >= t.size(1) else t.contiguous()


class _SpatialSoftmax3D(torch.autograd.Function):
    """feature [B,C,D,H,W] -> (keypoints [B,3C], maxpool [B,C]), the two halves of one [B,4C] buffer."""

    @staticmethod
    def forward(ctx, feature, temperature, slices):
        feature = _ops.readable(feature)
        dev = feature.device
        B, C, D, H, W = feature.shape
        rows, n = B * C, D * H * W
        out = torch.empty(B, 4 * C, dtype=torch.float32, device=dev)
        stats = torch.empty(rows, STATS, dtype=torch.float32, device=dev)
        # the slice records: written by every forward before it reads them
        ws = _ops.workspace(dev, _lib.lib().mgs_spatial_softmax_workspace_bytes(rows, n))
        keypoints, maxpool = out[:, :3 * C], out[:, 3 * C:]
        _ops.call("mgs_spatial_softmax_forward", dev, rows, C, D, H, W, temperature, feature.data_ptr(),
                  keypoints.data_ptr(), out.stride(0), maxpool.data_ptr(), out.stride(0),
                  stats.data_ptr(), ws.data_ptr(), ws.numel(), slices)
        ctx.save_for_backward(feature, stats)
        ctx.temperature, ctx.slices = temperature, slices
        ctx.set_materialize_grads(False)
        return keypoints, maxpool

    @staticmethod
    def backward(ctx, g_keypoints, g_max):
        if g_keypoints is None and g_max is None:
            return None, None, None
        feature, stats = ctx.saved_tensors
        dev = feature.device
        B, C, D, H, W = feature.shape
        g_feature = torch.empty_like(feature)
        gk = gm = None
        if g_keypoints is not None:
            gk = _rows_by_stride(g_keypoints.to(torch.float32))
        if g_max is not None:
            gm = _rows_by_stride(g_max.to(torch.float32))
        _ops.call("mgs_spatial_softmax_backward", dev, B * C, C, D, H, W, ctx.temperature, feature.data_ptr(), stats.data_ptr(),
                  _ops.ptr(gk), gk.stride(0) if gk is not None else 0, _ops.ptr(gm), gm.stride(0) if gm is not None else 0,
                  g_feature.data_ptr(), ctx.slices)
        return g_feature, None, None


def _spatial_softmax3d(feature, temperature, slices=0):
    """(keypoints, maxpool); slices: 0 = the library's split of a row over workgroups, 1..64 = that many (a test aid)."""
    if not isinstance(feature, torch.Tensor) or not feature.is_cuda or feature.dtype != torch.float32:
        raise RuntimeError(f"spatial_softmax3d needs a float32 tensor on a HIP device (feature is "
                           f"{getattr(feature, 'dtype', type(feature))} on {getattr(feature, 'device', 'the host')}); "
                           "there is no CPU path")
    if feature.dim() != 5 or feature.numel() == 0:
        raise ValueError(f"expected feature [B,C,D,H,W] with no empty dimension, got {tuple(feature.shape)}")
    temperature = float(temperature)
    if not (temperature > 0.0 and np.isfinite(temperature)):
        raise ValueError(f"temperature = {temperature}: must be positive and finite")
    return _SpatialSoftmax3D.apply(feature, temperature, int(slices))


def spatial_softmax3d(feature, temperature=0.01, with_max=False):
    """feature [B,C,D,H,W], fp32 on a HIP device -> keypoints [B,3C] (channel c's expected (x, y, z) at columns 3c..3c+2, in the
    reference's position tables), or with_max: (keypoints, maxpool [B,C]), the two halves of one [B,4C] buffer."""
    keypoints, maxpool = _spatial_softmax3d(feature, temperature)
    return (keypoints, maxpool) if with_max else keypoints


class SpatialSoftmax3D(nn.Module):
    """helpers/network_utils.py:927's SpatialSoftmax3D."""

    def __init__(self, depth, height, width, channel):
        super().__init__()
        self.depth = depth
        self.height = height
        self.width = width
        self.channel = channel
        self.temperature = 0.01
        pos_x, pos_y, pos_z = np.meshgrid(np.linspace(-1., 1., self.depth), np.linspace(-1., 1., self.height),
                                          np.linspace(-1., 1., self.width))
        n = self.depth * self.height * self.width
        self.register_buffer("pos_x", torch.from_numpy(pos_x.reshape(n)).float())
        self.register_buffer("pos_y", torch.from_numpy(pos_y.reshape(n)).float())
        self.register_buffer("pos_z", torch.from_numpy(pos_z.reshape(n)).float())

    def _checked(self, feature):
        want = (self.channel, self.depth, self.height, self.width)
        if not isinstance(feature, torch.Tensor) or feature.dim() != 5 or tuple(feature.shape[1:]) != want:
            raise ValueError(f"feature {tuple(getattr(feature, 'shape', ()))} does not match the module's [B, {want[0]}, {want[1]}, "
                             f"{want[2]}, {want[3]}] (channel, depth, height, width)")
        return feature

    def forward(self, feature):
        """[B,C,D,H,W] -> keypoints [B,3C]."""
        return spatial_softmax3d(self._checked(feature), self.temperature)

    def forward_with_max(self, feature):
        """[B,C,D,H,W] -> (keypoints [B,3C], maxpool [B,C]): `ss(x)` and `global_maxp(x).view(b, -1)` from one read of x."""
        return spatial_softmax3d(self._checked(feature), self.temperature, with_max=True)
