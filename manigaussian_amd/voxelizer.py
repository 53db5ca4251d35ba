"""The agent's voxel grid: the point cloud scatter-meaned into V^3 voxels, fused and deterministic.

Reference: voxel/voxel_grid.py:15-229 (VoxelGrid, coords_to_bounding_voxel_grid), called by
agents/manigaussian_bc/qattention_manigaussian_bc_agent.py:217 and :313 on the flattened camera clouds (:205-214).
`VoxelGrid` has the reference's constructor and method; `voxelize_images` takes the per-camera images as QFunction.forward
holds them and reads them in place.  Both return the reference's shapes and VALUES -- [B,V,V,V,Fc+7] =
[mean features | mean xyz | index / V | occupancy] -- and, on the same inputs, the bits of the reference module run on a CPU:
every voxel's points are added in ascending point index and divided once (csrc/mgs_voxelize.hip), so two runs give the
same grid, which the reference's scatter_add_ on a GPU does not promise.

Forward only: the reference detaches the grid (...agent.py:221) and its inputs are data.  The result never requires grad,
whatever the inputs do.  There is no CPU path.

memory="channels_first" (default): the result is a permuted view of a contiguous [B,C,V,V,V] buffer, so the caller's unchanged
`voxel_grid.permute(0, 4, 1, 2, 3)` is contiguous and Conv3d copies nothing.  memory="channels_last": contiguous
[B,V,V,V,C], the reference's layout.
"""
import torch
from torch import nn

from . import _lib, _ops

MEMORY = ("channels_first", "channels_last")
MAX_FEATURES = 64  # MGS_VOXELIZE_MAX_FEATURES
MAX_IMAGES = 8     # MGS_VOXELIZE_MAX_SOURCES

_WS_BYTES = {}  # (B, N, V) -> bytes of the workspace; the library zeroes what it needs of it in every call


def _workspace(dev, B, N, V):
    n = _WS_BYTES.get((B, N, V))
    if n is None:
        n = _lib.lib().mgs_voxelize_workspace_bytes(B, N, V)
        if n == 0:
            raise ValueError(f"voxelizer: B = {B}, N = {N}, V = {V} is beyond the library's limits "
                             "(B <= 65536, N <= 2^24, B V^3 and B N below 2^31)")
        _WS_BYTES[B, N, V] = n
    return _ops.workspace(dev, n)


def _check_memory(memory):
    if memory not in MEMORY:
        raise ValueError(f"memory must be one of {MEMORY}, got {memory!r}")


def _data(t):
    return t.detach().float().contiguous()


def _bounds(bounds, B, dev):
    b = torch.as_tensor(bounds, dtype=torch.float32, device=dev).detach().reshape(-1, 6)
    if b.size(0) != B:
        if b.size(0) != 1:
            raise ValueError(f"coord_bounds holds {b.size(0)} rows for a batch of {B}")
        b = b.expand(B, 6)
    return b.contiguous()


def _alloc(B, V, C, memory, dev):
    shape = (B, C, V, V, V) if memory == "channels_first" else (B, V, V, V, C)
    return torch.empty(shape, dtype=torch.float32, device=dev)


def _as_reference(grid, memory):
    return grid.permute(0, 2, 3, 4, 1) if memory == "channels_first" else grid


def voxelize(coords, features, bounds, voxel_size, memory="channels_first"):
    """coords [B,N,3], features [B,N,Fc] or None, bounds [B,6] or [1,6] or [6] (a device tensor costs no copy)
    -> [B,V,V,V,Fc+7] (see the module's text for `memory`)."""
    _check_memory(memory)
    if not coords.is_cuda or (features is not None and not features.is_cuda):
        raise RuntimeError("the voxelizer needs tensors on a HIP device; there is no CPU path")
    if coords.dim() != 3 or coords.size(-1) != 3:
        raise ValueError(f"expected coords [B, N, 3], got {tuple(coords.shape)}")
    dev = coords.device
    B, N, V = coords.size(0), coords.size(1), int(voxel_size)
    Fc = 0 if features is None else features.size(-1)
    if features is not None and (features.dim() != 3 or features.shape[:2] != coords.shape[:2]):
        raise ValueError(f"expected features [{B}, {N}, Fc], got {tuple(features.shape)}")
    if Fc > MAX_FEATURES:
        raise ValueError(f"feature width {Fc} is above the library's {MAX_FEATURES}")
    pts = _data(coords)
    fts = _data(features) if Fc > 0 else None
    bd = _bounds(bounds, B, dev)
    ws = _workspace(dev, B, N, V)
    grid = _alloc(B, V, Fc + 7, memory, dev)
    _ops.call("mgs_voxelize_forward", dev, B, N, V, Fc, int(memory == "channels_first"), _ops.ptr(pts), _ops.ptr(fts),
              bd.data_ptr(), grid.data_ptr(), ws.data_ptr(), ws.numel())
    return _as_reference(grid, memory)


def voxelize_images(pcds, rgbs, bounds, voxel_size, memory="channels_first"):
    """The grid of the cloud that ...agent.py:205-214 flattens -- cat over cameras of pcd.permute(0, 2, 3, 1).reshape(B, -1, 3),
    features likewise -- read from the images in place: pcds, rgbs are lists of [B,3,H,W] and [B,Fc,H,W] tensors (one pair
    per camera, all of one size; rgbs None or empty: no features).  No torch kernel runs unless an image is not contiguous
    fp32 or the bounds are not a device tensor of B rows."""
    _check_memory(memory)
    pcds = list(pcds)
    rgbs = list(rgbs) if rgbs else []
    if not pcds or len(pcds) > MAX_IMAGES or (rgbs and len(rgbs) != len(pcds)):
        raise ValueError(f"expected 1 .. {MAX_IMAGES} point-cloud images and as many colour images, got {len(pcds)} and {len(rgbs)}")
    if not all(t.is_cuda for t in pcds + rgbs):
        raise RuntimeError("the voxelizer needs tensors on a HIP device; there is no CPU path")
    B, three, H, W = pcds[0].shape
    Fc = rgbs[0].size(1) if rgbs else 0
    if three != 3 or any(t.shape != (B, 3, H, W) for t in pcds) or any(t.shape != (B, Fc, H, W) for t in rgbs):
        raise ValueError("every point-cloud image must be [B,3,H,W] and every colour image [B,Fc,H,W] of the same B, H, W")
    if Fc > MAX_FEATURES:
        raise ValueError(f"feature width {Fc} is above the library's {MAX_FEATURES}")
    dev, V, n = pcds[0].device, int(voxel_size), len(pcds)
    pts = [_data(t) for t in pcds]
    fts = [_data(t) for t in rgbs]
    bd = _bounds(bounds, B, dev)
    ws = _workspace(dev, B, n * H * W, V)
    grid = _alloc(B, V, Fc + 7, memory, dev)
    cp = (_lib.c_fp * n)(*[t.data_ptr() for t in pts])
    fp = (_lib.c_fp * n)(*[t.data_ptr() for t in fts]) if Fc > 0 else None
    _ops.call("mgs_voxelize_forward_images", dev, B, n, H * W, V, Fc, int(memory == "channels_first"), cp, fp,
              bd.data_ptr(), grid.data_ptr(), ws.data_ptr(), ws.numel())
    return _as_reference(grid, memory)


class VoxelGrid(nn.Module):
    """voxel/voxel_grid.py's VoxelGrid: the reference's constructor arguments in the reference's order, plus `memory`.
    No parameters and no buffers: state_dict() is empty (the reference's loader ignores `_voxelizer` keys,
    ...agent.py:1222).  batch_size is kept for the signature only: the grid follows the batch of the coords it is given."""

    def __init__(self, coord_bounds, voxel_size: int, device, batch_size, feature_size, max_num_coords: int,
                 memory="channels_first"):
        super().__init__()
        _check_memory(memory)
        if not 0 <= int(feature_size) <= MAX_FEATURES:
            raise ValueError(f"feature_size {feature_size} outside 0 .. {MAX_FEATURES}")
        self._device = device
        self._voxel_size = int(voxel_size)
        self._batch_size = batch_size
        self._feature_size = int(feature_size)
        self._num_coords = int(max_num_coords)
        self._memory = memory
        self._coord_bounds_host = torch.tensor(coord_bounds, dtype=torch.float).reshape(1, 6)
        self._coord_bounds = None  # the constructor's bounds on the device of the first call (not a buffer: no state)

    def _own_bounds(self, dev):
        if self._coord_bounds is None or self._coord_bounds.device != dev:
            self._coord_bounds = self._coord_bounds_host.to(dev)
        return self._coord_bounds

    def coords_to_bounding_voxel_grid(self, coords, coord_features=None, coord_bounds=None, only_features=False,
                                      return_density=False):
        width = 0 if coord_features is None else coord_features.size(-1)
        if width != self._feature_size:
            raise ValueError(f"coord_features are {width} wide, this VoxelGrid was built with feature_size {self._feature_size}")
        if coords.size(1) > self._num_coords:
            raise ValueError(f"{coords.size(1)} points, this VoxelGrid was built with max_num_coords {self._num_coords}")
        if not coords.is_cuda or (coord_features is not None and not coord_features.is_cuda):
            raise RuntimeError("VoxelGrid needs tensors on a HIP device; there is no CPU path")
        bounds = self._own_bounds(coords.device) if coord_bounds is None else coord_bounds
        vox = voxelize(coords, coord_features, bounds, self._voxel_size, self._memory)
        if only_features:
            return vox[..., :-7]
        if return_density:
            return vox, vox[..., -1:]
        return vox
