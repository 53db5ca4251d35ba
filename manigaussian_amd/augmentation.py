"""The agent's SE(3) augmentation (voxel/augmentation.py:11-377), fused and without a host read.

Reference: `apply_se3_augmentation_with_camera_pose`, called by agents/manigaussian_bc/qattention_manigaussian_bc_agent.py:751-767
and on by default (conf/method/ManiGaussian_BC.yaml:61-65).  There it is a Python rejection loop: every attempt draws a
perturbation on the CPU, composes it with the gripper pose on the device, reads the device back (at least 3 + 2 B reads per
attempt, up to 10 attempts -- derived from the code, not measured), discretises sample by sample with numpy and scipy, and on
success transforms every camera's cloud with a dozen torch ops.  Here it is two launches of csrc/mgs_augment.hip whatever the
batch, the camera count or the attempts: `select` evaluates all attempts side by side and picks, `apply` transforms all clouds and
camera poses.  No device read, no host loop, deterministic, capturable into a HIP graph.  The ops are small: what this buys is the
removed synchronisation, not bandwidth.

`apply_se3_augmentation_with_camera_pose` and `apply_se3_augmentation` keep the reference's argument order and return tuples;
`Se3Augmentation` is the module behind them.  The values are the reference's (include/mgsplat.h states every step's precision:
fp32 where torch runs it, fp64 where numpy and scipy run it) for the same draws.  What differs:
  * the random stream is the library's own counter-based one (Philox4x32-10 of (seed, offset, attempt, sample)), as with the
    attention dropout: the same torch seed gives other perturbations than the reference's run.  Seed and offset live in a device
    buffer of the module (`rng_state`, int64 [2], not in state_dict()); every call that draws advances the offset by an in-place
    device add, so a replayed graph draws afresh.  `draws` injects a table instead (tests);
  * inputs are never modified: the reference overwrites the tensors of `camera_pose` in place, this returns new ones;
  * the actions come back as int64 on every path, the identity path included (the reference hands its int32 inputs back there);
  * retry="sample" (opt-in, not the reference's): every sample takes its own first valid attempt;
  * fp32 HIP tensors only: there is no CPU path.
"""
import ctypes
import math

import torch
from torch import nn

from . import _lib, _ops

MAX_CAMERAS = _lib.SE3_MAX_SOURCES
MAX_BATCH = _lib.SE3_MAX_BATCH
MAX_ATTEMPTS = _lib.SE3_MAX_ATTEMPTS
RETRY = ("batch", "sample")


def workspace_bytes(B):
    """Bytes of the scratch `select` leaves for `apply` (one transform record per sample); 0: B is beyond the library's limit."""
    return _lib.lib().mgs_se3_workspace_bytes(int(B))


def _as_int64(v):
    v = int(v) & 0xFFFFFFFFFFFFFFFF
    return v - (1 << 64) if v >= (1 << 63) else v


def _triple(v, name):
    if torch.is_tensor(v):
        v = v.detach().reshape(-1).tolist()
    elif not isinstance(v, (list, tuple)):
        v = [v]
    v = [float(x) for x in v]
    if len(v) == 1:
        v = v * 3
    if len(v) != 3:
        raise ValueError(f"{name} must hold 1 or 3 values, got {len(v)}")
    return tuple(v)


def _planar(t):
    """A [B,3,H,W] fp32 cloud as (tensor, sample stride, plane stride): itself when its planes are contiguous (a channel slice of
    a wider tensor, a batch slice, an expand over the batch), else a contiguous copy (channel-last, strided pixels)."""
    B, _, H, W = t.shape
    sb, sc, sh, sw = t.stride()
    rows_ok = (sw == 1 or W == 1) and (sh == W or H == 1)
    if not (rows_ok and sc >= H * W and sb >= 0):
        t = t.contiguous()
        sb, sc = t.stride(0), t.stride(1)
    return t, sb, max(sc, H * W)


def se3_draws(attempts, B, rot_steps, rng_state):
    """The draws `select` takes for this (seed, offset): fp32 [attempts,B,6] = trans_u in [-1,1)^3, then the roll, pitch and yaw
    steps (integers in [-k,k] as floats; 0 where k = 0).  A test and debug aid; its result can be passed back as `draws`."""
    if not rng_state.is_cuda or rng_state.dtype != torch.int64 or rng_state.numel() != 2 or not rng_state.is_contiguous():
        raise ValueError("rng_state must be a contiguous int64 tensor (seed, offset) on a HIP device")
    a = _lib.MgsSe3Args()
    a.B, a.attempts = int(B), int(attempts)
    a.rot_steps[:] = [int(k) for k in rot_steps]
    a.rng_state = rng_state.data_ptr()
    out = torch.empty(a.attempts, a.B, 6, dtype=torch.float32, device=rng_state.device)
    _ops.call("mgs_se3_draws", rng_state.device, ctypes.byref(a), out.data_ptr())
    return out


class Se3Augmentation(nn.Module):
    """The augmentation with its configuration bound: no parameters, one buffer (`rng_state`) that is not in state_dict().

    trans_aug_range: 1 or 3 fractions of the bounds' range (a float64 tensor, as the agent builds it from its config, a float32
    tensor -- then the translation is composed in fp32 throughout, as torch would -- or plain numbers, taken as float64);
    rot_aug_range: 3 angles in degrees, drawn in steps of rot_aug_resolution; voxel_size, rot_resolution: the discretisation;
    layer > 0: sample b is discretised against row b of the bounds, else against row 0 (the reference's `bounds_idx`).
    `last_info` after a call: int32 device tensor [1 + B], the first attempt valid for the whole batch and the attempt every
    sample took, -1 for the identity."""

    def __init__(self, trans_aug_range, rot_aug_range, rot_aug_resolution, voxel_size, rot_resolution, layer=0, attempts=10,
                 retry="batch"):
        super().__init__()
        if retry not in RETRY:
            raise ValueError(f"retry must be one of {RETRY}, got {retry!r}")
        if not 1 <= int(attempts) <= MAX_ATTEMPTS:
            raise ValueError(f"attempts = {attempts} outside 1 .. {MAX_ATTEMPTS}")
        if int(voxel_size) < 1 or not rot_resolution > 0 or not rot_aug_resolution > 0:
            raise ValueError(f"voxel_size {voxel_size}, rot_resolution {rot_resolution} and rot_aug_resolution "
                             f"{rot_aug_resolution} must be positive")
        self.trans_f64 = not (torch.is_tensor(trans_aug_range) and trans_aug_range.dtype != torch.float64)
        self.trans_aug_range = _triple(trans_aug_range, "trans_aug_range")
        rot = _triple(rot_aug_range, "rot_aug_range")
        self.rot_steps = tuple(int(r // rot_aug_resolution) for r in rot)
        if min(self.rot_steps) < 0:
            raise ValueError(f"rot_aug_range {rot} must not be negative")
        self.rot_aug_resolution = rot_aug_resolution
        self.voxel_size, self.rot_resolution = int(voxel_size), rot_resolution
        self.layer, self.attempts, self.retry = int(layer), int(attempts), retry
        self.register_buffer("rng_state", torch.zeros(2, dtype=torch.int64), persistent=False)
        self._seeded = False
        self.last_info = None

    def manual_seed(self, seed, offset=0):
        """Restart the module's stream at (seed, offset)."""
        self.rng_state.copy_(torch.tensor([_as_int64(seed), _as_int64(offset)], dtype=torch.int64))
        self._seeded = True
        return self

    def _args(self, B):
        a = _lib.MgsSe3Args()
        a.B, a.attempts, a.retry, a.layer, a.voxel_size = B, self.attempts, RETRY.index(self.retry), self.layer, self.voxel_size
        a.rot_bins = int(360 / self.rot_resolution)
        a.trans_f64 = int(self.trans_f64)
        a.rot_steps[:] = self.rot_steps
        a.rot_step_rad = math.radians(self.rot_aug_resolution)
        a.rot_resolution = float(self.rot_resolution)
        a.trans_aug_range[:] = self.trans_aug_range
        return a

    def forward(self, pcd, camera_pose, action_gripper_pose, action_trans, action_rot_grip, bounds, draws=None):
        """pcd: list of [B,3,H,W] clouds, one per camera (read in place by strides where their planes are contiguous);
        camera_pose: list of [B,4,4] (or None); action_gripper_pose [B,7] (translation, quaternion xyzw); action_trans [B,3] and
        action_rot_grip [B,4], int32 or int64; bounds [1,6] or [B,6]; draws: fp32 [attempts,B,6] to take in place of the stream.
        -> (action_trans int64 [B,3], action_rot_grip int64 [B,4], list of new clouds, list of new poses)."""
        pcd = list(pcd)
        poses = list(camera_pose) if camera_pose is not None else []
        if not pcd or len(pcd) > MAX_CAMERAS or len(poses) > MAX_CAMERAS:
            raise ValueError(f"expected 1 .. {MAX_CAMERAS} clouds and at most as many camera poses, got {len(pcd)} and {len(poses)}")
        B = pcd[0].size(0)
        shapes = f"clouds {[tuple(t.shape) for t in pcd]}, poses {[tuple(t.shape) for t in poses]}, gripper pose " \
                 f"{tuple(action_gripper_pose.shape)}, action_trans {tuple(action_trans.shape)}, action_rot_grip " \
                 f"{tuple(action_rot_grip.shape)}"
        if any(t.dim() != 4 or t.size(0) != B or t.size(1) != 3 or t.size(2) * t.size(3) < 1 for t in pcd) or \
                any(t.shape != (B, 4, 4) for t in poses) or action_gripper_pose.shape != (B, 7) or \
                action_trans.shape != (B, 3) or action_rot_grip.shape != (B, 4):
            raise ValueError(f"expected clouds [B,3,H,W], poses [B,4,4], a gripper pose [B,7], action_trans [B,3] and "
                             f"action_rot_grip [B,4] of one batch size, got {shapes}")
        if B > MAX_BATCH:
            raise ValueError(f"batch size {B} is above the library's {MAX_BATCH} ({shapes})")
        if any(t.size(2) * t.size(3) > (1 << 24) for t in pcd):
            raise ValueError(f"a cloud of more than 2^24 points per sample ({shapes})")
        n_bounds = torch.as_tensor(bounds).reshape(-1, 6).size(0)
        if n_bounds not in (1, B):
            raise ValueError(f"bounds hold {n_bounds} rows for a batch of {B}")
        if draws is not None and (draws.shape != (self.attempts, B, 6) or draws.dtype != torch.float32):
            raise ValueError(f"draws must be float32 [{self.attempts}, {B}, 6], got {draws.dtype} {tuple(draws.shape)}")
        for name, t in [("pcd", t) for t in pcd] + [("camera_pose", t) for t in poses] + \
                [("action_gripper_pose", action_gripper_pose), ("action_trans", action_trans),
                 ("action_rot_grip", action_rot_grip)] + ([("draws", draws)] if draws is not None else []):
            if not t.is_cuda:
                raise RuntimeError(f"the SE(3) augmentation needs tensors on a HIP device ({name} is on {t.device}); "
                                   "there is no CPU path")
        if any(t.dtype != torch.float32 for t in pcd):
            raise RuntimeError(f"the SE(3) augmentation needs float32 clouds, got {[t.dtype for t in pcd]}; there is no other path")
        dev = pcd[0].device
        if self.rng_state.device != dev:
            self.rng_state = self.rng_state.to(dev)
        if draws is None and not self._seeded:
            self.manual_seed(torch.initial_seed())

        grip = action_gripper_pose.detach().to(torch.float32).contiguous()
        acts = [t.detach() if t.dtype in (torch.int32, torch.int64) else t.detach().to(torch.int64)
                for t in (action_trans, action_rot_grip)]
        if acts[0].dtype != acts[1].dtype:
            acts = [t.to(torch.int64) for t in acts]
        acts = [t.contiguous() for t in acts]
        bd = torch.as_tensor(bounds, dtype=torch.float32, device=dev).detach().reshape(-1, 6).contiguous()
        srcs = [_planar(t.detach()) for t in pcd]
        pin = [t.detach().to(torch.float32).contiguous() for t in poses]
        if draws is not None:
            draws = draws.detach().contiguous()

        out_trans = torch.empty(B, 3, dtype=torch.int64, device=dev)
        out_rot = torch.empty(B, 4, dtype=torch.int64, device=dev)
        info = torch.empty(1 + B, dtype=torch.int32, device=dev)
        outs = [torch.empty(t.shape, dtype=torch.float32, device=dev) for t in pcd]
        pout = [torch.empty(B, 4, 4, dtype=torch.float32, device=dev) for _ in pin]
        ws = _ops.workspace(dev, workspace_bytes(B))

        a = self._args(B)
        a.bounds_rows, a.action_i64 = bd.size(0), int(acts[0].dtype == torch.int64)
        a.gripper_pose, a.action_trans, a.action_rot_grip, a.bounds = grip.data_ptr(), acts[0].data_ptr(), acts[1].data_ptr(), bd.data_ptr()
        a.rng_state = self.rng_state.data_ptr()
        a.draws = draws.data_ptr() if draws is not None else None
        a.n_sources, a.n_poses = len(srcs), len(pin)
        for i, ((t, sb, sc), o) in enumerate(zip(srcs, outs)):
            a.src[i], a.dst[i], a.n_points[i], a.stride_b[i], a.stride_c[i] = t.data_ptr(), o.data_ptr(), t.size(2) * t.size(3), sb, sc
        for i, (t, o) in enumerate(zip(pin, pout)):
            a.pose_in[i], a.pose_out[i] = t.data_ptr(), o.data_ptr()
        _ops.call("mgs_se3_select", dev, ctypes.byref(a), out_trans.data_ptr(), out_rot.data_ptr(), info.data_ptr(),
                  ws.data_ptr(), ws.numel())
        _ops.call("mgs_se3_apply", dev, ctypes.byref(a), ws.data_ptr(), ws.numel())
        if draws is None:
            self.rng_state[1:].add_(1)  # (after the launch that read it, in stream order)
        self.last_info = info
        return out_trans, out_rot, outs, pout


_CACHED = {}  # (device, configuration) -> the Se3Augmentation the drop-in functions use


def _cached(device, layer, trans_aug_range, rot_aug_range, rot_aug_resolution, voxel_size, rot_resolution):
    f64 = not (torch.is_tensor(trans_aug_range) and trans_aug_range.dtype != torch.float64)
    key = (str(device), int(layer), f64, _triple(trans_aug_range, "trans_aug_range"), _triple(rot_aug_range, "rot_aug_range"),
           rot_aug_resolution, int(voxel_size), rot_resolution)
    m = _CACHED.get(key)
    if m is None:
        m = _CACHED[key] = Se3Augmentation(trans_aug_range, rot_aug_range, rot_aug_resolution, voxel_size, rot_resolution,
                                           layer=layer)
    return m


def apply_se3_augmentation_with_camera_pose(pcd, camera_pose, action_gripper_pose, action_trans, action_rot_grip, bounds, layer,
                                            trans_aug_range, rot_aug_range, rot_aug_resolution, voxel_size, rot_resolution,
                                            device):
    """voxel/augmentation.py:256's function, its arguments in its order -> (action_trans, action_rot_grip, pcd, camera_pose).
    The configuration is read on the host at every call (it keys the cached module): hand trans_aug_range over as the agent
    does, a CPU tensor or a list -- a device tensor there would cost the read this module exists to avoid."""
    m = _cached(pcd[0].device if len(pcd) else device, layer, trans_aug_range, rot_aug_range, rot_aug_resolution, voxel_size,
                rot_resolution)
    return m(pcd, camera_pose, action_gripper_pose, action_trans, action_rot_grip, bounds)


def apply_se3_augmentation(pcd, action_gripper_pose, action_trans, action_rot_grip, bounds, layer, trans_aug_range,
                           rot_aug_range, rot_aug_resolution, voxel_size, rot_resolution, device):
    """voxel/augmentation.py:134's function (no cameras) -> (action_trans, action_rot_grip, pcd)."""
    m = _cached(pcd[0].device if len(pcd) else device, layer, trans_aug_range, rot_aug_range, rot_aug_resolution, voxel_size,
                rot_resolution)
    return m(pcd, None, action_gripper_pose, action_trans, action_rot_grip, bounds)[:3]
