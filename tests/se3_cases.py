"""The SE(3) augmentation's truth -- TEST INFRASTRUCTURE (tests/test_augmentation.py, tests/golden/make_golden_se3.py,
tests/tools/se3_graph_capture_check.py).

The truth is the reference itself: helpers/utils.py and voxel/augmentation.py are loaded UNMODIFIED where the reference tree is
present ($MGS_REFERENCE_ROOT, default /root/reference) and executed on the CPU.  What the container lacks is stood in for:
  * pyrender, trimesh, rlbench, pyrep, termcolor: empty modules with the few names helpers/utils.py imports (never called);
  * pytorch3d.transforms: its three functions the augmentation calls -- quaternion_to_matrix (wxyz), euler_angles_to_matrix
    (.., "XYZ"), matrix_to_quaternion -- as scipy.spatial.transform.Rotation evaluated in float64 and cast to fp32.  The real
    pytorch3d computes them in fp32: it and the kernel differ from this stand-in by fp32 rounding, which is why the fixture
    generator keeps only cases whose every discretisation decision is at least MARGIN bins from its boundary;
  * utils.rand_dist / utils.rand_discrete: served from a draw table [attempts,B,6] in the reference's call order (per attempt one
    (bs,3) uniform, then roll, pitch, yaw; no draw where the step count is 0), so the reference and the kernel see the same draws.
utils.point_to_voxel_index and utils.quaternion_to_discrete_euler are wrapped (not changed) to record every decision's float64
distance to its boundary.

Without the reference tree `reference()` is None and the tests use the committed fixtures tests/golden/se3/*.npz.
"""
import glob
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "se3")
REF_ROOT = os.environ.get("MGS_REFERENCE_ROOT", "/root/reference")

ATTEMPTS = 10          # the reference's
VOXEL_SIZE = 100       # conf/method/ManiGaussian_BC.yaml
ROT_RESOLUTION = 5
ROT_AUG_RESOLUTION = 5
MARGIN = 1e-4          # bins: the least distance of a kept case's decisions from their boundaries
SCENE_BOUNDS = [-0.3, -0.5, 0.6, 0.7, 0.5, 1.6]

# name, B, H, W, cameras, bounds ("one": [1,6], layer 0 | "per": [B,6] of different rows, layer 1), rot_aug_range, trans_aug_range,
# construction ("": every sample well inside | "low": one sample within 0.01 of the lower bound, accepted at attempt 2 |
# "never": one sample 0.13 below the lower bound, never accepted | "above": one sample above the upper bound, valid and clamped)
CASES = [
    ("b1_4x4_c1", 1, 4, 4, 1, "one", [0, 0, 45], 0.125, ""),
    ("b3_5x7_c2", 3, 5, 7, 2, "one", [0, 0, 45], 0.125, ""),
    ("b8_4x4_c3", 8, 4, 4, 3, "one", [10, 15, 45], 0.125, ""),
    ("b3_5x7_c3_per", 3, 5, 7, 3, "per", [10, 15, 45], 0.125, ""),
    ("b8_5x7_c1_per", 8, 5, 7, 1, "per", [0, 0, 45], 0.125, ""),
    ("b3_4x4_c2_notrans", 3, 4, 4, 2, "one", [0, 0, 45], 0.0, ""),
    ("b1_5x7_c2_notrans_rpy", 1, 5, 7, 2, "one", [10, 15, 45], 0.0, ""),
    ("b3_5x7_c2_low", 3, 5, 7, 2, "one", [0, 0, 45], 0.125, "low"),
    ("b8_4x4_c1_low_rpy", 8, 4, 4, 1, "one", [10, 15, 45], 0.125, "low"),
    ("b3_4x4_c3_never", 3, 4, 4, 3, "one", [0, 0, 45], 0.125, "never"),
    ("b1_5x7_c1_never", 1, 5, 7, 1, "one", [10, 15, 45], 0.125, "never"),
    ("b8_5x7_c2_above", 8, 5, 7, 2, "one", [0, 0, 45], 0.125, "above"),
]


# ---- the reference, executed in place ----------------------------------------------------------------------------------------
class _Empty(types.ModuleType):
    """A stand-in module: any name it is asked for is `object` (annotations and imports resolve; nothing is ever called)."""

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return object


def _stub(name, **attrs):
    if name not in sys.modules:
        m = _Empty(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
    return sys.modules[name]


def _rotation():
    from scipy.spatial.transform import Rotation
    return Rotation


def _quaternion_to_matrix(q):
    wxyz = q.detach().cpu().double().numpy()
    m = _rotation().from_quat(np.concatenate([wxyz[..., 1:], wxyz[..., :1]], -1)).as_matrix()
    return torch.from_numpy(m).to(dtype=q.dtype, device=q.device)


def _euler_angles_to_matrix(angles, convention):
    assert convention == "XYZ"
    m = _rotation().from_euler("XYZ", angles.detach().cpu().double().numpy()).as_matrix()
    return torch.from_numpy(m).to(dtype=angles.dtype, device=angles.device)


def _matrix_to_quaternion(m):
    xyzw = _rotation().from_matrix(m.detach().cpu().double().numpy()).as_quat()
    return torch.from_numpy(np.concatenate([xyzw[..., 3:], xyzw[..., :3]], -1)).to(dtype=m.dtype, device=m.device)


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


_REF = []


def have_reference():
    return os.path.isfile(os.path.join(REF_ROOT, "voxel", "augmentation.py")) and \
        os.path.isfile(os.path.join(REF_ROOT, "helpers", "utils.py"))


def reference():
    """(the reference's voxel.augmentation module, its helpers.utils module), or None without the reference tree."""
    if _REF:
        return _REF[0]
    if not have_reference():
        return None
    _stub("termcolor", colored=lambda s, *a, **k: s, cprint=lambda *a, **k: None)
    _stub("trimesh")
    pr = _stub("pyrender")
    pr.trackball = _stub("pyrender.trackball", Trackball=object)
    rl = _stub("rlbench", CameraConfig=object, ObservationConfig=object)
    rl.backend = _stub("rlbench.backend")
    rl.backend.const = _stub("rlbench.backend.const", DEPTH_SCALE=2 ** 24 - 1)
    rl.backend.observation = _stub("rlbench.backend.observation", Observation=object)
    pp = _stub("pyrep")
    pp.const = _stub("pyrep.const", RenderMode=object)
    p3 = _stub("pytorch3d")
    p3.transforms = _stub("pytorch3d.transforms", quaternion_to_matrix=_quaternion_to_matrix,
                          euler_angles_to_matrix=_euler_angles_to_matrix, matrix_to_quaternion=_matrix_to_quaternion)
    helpers = _stub("helpers")
    helpers.__path__ = []
    utils = _load("helpers.utils", os.path.join(REF_ROOT, "helpers", "utils.py"))
    helpers.utils = utils
    aug = _load("_mgs_reference_voxel_augmentation", os.path.join(REF_ROOT, "voxel", "augmentation.py"))
    _REF.append((aug, utils))
    return _REF[0]


class _Served:
    """utils.rand_dist / rand_discrete from a draw table, and the margins of every discretisation decision."""

    def __init__(self, utils, table):
        self.utils, self.table = utils, table
        self.attempt, self.axis = -1, 0
        self.margins = []  # (attempt, float64 distance to the nearest decision boundary, in bins)

    def rand_dist(self, size, min=-1.0, max=1.0):
        self.attempt += 1
        self.axis = 0
        assert tuple(size) == (self.table.shape[1], 3) and (min, max) == (-1.0, 1.0)
        return torch.from_numpy(self.table[self.attempt, :, 0:3].astype(np.float32))

    def rand_discrete(self, size, min=0, max=1):
        i = self.axis
        self.axis += 1
        if min == max:
            return torch.zeros(size)
        steps = self.table[self.attempt, :, 3 + i]
        assert tuple(size) == (self.table.shape[1], 1) and np.all(steps == np.round(steps)) and np.all(np.abs(steps) <= max)
        return torch.from_numpy(steps.astype(np.int64)).reshape(size)

    def point_to_voxel_index(self, point, voxel_size, coord_bounds):
        bb_mins, bb_maxs = np.array(coord_bounds[0:3]), np.array(coord_bounds[3:])
        res = (bb_maxs - bb_mins) / (np.array([voxel_size] * 3) + 1e-12)
        x = ((point - bb_mins) / (res + 1e-12)).astype(np.float64)
        for v in x:
            if v < voxel_size:  # (at and above V the index is clamped: no decision)
                self.margins.append((self.attempt, float(abs(v - np.round(v)))))
        return self._point_to_voxel_index(point, voxel_size, coord_bounds)

    def quaternion_to_discrete_euler(self, quaternion, resolution):
        euler = _rotation().from_quat(quaternion).as_euler("xyz", degrees=True) + 180
        y = euler / resolution
        for v in y:
            self.margins.append((self.attempt, float(abs((v - np.floor(v)) - 0.5))))
        return self._quaternion_to_discrete_euler(quaternion, resolution)

    def __enter__(self):
        u = self.utils
        self._saved = (u.rand_dist, u.rand_discrete, u.point_to_voxel_index, u.quaternion_to_discrete_euler)
        self._point_to_voxel_index, self._quaternion_to_discrete_euler = u.point_to_voxel_index, u.quaternion_to_discrete_euler
        u.rand_dist, u.rand_discrete = self.rand_dist, self.rand_discrete
        u.point_to_voxel_index, u.quaternion_to_discrete_euler = self.point_to_voxel_index, self.quaternion_to_discrete_euler
        return self

    def __exit__(self, *a):
        u = self.utils
        u.rand_dist, u.rand_discrete, u.point_to_voxel_index, u.quaternion_to_discrete_euler = self._saved


def trans_aug_tensor(value):
    """trans_aug_range as the agent hands it over: a float64 tensor built from a numpy array of its config list."""
    return torch.from_numpy(np.array([value] * 3))


def run_reference(inp, table, rows=None):
    """The reference on a case's inputs (dict of numpy arrays, see make_inputs) with the draws of `table`; rows: None for the
    batch, or a sample index for the single-sample call with that sample's rows.  -> dict(trans int64 [B,3], rot_grip int64
    [B,4], attempt (-1: identity), pcd list, pose list, margin: the least margin of the decisions up to the chosen attempt)."""
    aug, utils = reference()
    sel = slice(None) if rows is None else slice(rows, rows + 1)
    bounds = inp["bounds"] if inp["bounds"].shape[0] == 1 else inp["bounds"][sel]
    pcd = [torch.from_numpy(p[sel].copy()) for p in inp["pcd"]]
    poses = [torch.from_numpy(p[sel].copy()) for p in inp["pose"]]
    a_trans, a_rot = torch.from_numpy(inp["action_trans"][sel].copy()), torch.from_numpy(inp["action_rot_grip"][sel].copy())
    with _Served(utils, table[:, sel]) as served:
        t, r, out_pcd, out_pose = aug.apply_se3_augmentation_with_camera_pose(
            pcd, poses, torch.from_numpy(inp["gripper"][sel].copy()), a_trans, a_rot, torch.from_numpy(bounds.copy()),
            int(inp["layer"]), trans_aug_tensor(float(inp["trans_aug_range"])), [float(v) for v in inp["rot_aug_range"]],
            ROT_AUG_RESOLUTION, VOXEL_SIZE, ROT_RESOLUTION, "cpu")
    identity = t is a_trans
    attempt = -1 if identity else served.attempt
    assert identity or (t.dtype == torch.int64 and r.dtype == torch.int64)
    used = [m for a, m in served.margins if identity or a <= attempt]
    return dict(trans=t.to(torch.int64).numpy(), rot_grip=r.to(torch.int64).numpy(), attempt=attempt,
                pcd=[p.numpy() for p in out_pcd], pose=[p.numpy() for p in out_pose], margin=min(used), decisions=len(used), close=sum(m < MARGIN for m in used))


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def make_inputs(spec, seed):
    """A case's inputs and draw table (numpy), from its row of CASES and a seed."""
    name, B, H, W, cams, bmode, rot_aug, trans_aug, special = spec
    rng = np.random.default_rng(seed)
    base = np.array(SCENE_BOUNDS, dtype=np.float32)
    if bmode == "per":
        bounds = base[None] + rng.uniform(-0.05, 0.05, (B, 6)).astype(np.float32)
    else:
        bounds = base[None].copy()
    rows = bounds if bmode == "per" else np.repeat(bounds, B, 0)
    lo, hi = rows[:, :3], rows[:, 3:]
    gripper = np.zeros((B, 7), dtype=np.float32)
    gripper[:, :3] = lo + (hi - lo) * rng.uniform(0.2, 0.8, (B, 3)).astype(np.float32)
    pitch = 60.0 if rot_aug[1] else 80.0  # (scipy's Euler extraction is unstable at the gimbal pole)
    eul = np.stack([rng.uniform(-180, 180, B), rng.uniform(-pitch, pitch, B), rng.uniform(-180, 180, B)], 1)
    quat = _rotation().from_euler("xyz", eul, degrees=True).as_quat() * rng.choice([-1.0, 1.0], (B, 1))
    gripper[:, 3:] = quat.astype(np.float32)
    k = [int(r // ROT_AUG_RESOLUTION) for r in rot_aug]
    table = np.zeros((ATTEMPTS, B, 6), dtype=np.float32)
    table[..., :3] = (2.0 * rng.random((ATTEMPTS, B, 3), dtype=np.float32) - 1.0).astype(np.float32)
    for i in range(3):
        table[..., 3 + i] = rng.integers(-k[i], k[i] + 1, (ATTEMPTS, B)) if k[i] else 0
    s = B - 1  # the constructed sample
    if special == "low":
        gripper[s, 0] = lo[s, 0] + 0.005
        table[0:2, s, 0] = -np.abs(table[0:2, s, 0]) - np.float32(0.1)
        table[2, s, 0] = np.abs(table[2, s, 0]) * np.float32(0.5) + np.float32(0.25)
        table[..., 0] = np.clip(table[..., 0], -1.0, np.float32(1.0 - 2.0 ** -23))
    elif special == "never":
        gripper[s, 0] = lo[s, 0] - 0.13
    elif special == "above":
        gripper[s, 2] = hi[s, 2] + 0.05
        table[0, s, 2] = 0.6
    ext_lo, ext_hi = rows[:, :3].min(0) - 0.2, rows[:, 3:].max(0) + 0.2
    pcd = [(ext_lo[None, :, None, None] + (ext_hi - ext_lo)[None, :, None, None] *
            rng.random((B, 3, H, W), dtype=np.float32)).astype(np.float32) for _ in range(cams)]
    pose = []
    for _ in range(cams):
        m = np.zeros((B, 4, 4), dtype=np.float32)
        m[:, :3, :3] = _rotation().random(B, random_state=int(rng.integers(1 << 30))).as_matrix().astype(np.float32)
        m[:, :3, 3] = rng.uniform(-2, 2, (B, 3)).astype(np.float32)
        m[:, 3, 3] = 1
        pose.append(m)
    action_trans = rng.integers(0, VOXEL_SIZE, (B, 3)).astype(np.int32)
    action_rot_grip = np.concatenate([rng.integers(0, 360 // ROT_RESOLUTION, (B, 3)), rng.integers(0, 2, (B, 1))], 1).astype(np.int32)
    inp = dict(bounds=bounds, gripper=gripper, pcd=pcd, pose=pose, action_trans=action_trans, action_rot_grip=action_rot_grip,
               layer=np.int64(1 if bmode == "per" else 0), trans_aug_range=np.float64(trans_aug),
               rot_aug_range=np.array(rot_aug, dtype=np.float64))
    return inp, table


def build_case(spec, seed):
    """Inputs, draws and the reference's results (batch call and one single-sample call per sample) as one flat dict of arrays."""
    inp, table = make_inputs(spec, seed)
    B = inp["gripper"].shape[0]
    ref = run_reference(inp, table)
    per = [run_reference(inp, table, rows=b) for b in range(B)]
    out = dict(seed=np.int64(seed), draws=table, bounds=inp["bounds"], gripper=inp["gripper"], action_trans=inp["action_trans"],
               action_rot_grip=inp["action_rot_grip"], layer=inp["layer"], trans_aug_range=inp["trans_aug_range"],
               rot_aug_range=inp["rot_aug_range"], n_cams=np.int64(len(inp["pcd"])),
               exp_trans=ref["trans"], exp_rot_grip=ref["rot_grip"], exp_attempt=np.int64(ref["attempt"]),
               s_trans=np.concatenate([p["trans"] for p in per]), s_rot_grip=np.concatenate([p["rot_grip"] for p in per]),
               s_attempt=np.array([p["attempt"] for p in per], dtype=np.int64),
               margin=np.float64(min([ref["margin"]] + [p["margin"] for p in per])),
               decisions=np.int64(ref["decisions"] + sum(p["decisions"] for p in per)),
               close=np.int64(ref["close"] + sum(p["close"] for p in per)))
    for i in range(len(inp["pcd"])):
        out[f"pcd{i}"], out[f"pose{i}"] = inp["pcd"][i], inp["pose"][i]
        out[f"exp_pcd{i}"], out[f"exp_pose{i}"] = ref["pcd"][i], ref["pose"][i]
        out[f"s_pcd{i}"] = np.concatenate([p["pcd"][i] for p in per])
        out[f"s_pose{i}"] = np.concatenate([p["pose"][i] for p in per])
    return out


def inputs_of(case):
    """The `inp` dict of run_reference from a loaded fixture."""
    n = int(case["n_cams"])
    return dict(bounds=case["bounds"], gripper=case["gripper"], pcd=[case[f"pcd{i}"] for i in range(n)],
                pose=[case[f"pose{i}"] for i in range(n)], action_trans=case["action_trans"],
                action_rot_grip=case["action_rot_grip"], layer=case["layer"], trans_aug_range=case["trans_aug_range"],
                rot_aug_range=case["rot_aug_range"])


_LOADED = {}


def load_cases():
    """{name: dict of arrays} of the committed fixtures (loaded once, shared, never modified)."""
    if not _LOADED:
        for path in sorted(glob.glob(os.path.join(GOLDEN, "*.npz"))):
            with np.load(path) as z:
                _LOADED[os.path.splitext(os.path.basename(path))[0]] = {k: z[k] for k in z.files}
    return _LOADED
