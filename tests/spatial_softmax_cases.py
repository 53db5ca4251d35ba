"""Cases, fixtures, bounds and the restatement shared by tests/test_spatial_softmax.py, tests/golden/make_golden_spatial_softmax.py
and tests/tools/spatial_softmax_graph_capture_check.py -- TEST INFRASTRUCTURE.

A fixture (tests/golden/spatial_softmax/<case>.npz, arrays only) holds what ManiGaussian's own SpatialSoftmax3D
(helpers/network_utils.py:927-963, executed unmodified on a CPU) and nn.AdaptiveMaxPool3d(1) were given and gave:
  x [B,C,D,H,W], g_k [B,3C], g_m [B,C]: the input and the two upstream gradients, float32;
  kp64, max64: the float64 module's keypoints and the global maximum -- the truth;
  dx64: the float64 gradient of sum(kp g_k) + sum(max g_m) towards x;
  argmax [B*C] (int64) and dx64_k_at_max [B*C]: dx64_k, the gradient of sum(kp g_k) alone, equals dx64 bit for bit everywhere but at
  each row's first maximum (the generator asserts it), so only its values THERE are stored; load_fixture() rebuilds dx64_k;
  ref_abs_err: the float32 module's own largest ABSOLUTE deviation from the truth's keypoints (they live in [-1, 1], may be 0);
  ref_err = (for dx, for dx_k): its largest deviation from the truth's gradient over max|truth|.  The yardsticks of the tolerances;
  pos_x, pos_y, pos_z (case `noncube` only): the reference module's three registered buffers.
"""
import importlib.util
import os

import numpy as np
import torch

from numerics import same_bits  # noqa: F401  (re-exported: the tests and the tools reach them through this module)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden", "spatial_softmax")
REF_FILE = os.path.join(os.environ.get("MGS_REFERENCE_ROOT", "/root/reference"), "helpers", "network_utils.py")
FACTOR = 16.0              # tolerance = FACTOR x the reference's own float32 error
KP_FLOOR = 2.0 ** -23      # ... and for the keypoints at least FACTOR ulps of 1 (coordinates live in [-1, 1])
REF_ERR_CEILING = 2e-4     # the generator refuses a case whose yardstick is looser than this
TEMPERATURE = 0.01

# name: B, C, D, H, W and the input
CASES = {
    "cube20":   dict(shape=(1, 6, 20, 20, 20), kind="randn", scale=0.05),
    "odd31":    dict(shape=(1, 2, 31, 31, 31), kind="randn", scale=0.05),    # N odd: the second row starts misaligned
    "noncube":  dict(shape=(2, 3, 5, 7, 9), kind="randn", scale=0.05),       # the meshgrid quirk
    "sharp":    dict(shape=(1, 4, 20, 20, 20), kind="randn", scale=0.3),     # one voxel holds almost all the mass
    "offset":   dict(shape=(1, 3, 12, 12, 12), kind="offset", scale=0.05),   # x / t ~ 3750: overflows without max subtraction
    "ties":     dict(shape=(1, 4, 16, 16, 16), kind="ties", scale=0.3),      # hundreds of voxels share the max; exact zeros
    "constant": dict(shape=(1, 2, 6, 6, 6), kind="constant", scale=0.7),     # uniform softmax, argmax = index 0
    "tiny":     dict(shape=(2, 3, 2, 3, 4), kind="randn", scale=0.02),
    "single":   dict(shape=(1, 2, 1, 1, 1), kind="randn", scale=1.0),        # keypoints are -1, softmax gradient 0
}


def make_inputs(case):
    """x, g_k, g_m: fp32 on the CPU, from a generator seeded by the case's position (the committed fixtures are these numbers)."""
    c = CASES[case]
    B, C, D, H, W = c["shape"]
    g = torch.Generator().manual_seed(2000 + list(CASES).index(case))
    r = torch.randn(B, C, D, H, W, generator=g)
    if c["kind"] == "randn":
        x = r * c["scale"]
    elif c["kind"] == "offset":
        x = r * c["scale"] + 37.5
    elif c["kind"] == "ties":
        x = torch.clamp(torch.relu(r * c["scale"]), max=0.15)
    else:
        x = torch.full((B, C, D, H, W), c["scale"])
    g_k = torch.randn(B, 3 * C, generator=g)
    g_m = torch.randn(B, C, generator=g)
    return x, g_k, g_m


def position_tables(D, H, W, dtype=torch.float32):
    """The reference's three buffers: float32 values (held in `dtype`)."""
    px, py, pz = np.meshgrid(np.linspace(-1., 1., D), np.linspace(-1., 1., H), np.linspace(-1., 1., W))
    return tuple(torch.from_numpy(p.reshape(D * H * W)).float().to(dtype) for p in (px, py, pz))


def restatement(x, D, H, W, temperature, dtype):
    """The reference's formula in plain torch ops, in `dtype`, on the device of x: (keypoints [B,3C], maxpool [B,C]),
    differentiable towards x when x requires grad.  Stands where the reference cannot be (the GPU tests); pinned against the
    fixtures on the CPU."""
    B, C = x.shape[:2]
    f = x.to(dtype).reshape(-1, D * H * W)
    p = torch.softmax(f / temperature, dim=-1)
    px, py, pz = (t.to(x.device) for t in position_tables(D, H, W, dtype))
    e = torch.cat([torch.sum(px * p, dim=1, keepdim=True), torch.sum(py * p, dim=1, keepdim=True),
                   torch.sum(pz * p, dim=1, keepdim=True)], 1)
    return e.view(-1, C * 3), f.max(dim=1)[0].view(B, C)


def first_argmax(x):
    """[B*C] lowest flat index holding each row's maximum."""
    f = x.reshape(x.size(0) * x.size(1), -1)
    index = torch.arange(f.size(1), device=x.device).expand_as(f)
    return torch.where(f == f.max(dim=1, keepdim=True)[0], index, f.size(1)).min(dim=1)[0]


# ---- the reference -----------------------------------------------------------------------------------------------------------
def have_reference() -> bool:
    return os.path.isfile(REF_FILE)


_REF = []


def load_reference():
    """helpers/network_utils.py, unmodified."""
    if not _REF:
        spec = importlib.util.spec_from_file_location("_mgs_reference_network_utils", REF_FILE)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        _REF.append(mod)
    return _REF[0]


def _run(ref, x, g_k, g_m, dtype):
    B, C, D, H, W = x.shape
    ss = ref.SpatialSoftmax3D(D, H, W, C).to(dtype)
    maxp = torch.nn.AdaptiveMaxPool3d(1)
    res = {}
    for name, with_max in (("dx", True), ("dx_k", False)):
        xx = x.detach().to(dtype).clone().requires_grad_(True)
        kp = ss(xx.contiguous())
        mx = maxp(xx).view(B, -1)
        loss = (kp * g_k.to(dtype)).sum()
        if with_max:
            loss = loss + (mx * g_m.to(dtype)).sum()
        loss.backward()
        res[name] = xx.grad
    res["kp"], res["max"] = kp.detach(), mx.detach()
    return res, ss


def reference_case(case):
    """{array name: numpy array}: the fixture of `case`, computed from the reference."""
    ref = load_reference()
    x, g_k, g_m = make_inputs(case)
    r32, ss32 = _run(ref, x, g_k, g_m, torch.float32)
    r64, _ = _run(ref, x, g_k, g_m, torch.float64)
    arg = first_argmax(x)
    rows = torch.arange(arg.numel())
    flat, flat_k = r64["dx"].reshape(arg.numel(), -1), r64["dx_k"].reshape(arg.numel(), -1)
    rebuilt = flat.clone()
    rebuilt[rows, arg] = flat_k[rows, arg]
    assert torch.equal(rebuilt, flat_k), case  # the max-pool's gradient lands on exactly one voxel per row, the first maximum
    out = {"x": x.numpy(), "g_k": g_k.numpy(), "g_m": g_m.numpy(), "kp64": r64["kp"].numpy(), "max64": r64["max"].numpy(),
           "dx64": r64["dx"].numpy(), "argmax": arg.numpy(), "dx64_k_at_max": flat_k[rows, arg].numpy()}
    err = [(r32["kp"].double() - r64["kp"]).abs().max().item()]
    for n in ("dx", "dx_k"):
        mag = r64[n].abs().max().item()
        err.append((r32[n].double() - r64[n]).abs().max().item() / mag if mag > 0 else 0.0)
    assert max(err) <= REF_ERR_CEILING, (case, err)
    out["ref_abs_err"] = np.asarray(err[0], dtype=np.float64)
    out["ref_err"] = np.asarray(err[1:], dtype=np.float64)
    if case == "noncube":
        for n in ("pos_x", "pos_y", "pos_z"):
            out[n] = getattr(ss32, n).numpy()
    return out


def fixture_path(case):
    return os.path.join(GOLDEN_DIR, case + ".npz")


_FIXTURES = {}


def load_fixture(case):
    """The committed fixture as {name: tensor}, loaded once and shared (do not modify); ref_err as {name: float}."""
    if case not in _FIXTURES:
        with np.load(fixture_path(case)) as z:
            f = {k: torch.from_numpy(z[k]) for k in z.files if k not in ("ref_err", "ref_abs_err")}
            f["ref_err"] = dict(zip(("kp", "dx", "dx_k"), [float(z["ref_abs_err"])] + z["ref_err"].tolist()))
        rows = torch.arange(f["argmax"].numel())
        dx_k = f["dx64"].reshape(rows.numel(), -1).clone()
        dx_k[rows, f["argmax"]] = f["dx64_k_at_max"]
        f["dx64_k"] = dx_k.reshape(f["dx64"].shape)
        _FIXTURES[case] = f
    return _FIXTURES[case]


def kp_bound(ref_abs_err):
    return max(FACTOR * ref_abs_err, FACTOR * KP_FLOOR)


def dx_bound(ref_err, truth):
    return FACTOR * ref_err * truth.abs().max().item()


def bounds(case, f=None):
    """{"kp" | "dx" | "dx_k": largest allowed |ours - truth|} from the fixture alone."""
    f = load_fixture(case) if f is None else f
    e = f["ref_err"]
    return {"kp": kp_bound(e["kp"]), "dx": dx_bound(e["dx"], f["dx64"]), "dx_k": dx_bound(e["dx_k"], f["dx64_k"])}
