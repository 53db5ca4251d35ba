"""Cases, fixtures, bounds and the restatement shared by tests/test_volume.py, tests/golden/make_golden_volume.py and
tests/tools/volume_graph_capture_check.py -- TEST INFRASTRUCTURE.

The op:  resample_pad(sources, s, p) = F.pad(F.interpolate(torch.cat(sources, 1), scale_factor=s, mode='trilinear',
align_corners=False), (p,) * 6, mode='replicate')  (`compose`).  The truth of a case is that composition in float64 on the
CPU; ref_err is the relative max error of the same composition in float32 against it; ours must lie within
FACTOR x max(ref_err, 2^-23) x max|truth|, for the output and every source gradient, and be bit-equal where ref_err == 0.

A module fixture (tests/golden/volume/<name>.npz, arrays only) holds what ManiGaussian's own Conv3DBlock / Conv3DUpsampleBlock
(helpers/network_utils.py:129-171, 374-391, executed unmodified on a CPU) were given and gave:
  x, g: the input and the upstream gradient, float32;  p.<key>: the module's parameters by state_dict key, float32;
  out64, dx64, dp64.<key>: the float64 module's output and the float64 gradients of sum(out g) towards x and every parameter;
  ref_err.out, ref_err.dx, ref_err.dp.<key>: the float32 module's largest deviation from each over max|truth|.
"""
import importlib.util
import os

import numpy as np
import torch
import torch.nn.functional as F

from numerics import rel_err, same_bits  # noqa: F401  (re-exported: the tests and the tools reach them through this module)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden", "volume")
REF_FILE = os.path.join(os.environ.get("MGS_REFERENCE_ROOT", "/root/reference"), "helpers", "network_utils.py")
FACTOR = 16.0              # tolerance = FACTOR x the reference's own float32 error ...
FLOOR = 2.0 ** -23         # ... which counts as at least one ulp of the truth's magnitude
REF_ERR_CEILING = 1e-5     # a case whose yardstick is looser than this is refused

# name: (the sources' shapes [B, C, D, H, W], scale, pad)
CASES = {
    "up5":       (((2, 3, 4, 5, 6),), 5, 2),                                   # production scale and pad, non-cube, B = 2
    "up2_w1":    (((1, 2, 3, 2, 1),), 2, 1),                                   # an axis of length 1: i1 clamps to i0 everywhere
    "up3_nopad": (((1, 2, 2, 3, 4),), 3, 0),                                   # odd scale (lambda = 0 at centres), no pad
    "one_voxel": (((1, 1, 1, 1, 1),), 5, 2),                                   # every output is the input; the gradient is sum(g)
    "pad2":      (((1, 2, 4, 5, 6),), 1, 2),                                   # pure pad: corner sums of (p + 1)^3 terms
    "cat_pad1":  (((1, 2, 3, 4, 5), (1, 3, 3, 4, 5)), 1, 1),                   # the second source is a channel slice [:, 1:4] of 5
    "cat3_up2":  (((2, 1, 2, 3, 4), (2, 1, 2, 3, 4), (2, 2, 2, 3, 4)), 2, 1),  # three sources, B = 2, scale and pad together
    "wide_row":  (((1, 2, 2, 3, 67),), 2, 1),                                  # output rows of 136 floats: past one wave
    "identity":  (((1, 2, 2, 3, 4),), 1, 0),                                   # bit-equal both ways
}
SLICED = {"cat_pad1": {1: (5, 1)}}  # case: {source index: (channels of the wider tensor, first channel of the slice)}


def make_sources(case, device="cpu"):
    """The case's sources, fp32, from a generator seeded by the case's position.  A source listed in SLICED is a channel slice of
    a wider tensor (a view: batch stride of the wider tensor, storage offset of the slice)."""
    shapes, _, _ = CASES[case]
    g = torch.Generator().manual_seed(4000 + list(CASES).index(case))
    out = []
    for k, (B, C, D, H, W) in enumerate(shapes):
        wide, first = SLICED.get(case, {}).get(k, (C, 0))
        t = torch.randn(B, wide, D, H, W, generator=g).to(device)
        out.append(t[:, first:first + C])
    return out


def make_upstream(case, device="cpu"):
    shapes, s, p = CASES[case]
    B, _, D, H, W = shapes[0]
    g = torch.Generator().manual_seed(4500 + list(CASES).index(case))
    return torch.randn(B, sum(sh[1] for sh in shapes), s * D + 2 * p, s * H + 2 * p, s * W + 2 * p, generator=g).to(device)


def compose(sources, scale, pad, dtype=None):
    """The plain torch composition, in `dtype` (default: the sources'), on the sources' device."""
    x = torch.cat([t if dtype is None else t.to(dtype) for t in sources], 1)
    if scale > 1:
        x = F.interpolate(x, scale_factor=scale, mode="trilinear", align_corners=False)
    return F.pad(x, (pad,) * 6, mode="replicate")


def compose_with_grads(sources, upstream, scale, pad, dtype):
    """(out, [gradient of sum(out upstream) towards each source]) of the composition in `dtype`."""
    leaves = [t.detach().to(dtype).clone().requires_grad_(True) for t in sources]
    out = compose(leaves, scale, pad)
    out.backward(upstream.to(dtype))
    return out.detach(), [t.grad for t in leaves]


def axis_weights(n, s, p, dtype=torch.float64):
    """[s n + 2 p, n]: the per-axis matrix of the formula (row op: weight 1 - lambda on i0, lambda on i1).  In float64 the
    arithmetic is float64 throughout, as torch's is for float64 tensors; in float32, 1 / s and lambda are float32, as the
    kernels compute them."""
    real = np.float64 if dtype == torch.float64 else np.float32
    A = torch.zeros(s * n + 2 * p, n, dtype=dtype)
    inv = real(1.0 / s)
    for op in range(s * n + 2 * p):
        o = min(max(op - p, 0), s * n - 1)
        src = max(real(inv * (real(o) + real(0.5)) - real(0.5)), real(0))
        i0 = int(np.floor(src))
        lam = real(src - real(i0))
        i1 = min(i0 + 1, n - 1)
        A[op, i0] += float(real(1) - lam)
        A[op, i1] += float(lam)
    return A


def restatement(sources, scale, pad, dtype=torch.float64):
    """The op from the three per-axis matrices: out[b, c, z, y, x] = sum A_D[z, k] A_H[y, j] A_W[x, i] cat[b, c, k, j, i].
    Differentiable towards the sources."""
    x = torch.cat([t.to(dtype) for t in sources], 1)
    D, H, W = x.shape[2:]
    Az, Ay, Ax = (axis_weights(n, scale, pad, dtype).to(x.device) for n in (D, H, W))
    return torch.einsum("zk,yj,xi,bckji->bczyx", Az, Ay, Ax, x)


def bound(ref_err):
    """Largest allowed relative error for a tensor whose float32 reference has ref_err."""
    return FACTOR * max(ref_err, FLOOR)


_TRUTH = {}


def truth(case):
    """The case's CPU truth, computed once and shared (do not modify): sources, upstream, out64, grads64 (one per source) and
    the float32 composition's ref_err for the output and every gradient."""
    if case not in _TRUTH:
        _, s, p = CASES[case]
        sources, upstream = make_sources(case), make_upstream(case)
        out64, g64 = compose_with_grads(sources, upstream, s, p, torch.float64)
        out32, g32 = compose_with_grads(sources, upstream, s, p, torch.float32)
        errs = dict(out=rel_err(out32, out64), grads=[rel_err(a, b) for a, b in zip(g32, g64)])
        assert max([errs["out"]] + errs["grads"]) <= REF_ERR_CEILING, (case, errs)
        _TRUTH[case] = dict(sources=sources, upstream=upstream, out64=out64, grads64=g64, ref_err=errs)
    return _TRUTH[case]


# ---- the module fixtures ---------------------------------------------------------------------------------------------------------
# name: (class, constructor arguments, input shape)
MODULES = {
    "up_s5_k5":   ("Conv3DUpsampleBlock", dict(in_channels=4, out_channels=6, strides=5, kernel_sizes=5, activation="lrelu"), (1, 4, 3, 4, 5)),
    "up_s2_k3":   ("Conv3DUpsampleBlock", dict(in_channels=3, out_channels=4, strides=2, kernel_sizes=3, activation="lrelu"), (2, 3, 3, 2, 4)),
    "up_s1_k3":   ("Conv3DUpsampleBlock", dict(in_channels=3, out_channels=4, strides=1, kernel_sizes=3, activation="lrelu"), (1, 3, 3, 2, 4)),
    "conv_k3":    ("Conv3DBlock", dict(in_channels=5, out_channels=4, kernel_sizes=3, strides=1, activation="lrelu"), (1, 5, 4, 5, 6)),
    "conv_k5_s5": ("Conv3DBlock", dict(in_channels=3, out_channels=4, kernel_sizes=5, strides=5, activation="lrelu"), (1, 3, 10, 10, 15)),
    "conv_k3_id": ("Conv3DBlock", dict(in_channels=4, out_channels=1, kernel_sizes=3, strides=1, activation=None), (1, 4, 4, 5, 6)),
}
STATE_KEYS = {
    "up_s5_k5": ["conv_up.0.conv3d.bias", "conv_up.0.conv3d.weight", "conv_up.2.conv3d.bias", "conv_up.2.conv3d.weight"],
    "up_s2_k3": ["conv_up.0.conv3d.bias", "conv_up.0.conv3d.weight", "conv_up.2.conv3d.bias", "conv_up.2.conv3d.weight"],
    "up_s1_k3": ["conv_up.0.conv3d.bias", "conv_up.0.conv3d.weight", "conv_up.1.conv3d.bias", "conv_up.1.conv3d.weight"],
    "conv_k3": ["conv3d.bias", "conv3d.weight"],
    "conv_k5_s5": ["conv3d.bias", "conv3d.weight"],
    "conv_k3_id": ["conv3d.bias", "conv3d.weight"],
}
SPLIT = {"conv_k3": 2}  # fixtures also fed as the list [x[:, :n], x[:, n:]]


def have_reference() -> bool:
    return os.path.isfile(REF_FILE)


_REF = []


def load_reference():
    """helpers/network_utils.py, unmodified."""
    if not _REF:
        spec = importlib.util.spec_from_file_location("_mgs_reference_network_utils_volume", REF_FILE)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        _REF.append(mod)
    return _REF[0]


def module_inputs(name):
    """x, g (the upstream gradient is drawn once the output's shape is known: g(shape)) and the parameter seed."""
    seed = 5000 + list(MODULES).index(name)
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(*MODULES[name][2], generator=gen)
    return x, (lambda shape: torch.randn(*shape, generator=gen)), seed


def build_module(namespace, name, seed):
    """The module of fixture `name` from `namespace` (the reference's file or manigaussian_amd), with biases drawn too (the
    reference zeroes them: a zero bias would leave its gradient path untested)."""
    cls, kw, _ = MODULES[name]
    torch.manual_seed(seed)
    m = getattr(namespace, cls)(**kw)
    gen = torch.Generator().manual_seed(seed + 500)
    with torch.no_grad():
        for k, v in sorted(m.state_dict().items()):
            if k.endswith("bias"):
                v.copy_(torch.randn(v.shape, generator=gen) * 0.1)
    return m


def run_module(m, x, g, dtype, device="cpu", split=None):
    """(out, dx, {key: dparam}) of module m (moved to dtype / device) on x with upstream g, as float64 CPU tensors."""
    m = m.to(device=device, dtype=dtype)
    m.zero_grad(set_to_none=True)
    xx = x.detach().to(device=device, dtype=dtype).clone().requires_grad_(True)
    out = m(xx) if split is None else m([xx[:, :split], xx[:, split:]])
    out.backward(g.to(device=device, dtype=dtype))
    dp = {k: v.grad.detach().double().cpu() for k, v in m.named_parameters()}
    return out.detach().double().cpu(), xx.grad.double().cpu(), dp


def reference_module_case(name):
    """{array name: numpy array}: the fixture of `name`, computed from the reference's classes."""
    ref = load_reference()
    x, draw, seed = module_inputs(name)
    m = build_module(ref, name, seed)
    params = {k: v.detach().clone() for k, v in m.state_dict().items()}
    with torch.no_grad():
        g = draw(m(x).shape)
    out32, dx32, dp32 = run_module(m, x, g, torch.float32)
    out64, dx64, dp64 = run_module(m, x, g, torch.float64)
    arrays = {"x": x.numpy(), "g": g.numpy(), "out64": out64.numpy(), "dx64": dx64.numpy(),
              "ref_err.out": np.float64(rel_err(out32, out64)), "ref_err.dx": np.float64(rel_err(dx32, dx64))}
    for k, v in params.items():
        arrays["p." + k] = v.numpy()
        arrays["dp64." + k] = dp64[k].numpy()
        arrays["ref_err.dp." + k] = np.float64(rel_err(dp32[k], dp64[k]))
    worst = max(float(v) for k, v in arrays.items() if k.startswith("ref_err."))
    assert worst <= REF_ERR_CEILING, (name, worst)
    assert sorted(params) == STATE_KEYS[name], (name, sorted(params))
    return arrays


def module_fixture_path(name):
    return os.path.join(GOLDEN_DIR, name + ".npz")


_MODULE_FIXTURES = {}


def load_module_fixture(name):
    """The committed fixture as {array name: tensor (float for ref_err.*)}, loaded once and shared (do not modify)."""
    if name not in _MODULE_FIXTURES:
        with np.load(module_fixture_path(name), allow_pickle=False) as z:
            _MODULE_FIXTURES[name] = {k: (float(z[k]) if k.startswith("ref_err.") else torch.from_numpy(z[k])) for k in z.files}
    return _MODULE_FIXTURES[name]


def fixture_module(namespace, name):
    """The module of fixture `name` from `namespace`, carrying the fixture's parameters (loaded with strict=True)."""
    f = load_module_fixture(name)
    cls, kw, _ = MODULES[name]
    m = getattr(namespace, cls)(**kw)
    m.load_state_dict({k[2:]: v for k, v in f.items() if k.startswith("p.")}, strict=True)
    return m


def module_errors(f, out, dx, dp):
    """{tensor name: (relative error against the fixture's truth, the fixture's ref_err)}."""
    res = {"out": (rel_err(out, f["out64"]), f["ref_err.out"]), "dx": (rel_err(dx, f["dx64"]), f["ref_err.dx"])}
    for k, v in dp.items():
        res["dp." + k] = (rel_err(v, f["dp64." + k]), f["ref_err.dp." + k])
    return res


# ---- the same modules in torch's own layers: what a caller runs without this library ------------------------------------------------
class _PlainBlock(torch.nn.Module):
    def __init__(self, in_channels, out_channels, kernel_sizes=3, strides=1, norm=None, activation=None):
        super().__init__()
        self.conv3d = torch.nn.Conv3d(in_channels, out_channels, kernel_sizes, strides, padding=kernel_sizes // 2,
                                      padding_mode="replicate")
        self.activation = torch.nn.LeakyReLU(0.02) if activation == "lrelu" else None
        assert activation in (None, "lrelu") and norm is None

    def forward(self, x):
        x = self.conv3d(x)
        return self.activation(x) if self.activation is not None else x


class _PlainUpsampleBlock(torch.nn.Module):
    def __init__(self, in_channels, out_channels, strides, kernel_sizes=3, norm=None, activation=None):
        super().__init__()
        layers = [_PlainBlock(in_channels, out_channels, kernel_sizes, 1, norm, activation)]
        if strides > 1:
            layers.append(torch.nn.Upsample(scale_factor=strides, mode="trilinear", align_corners=False))
        layers.append(_PlainBlock(out_channels, out_channels, kernel_sizes, 1, norm, activation))
        self.conv_up = torch.nn.Sequential(*layers)

    def forward(self, x):
        return self.conv_up(x)


class plain:
    """A namespace for fixture_module(): nn.Upsample + nn.Conv3d(padding_mode='replicate') + nn.LeakyReLU."""
    Conv3DBlock = _PlainBlock
    Conv3DUpsampleBlock = _PlainUpsampleBlock
