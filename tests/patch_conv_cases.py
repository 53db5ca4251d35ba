"""The patch-embedding family's cases and inputs for tests/test_patch_conv.py and tests/tools/conv_graph_capture_check.py -- TEST
INFRASTRUCTURE.  The reference is torch's own act(F.conv3d(F.pad(x, (pad,) * 6, mode), w, b, stride=k)) on the CPU; how it is shared,
its yardstick and the bound: tests/conv_cases.py.

A case with an activation walks the generator's seeds from its fixed base until no pre-activation has |z64| < abn_cases.KINK (for every
case that shares the data, in that case's own padding mode and with its own bias or none): a float32 run could otherwise
legitimately take the other branch.

The kernels' own tiles (csrc/mgs_patch.hip), which the seam cases straddle: every pass takes M_TILE patches at a time, consecutive in
linear (od, oh, ow) order inside a batch entry; the forward takes N_TILE output channels per workgroup and K_SLAB input channels of
one (kd, kh) per stage; backward-data takes up to CIN_GROUP input channels per workgroup, W_NTILE rows (channel, tap) at a time; the
weight gradient takes N_TILE output channels x W_NTILE columns (channel, tap) -- the k^3 taps padded to a multiple of 32, of 4
(k = 2, 3), 2 (k = 4) or 1 (k = 5) channels -- and cuts the tiles of patches into at most MAX_RUNS records, as many as fit REC_BYTES
(at least MIN_RUNS).
"""
import importlib

import torch
import torch.nn.functional as F

import conv_cases
from abn_cases import KINK
from conv_cases import FACTOR, FLOOR, REF_ERR_CEILING, bound, same_bits  # noqa: F401

M_TILE, N_TILE, K_SLAB = 32, 128, 8
CIN_GROUP, W_NTILE = 32, 128
MAX_RUNS, MIN_RUNS, REC_BYTES = 64, 2, 64 << 20
MAX_SEEDS = 40
EXACT_SLOPE = 0.5

# name: B, Cin, Cout, D x H x W, k, pad; mode, bias, slope (None: no activation), the mean of x; `data`: the case whose inputs it shares
CASES = {
    "one_patch":  dict(shape=(1, 8, 32, (5, 5, 5), 5, 0), slope=0.0),
    "one_voxel":  dict(shape=(1, 8, 32, (1, 1, 1), 5, 2), slope=0.0),        # all 125 taps clamp onto one voxel
    "site_small": dict(shape=(1, 128, 128, (10, 10, 10), 5, 2), slope=0.0),  # the site's channels; voxels 8, 9 of each axis uncovered
    "odd":        dict(shape=(2, 24, 96, (7, 11, 13), 5, 2), slope=0.02),    # batch; Cout no multiple of 64; rows off 16-byte boundaries
    "odd_zeros":  dict(shape=(2, 24, 96, (7, 11, 13), 5, 2), mode="zeros", bias=False, slope=None, data="odd"),
    "k2":         dict(shape=(2, 16, 32, (5, 6, 7), 2, 1), slope=0.0),
    "k3":         dict(shape=(1, 8, 64, (7, 8, 10), 3, 1), slope=None),
    "k4_rest":    dict(shape=(1, 8, 32, (9, 10, 11), 4, 0), slope=0.0),      # a remainder on every axis
    "max_c":      dict(shape=(1, 256, 256, (5, 5, 5), 5, 0), slope=0.0),     # the channel limits
    "row100":     dict(shape=(1, 8, 32, (5, 10, 100), 5, 2), slope=0.0),     # the site's row length, 20 patches per row
    "long_sum":   dict(shape=(2, 8, 32, (60, 60, 60), 5, 2), slope=0.0, mean=1.0),   # 3 456-term dw / db sums over many records
    # one past each tile constant, on each axis the kernels tile
    "seam_m":     dict(shape=(1, 8, 32, (1, 8, 32), 3, 1), slope=0.0),       # 1 x 3 x 11 = M_TILE + 1 patches: rows end inside the tile
    "seam_n":     dict(shape=(1, 8, N_TILE + 32, (4, 6, 7), 5, 2), slope=0.0),
    "seam_k":     dict(shape=(1, K_SLAB + 8, 32, (5, 5, 6), 5, 0), slope=0.0),
    "seam_cin":   dict(shape=(1, CIN_GROUP + 8, 32, (6, 7, 8), 3, 1), slope=0.0),
    "seams":      dict(shape=(2, CIN_GROUP + 8, N_TILE + 32, (11, 20, 38), 3, 1), slope=0.02),   # several tiles in every sense, partial last ones
}
ALL = list(CASES)


def shape_of(case):
    """B, Cin, Cout, (D, H, W), k, pad"""
    return (2, 8, 32, (5, 7, 10), 5, 2) if case == "exact" else CASES[case]["shape"]


def has_bias(case):
    return case == "exact" or CASES[case].get("bias", True)


def mode_of(case):
    return "replicate" if case == "exact" else CASES[case].get("mode", "replicate")


def slope_of(case):
    return EXACT_SLOPE if case == "exact" else CASES[case]["slope"]


def quantities(case):
    return conv_cases.quantities(has_bias(case))


def out_extents(case):
    _, _, _, ext, k, pad = shape_of(case)
    return tuple((e + 2 * pad - k) // k + 1 for e in ext)


def patches(case):
    o = out_extents(case)
    return o[0] * o[1] * o[2]


def call(case, x, w, b, split=None):
    """The op on a case's extra arguments; split None: the public op."""
    m = importlib.import_module("manigaussian_amd.patch")
    a = (x, w, b, shape_of(case)[5], mode_of(case), slope_of(case))
    return m.patch_conv3d(*a) if split is None else m._patch_conv3d(*a, split)


def _padded(x, pad, mode):
    return F.pad(x, (pad,) * 6, mode="replicate" if mode == "replicate" else "constant") if pad else x


def _draw(case, seed):
    c = CASES[case]
    B, cin, cout, ext, k, _ = c["shape"]
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, cin, *ext, generator=gen) + c.get("mean", 0.0)
    w = torch.randn(cout, cin, k, k, k, generator=gen) * (cin * k ** 3) ** -0.5
    b = torch.randn(cout, generator=gen)
    g = torch.randn(B, cout, *out_extents(case), generator=gen)
    return {"x": x, "w": w, "b": b, "g": g}


_INPUTS = {}


def make_inputs(case):
    """{x, w, b (or None), g, seed}: fp32 CPU tensors from a seeded generator; weights scaled by (Cin k^3)^-1/2.  Cases that share data
    share the seed: the first from the owner's base at which every case of the group that has an activation keeps all its
    pre-activations KINK away from zero."""
    owner = CASES[case].get("data", case)
    if owner not in _INPUTS:
        group = [n for n in ALL if CASES[n].get("data", n) == owner and slope_of(n) is not None]
        base = 12000 + 100 * ALL.index(owner)
        for seed in range(base, base + MAX_SEEDS):
            t = _draw(owner, seed)
            ok = True
            for n in group:
                _, _, _, _, k, pad = shape_of(n)
                z = F.conv3d(_padded(t["x"].double(), pad, mode_of(n)), t["w"].double(), t["b"].double() if has_bias(n) else None, stride=k)
                ok = ok and z.abs().min().item() >= KINK
            if ok:
                break
        else:
            raise RuntimeError(f"{owner}: no seed in {MAX_SEEDS} keeps every pre-activation {KINK} away from zero")
        t["seed"] = seed
        _INPUTS[owner] = t
    t = dict(_INPUTS[owner])
    if not has_bias(case):
        t["b"] = None
    return t


def exact_inputs():
    """Small integers at [2, 8 -> 32, 5 x 7 x 10], k = 5, pad 2 (the bias: integers + 1/2, so that no pre-activation is zero; the slope
    1/2): every sum is exact in float32 -- 1000 terms of magnitude <= 8 stay below 2^24."""
    gen = torch.Generator().manual_seed(12900)

    def ints(lo, hi, *shape):
        return torch.randint(lo, hi + 1, shape, generator=gen).float()
    return {"x": ints(-4, 4, 2, 8, 5, 7, 10), "w": ints(-2, 2, 32, 8, 5, 5, 5), "b": ints(-3, 3, 32) + 0.5, "g": ints(-2, 2, 2, 32, 1, 2, 2)}


def torchs(t, dtype, case, device="cpu", with_z=False):
    """{y, dx, dw, db} of torch's own ops on the inputs t, in dtype on device; loss = sum(y g)."""
    def leaf(v):   # (a copy: cases that share inputs must not share leaves)
        return v.detach().to(device, dtype).clone().requires_grad_(True)
    _, _, _, _, k, pad = shape_of(case)
    slope = slope_of(case)
    x, w = leaf(t["x"]), leaf(t["w"])
    b = None if t["b"] is None else leaf(t["b"])
    z = F.conv3d(_padded(x, pad, mode_of(case)), w, b, stride=k)
    y = z if slope is None else F.leaky_relu(z, slope)
    (y * t["g"].to(device, dtype)).sum().backward()
    r = {"y": y.detach(), "dx": x.grad, "dw": w.grad, "db": None if b is None else b.grad}
    if with_z:
        r["z"] = z.detach()
    return r


def reference(case):
    """{x, w, b, g (float32), z64, y64, dx64, dw64, db64, ref_err: {quantity: yardstick}}, computed once and shared."""
    return conv_cases.reference("patch", case, exact_inputs if case == "exact" else lambda: make_inputs(case),
                                lambda t, dtype: torchs(t, dtype, case, with_z=dtype is torch.float64), quantities(case), also=("z",))
