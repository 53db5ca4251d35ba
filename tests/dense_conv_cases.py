"""The dense family's cases and inputs for tests/test_dense_conv.py and tests/tools/conv_graph_capture_check.py -- TEST
INFRASTRUCTURE.  The reference is torch's own F.conv3d (+ F.leaky_relu) on the CPU; how it is shared, its yardstick and the bound:
tests/conv_cases.py.

A case with an activation walks the generator's seeds from its fixed base until no pre-activation has |z64| < abn_cases.KINK (with and
without the bias: the cases that share its data drop it): a float32 run could otherwise legitimately take the other branch.  The two
long sums have no activation: among their 4 million (221 000) pre-activations some lie that close to zero under every seed.

The kernels' own tiles (csrc/mgs_dense.hip), which the seam cases straddle: the forward (and backward-data, which is the same kernel
with the channel counts exchanged) takes M_TILE consecutive output voxels x N_TILE output channels per workgroup and K_SLAB input
channels of one tap per stage; the weight gradient takes segments of up to W_SEG voxels of an output row, N-tiles of W_NTILE
columns (ci, tap) -- 4 channels x 27 taps padded to 32, or 1 channel x 125 taps padded to 128 -- and N_TILE output channels, and
cuts the segments into at most MAX_RUNS records.
"""
import torch
import torch.nn.functional as F

import conv_cases
from abn_cases import KINK
from conv_cases import FACTOR, FLOOR, REF_ERR_CEILING, bound, same_bits  # noqa: F401

M_TILE, N_TILE, K_SLAB = 128, 128, 8
W_SEG, W_NTILE = 64, 128
MAX_RUNS = 64
MAX_SEEDS = 40
SLOPE = 0.02

# name: B, Cin, Cout, k, the OUTPUT's D x H x W (the input is k - 1 larger); bias, slope (None: no activation), the mean of x;
# `data`: the case whose inputs it shares
CASES = {
    "one_out_k3":     dict(shape=(1, 8, 32, 3, (1, 1, 1))),      # all but one lane of every tile is masked
    "one_out_k5":     dict(shape=(1, 8, 32, 5, (1, 1, 1))),
    "odd_k3":         dict(shape=(2, 24, 96, 3, (5, 7, 9))),     # odd rows, row ends inside a wave's run, a batch
    "odd_k5":         dict(shape=(2, 8, 32, 5, (3, 5, 7))),
    "plain":          dict(shape=(2, 24, 96, 3, (5, 7, 9)), slope=None, data="odd_k3"),
    "relu":           dict(shape=(2, 24, 96, 3, (5, 7, 9)), slope=0.0, data="odd_k3"),
    "no_bias":        dict(shape=(2, 24, 96, 3, (5, 7, 9)), bias=False, data="odd_k3"),   # null bias, null db
    "m_seam":         dict(shape=(1, 8, 32, 3, (1, 3, (M_TILE + 1) // 3))),   # M_TILE + 1 = 3 x 43 voxels: rows end inside the tile
    "n_seam":         dict(shape=(1, 8, N_TILE + 32, 3, (2, 3, 4))),
    "k_seam":         dict(shape=(1, K_SLAB + 8, 32, 3, (2, 3, 4))),
    "row_seam":       dict(shape=(1, 8, 32, 3, (2, 2, W_SEG + 1))),
    "seams":          dict(shape=(2, 3 * K_SLAB, N_TILE + 32, 5, (2, 3, W_SEG + 6))),   # several tiles in every sense, partial last ones
    "max_channels":   dict(shape=(1, 256, 256, 3, (2, 2, 3))),
    "final_head":     dict(shape=(1, 256, 128, 3, (3, 4, 35))),  # the sites' own channels at toy extents
    "up0_last_head":  dict(shape=(1, 128, 128, 5, (2, 3, 34))),
    "up0_first_head": dict(shape=(1, 256, 128, 5, (2, 2, 33))),
    "long_sum":       dict(shape=(2, 8, 32, 3, (40, 40, 40)), slope=None, mean=1.0),    # 128 000-term dw / db sums, many records
    "long_sum_head":  dict(shape=(1, 128, 128, 5, (12, 12, 12)), slope=None),
}
ALL = list(CASES)
EXACT = {"exact_k3": 3, "exact_k5": 5}
assert CASES["m_seam"]["shape"][4][1] * CASES["m_seam"]["shape"][4][2] == M_TILE + 1


def has_bias(case):
    return case in EXACT or CASES[case].get("bias", True)


def slope_of(case):
    return 0.5 if case in EXACT else CASES[case].get("slope", SLOPE)


def quantities(case):
    return conv_cases.quantities(has_bias(case))


def in_extents(ext, k):
    return tuple(e + k - 1 for e in ext)


def _draw(case, seed):
    c = CASES[case]
    B, cin, cout, k, ext = c["shape"]
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, cin, *in_extents(ext, k), generator=gen) + c.get("mean", 0.0)
    w = torch.randn(cout, cin, k, k, k, generator=gen) * (cin * k ** 3) ** -0.5
    b = torch.randn(cout, generator=gen)
    g = torch.randn(B, cout, *ext, generator=gen)
    return {"x": x, "w": w, "b": b, "g": g}


_INPUTS = {}


def make_inputs(case):
    """{x, w, b (or None), g, seed}: fp32 CPU tensors from a seeded generator; weights scaled by (Cin k^3)^-1/2.  Cases that share data
    share the seed, which is the first from the owner's base whose pre-activations all keep KINK away from zero where the owner or a
    sharer has an activation."""
    owner = CASES[case].get("data", case)
    if owner not in _INPUTS:
        group = [n for n in ALL if CASES[n].get("data", n) == owner]
        active = any(slope_of(n) is not None for n in group)
        base = 9000 + 100 * ALL.index(owner)
        for seed in range(base, base + MAX_SEEDS):
            t = _draw(owner, seed)
            if not active:
                break
            z = F.conv3d(t["x"].double(), t["w"].double())
            zb = z + t["b"].double().view(1, -1, 1, 1, 1)
            if min(z.abs().min().item(), zb.abs().min().item()) >= KINK:
                break
        else:
            raise RuntimeError(f"{owner}: no seed in {MAX_SEEDS} keeps every pre-activation {KINK} away from zero")
        t["seed"] = seed
        _INPUTS[owner] = t
    t = dict(_INPUTS[owner])
    if not has_bias(case):
        t["b"] = None
    return t


def exact_inputs(case):
    """Small integers at [2, 16 -> 32], output 3 x 4 x 5 (the bias: integers + 1/2, so that no pre-activation is zero): every partial sum
    is exact in float32."""
    k = EXACT[case]
    gen = torch.Generator().manual_seed(9900 + k)

    def ints(lo, hi, *shape):
        return torch.randint(lo, hi + 1, shape, generator=gen).float()
    return {"x": ints(-4, 4, 2, 16, *in_extents((3, 4, 5), k)), "w": ints(-2, 2, 32, 16, k, k, k), "b": ints(-3, 3, 32) + 0.5,
            "g": ints(-2, 2, 2, 32, 3, 4, 5)}


def torchs(t, dtype, slope, device="cpu", with_z=False):
    """{y, dx, dw, db} of torch's own ops on the inputs t, in dtype on device; loss = sum(y g)."""
    def leaf(v):   # (a copy: cases that share inputs must not share leaves)
        return v.detach().to(device, dtype).clone().requires_grad_(True)
    x, w = leaf(t["x"]), leaf(t["w"])
    b = None if t["b"] is None else leaf(t["b"])
    z = F.conv3d(x, w, b)
    y = z if slope is None else F.leaky_relu(z, slope)
    (y * t["g"].to(device, dtype)).sum().backward()
    r = {"y": y.detach(), "dx": x.grad, "dw": w.grad, "db": None if b is None else b.grad}
    if with_z:
        r["z"] = z.detach()
    return r


def reference(case):
    """{x, w, b, g (float32), z64, y64, dx64, dw64, db64, ref_err: {quantity: yardstick}}, computed once and shared."""
    return conv_cases.reference("dense", case, lambda: exact_inputs(case) if case in EXACT else make_inputs(case),
                                lambda t, dtype: torchs(t, dtype, slope_of(case), with_z=dtype is torch.float64), quantities(case),
                                also=("z",))


def exact_partial_sum_bound(case):
    """The largest sum of |term|s of any element of y, dx, dw and db of an exact case: every partial sum of every order lies below it."""
    t = {k: (v.abs() if v is not None else None) for k, v in exact_inputs(case).items()}
    r = torchs(t, torch.float64, None)
    return max(v.max().item() for v in r.values())
