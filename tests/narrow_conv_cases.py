"""The narrow-output family's cases and inputs for tests/test_narrow_conv.py and tests/tools/conv_graph_capture_check.py -- TEST
INFRASTRUCTURE.  The reference is torch's own F.conv3d(F.pad(x, (1,) * 6, mode), w, b) on the CPU; how it is shared, its yardstick and
the bound: tests/conv_cases.py.

The kernels' own tile (csrc/mgs_narrow.hip), which the seam cases straddle: TILE_W x TILE_H x TILE_D = 32 x 8 x 8 voxels per group of
128 threads, a register block of 4 (D) x 4 (W) voxels per thread; rows whose length is a multiple of 4 are stored 16 bytes at a time,
others word by word; the forward splits the input channels over 4 groups, backward-data walks 16 input channels per workgroup, the
weight gradient 2 (Cout = 1) or 1; the partial records: at most 64 runs of tiles.
"""
import torch
import torch.nn.functional as F

import conv_cases
from conv_cases import FACTOR, FLOOR, REF_ERR_CEILING, bound, same_bits  # noqa: F401

TILE_W, TILE_H, TILE_D = 32, 8, 8
MAX_RUNS = 64

# name: B, Cin, Cout, D x H x W, bias, the pad (and the mean of x; `data`: the case whose inputs it shares)
CASES = {
    "one_voxel":     dict(shape=(1, 2, 1, (1, 1, 1), True), mode="replicate"),    # all 27 taps clamp onto one voxel; the n = 1 set
    "thin":          dict(shape=(1, 3, 2, (1, 1, 5), True), mode="replicate"),    # two extents of 1
    "two":           dict(shape=(2, 3, 1, (2, 2, 2), True), mode="replicate"),    # both borders adjacent, every voxel a corner, batch
    "odd":           dict(shape=(2, 5, 3, (5, 7, 9), True), mode="replicate"),    # odd everything, rows off 16-byte boundaries
    "odd_zeros":     dict(shape=(2, 5, 3, (5, 7, 9), True), mode="zeros", data="odd"),   # the other mode on the same data
    "head":          dict(shape=(1, 128, 1, (6, 6, 6), True), mode="replicate"),  # the site's channels
    "head_zeros":    dict(shape=(1, 128, 1, (6, 6, 6), False), mode="zeros"),     # null bias, null db
    "wide_in":       dict(shape=(1, 130, 4, (4, 5, 6), True), mode="replicate"),  # Cin not a multiple of any group, Cout = 4
    "max_in":        dict(shape=(1, 256, 2, (3, 3, 3), True), mode="replicate"),  # the channel limit
    "seam_w":        dict(shape=(1, 4, 1, (2, 3, TILE_W + 1), True), mode="replicate"),   # a tile's halo across a seam along W ...
    "seam_h":        dict(shape=(1, 4, 2, (2, TILE_H + 1, 5), True), mode="replicate"),   # ... along H ...
    "seam_d":        dict(shape=(1, 4, 1, (TILE_D + 1, 3, 4), True), mode="replicate"),   # ... along D; the partial last tile
    "seams":         dict(shape=(1, 3, 1, (9, 17, 65), True), mode="replicate"),  # several tiles in every dimension, partial last ones
    "long_sum":      dict(shape=(2, 2, 2, (48, 48, 48), True), mode="replicate", mean=3.0),    # 221 184-term dw / db sums, many records
    "long_sum_head": dict(shape=(1, 128, 1, (24, 24, 24), True), mode="replicate", mean=1.0),  # the site's channels over many runs
}
ALL = list(CASES)


def has_bias(case):
    return case == "exact" or conv_cases.has_bias(CASES, case)


def mode_of(case):
    return "replicate" if case == "exact" else CASES[case]["mode"]


def quantities(case):
    return conv_cases.quantities(has_bias(case))


def make_inputs(case):
    """{x, w, b (or None), g}: fp32 CPU tensors from a seeded generator; weights scaled by (27 Cin)^-1/2."""
    c = CASES[case]
    B, cin, cout, ext, bias = c["shape"]
    gen = torch.Generator().manual_seed(8000 + ALL.index(c.get("data", case)))
    x = torch.randn(B, cin, *ext, generator=gen) + c.get("mean", 0.0)
    w = torch.randn(cout, cin, 3, 3, 3, generator=gen) * (27 * cin) ** -0.5
    b = torch.randn(cout, generator=gen) if bias else None
    g = torch.randn(B, cout, *ext, generator=gen)
    return {"x": x, "w": w, "b": b, "g": g}


def exact_inputs():
    """Small integers at [2, 5 -> 2, 3 x 4 x 5]: every sum is exact in float32 (the largest magnitude of any result is below 2^24)."""
    gen = torch.Generator().manual_seed(8100)

    def ints(lo, hi, *shape):
        return torch.randint(lo, hi + 1, shape, generator=gen).float()
    return {"x": ints(-4, 4, 2, 5, 3, 4, 5), "w": ints(-2, 2, 2, 5, 3, 3, 3), "b": ints(-3, 3, 2), "g": ints(-2, 2, 2, 2, 3, 4, 5)}


def torchs(t, dtype, mode="replicate", device="cpu"):
    """{y, dx, dw, db} of torch's own ops on the inputs t, in dtype on device; loss = sum(y g)."""
    x = t["x"].to(device, dtype).requires_grad_(True)
    w = t["w"].to(device, dtype).requires_grad_(True)
    b = None if t["b"] is None else t["b"].to(device, dtype).requires_grad_(True)
    y = F.conv3d(F.pad(x, (1,) * 6, mode="replicate" if mode == "replicate" else "constant"), w, b)
    (y * t["g"].to(device, dtype)).sum().backward()
    return {"y": y.detach(), "dx": x.grad, "dw": w.grad, "db": None if b is None else b.grad}


def reference(case):
    """{x, w, b, g (float32), y64, dx64, dw64, db64, ref_err: {quantity: yardstick}}, computed once and shared."""
    return conv_cases.reference("narrow", case, exact_inputs if case == "exact" else lambda: make_inputs(case),
                                lambda t, dtype: torchs(t, dtype, mode_of(case)), quantities(case))
