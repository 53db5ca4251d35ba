"""The pointwise family's cases and inputs for tests/test_pointwise.py and tests/tools/conv_graph_capture_check.py -- TEST
INFRASTRUCTURE.  The reference is torch's own F.conv3d on the CPU; how it is shared, its yardstick and the bound: tests/conv_cases.py.

The kernels' own tiles (csrc/mgs_pointwise.hip), which the seam cases straddle; n = D H W:
  forward (and the input gradient alone): 1024 consecutive voxels per workgroup, 4 per thread; 16-byte accesses where n is a multiple
  of 4, single words otherwise; up to 16 input channels in registers, above that 8 output channels per pass;
  backward with dw or db: tiles of 256 voxels up to 8 input channels, of 128 above; 8 output channels per wave, 8 waves; above 16 input
  channels one launch per 16; the partial records: at most 64 runs of tiles.
"""
import torch
import torch.nn.functional as F

import conv_cases
from conv_cases import FACTOR, FLOOR, REF_ERR_CEILING, bound, same_bits  # noqa: F401

FWD_TILE = 1024
BWD_TILE_8, BWD_TILE_16 = 256, 128
MAX_RUNS = 64

# name: B, Cin, Cout, D x H x W, bias (and the mean of x)
CASES = {
    "one_voxel":      dict(shape=(1, 2, 3, (1, 1, 1), True)),        # a single column
    "scalar":         dict(shape=(1, 1, 1, (3, 3, 3), False)),       # one channel each side
    "odd":            dict(shape=(2, 3, 5, (5, 7, 9), True)),        # batch, odd channels; n = 315: rows start off 16-byte boundaries
    "stem_out":       dict(shape=(1, 8, 64, (12, 12, 12), True)),    # conv_out's channels; n = 1728: a whole forward tile and a part
    "stem_out_batch": dict(shape=(2, 8, 64, (7, 6, 5), True)),       # the same with a batch and n = 210
    "in_pre":         dict(shape=(1, 10, 64, (8, 8, 8), True)),      # 10 input channels: the 16-channel forms, 128-voxel tiles
    "wide":           dict(shape=(1, 64, 64, (4, 4, 4), True)),      # the Cin > 16 path, 64-term sums, four launches of the backward
    "wide_odd":       dict(shape=(2, 20, 17, (3, 5, 7), True)),      # Cin > 16 with single-word accesses, a last group of 4, 17 = 2 x 8 + 1
    "narrow_out":     dict(shape=(1, 64, 1, (6, 6, 6), True)),       # one output channel
    "no_bias":        dict(shape=(1, 8, 64, (6, 6, 6), False)),      # null bias, null db
    "tail_1":         dict(shape=(1, 8, 16, (1, 1, 1025), True)),    # one element past a power of two (and past FWD_TILE)
    "tail_3":         dict(shape=(2, 4, 4, (3, 11, 31), True)),      # n = 1023, odd rows
    "seam":           dict(shape=(1, 8, 8, (1, 3, 2731), True)),     # n = 8193 = 8 FWD_TILE + 1 = 32 BWD_TILE_8 + 1
    "seam_vec":       dict(shape=(1, 8, 8, (1, 4, BWD_TILE_8 + 1), True)),   # n = 1028 = FWD_TILE + 4 = 4 BWD_TILE_8 + 4, 16-byte accesses
    "seam_16":        dict(shape=(1, 10, 9, (1, 3, 43), True)),      # n = 129 = BWD_TILE_16 + 1
    "long_sum":       dict(shape=(2, 2, 2, (48, 48, 48), True), mean=3.0),   # dw / db sums of 221 184 terms and their merge
    "long_sum_stem":  dict(shape=(1, 8, 64, (40, 40, 40), True), mean=1.0),  # the stem's channels over many runs
}
ALL = list(CASES)


def has_bias(case):
    return conv_cases.has_bias(CASES, case)


def quantities(case):
    return conv_cases.quantities(has_bias(case))


def make_inputs(case):
    """{x, w, b (or None), g}: fp32 CPU tensors from a seeded generator; weights scaled by Cin^-1/2."""
    c = CASES[case]
    B, cin, cout, ext, bias = c["shape"]
    gen = torch.Generator().manual_seed(7000 + ALL.index(case))
    x = torch.randn(B, cin, *ext, generator=gen) + c.get("mean", 0.0)
    w = torch.randn(cout, cin, 1, 1, 1, generator=gen) * cin ** -0.5
    b = torch.randn(cout, generator=gen) if bias else None
    g = torch.randn(B, cout, *ext, generator=gen)
    return {"x": x, "w": w, "b": b, "g": g}


def torchs(t, dtype, device="cpu"):
    """{y, dx, dw, db} of torch's own op on the inputs t, in dtype on device; loss = sum(y g)."""
    x = t["x"].to(device, dtype).requires_grad_(True)
    w = t["w"].to(device, dtype).requires_grad_(True)
    b = None if t["b"] is None else t["b"].to(device, dtype).requires_grad_(True)
    y = F.conv3d(x, w, b)
    (y * t["g"].to(device, dtype)).sum().backward()
    return {"y": y.detach(), "dx": x.grad, "dw": w.grad, "db": None if b is None else b.grad}


def reference(case):
    """{x, w, b, g (float32), y64, dx64, dw64, db64, ref_err: {quantity: yardstick}}, computed once and shared."""
    return conv_cases.reference("pointwise", case, lambda: make_inputs(case), torchs, quantities(case))
