"""The wide pointwise family's cases and inputs (Cin 1..16, Cout 65..256) for tests/test_wide_pointwise.py and
tests/tools/wide_pointwise_graph_capture_check.py -- TEST INFRASTRUCTURE.  The reference is torch's own F.conv3d on the CPU; how it is
shared, its yardstick and the bound: tests/conv_cases.py.

The kernels' own tiles (csrc/mgs_pointwise.hip), which the seam cases straddle; n = D H W:
  forward: 1024 consecutive voxels per workgroup, 4 per thread; 16-byte accesses where n is a multiple of 4, single words otherwise;
  the input channels in registers (8 or 16 of them), any number of output channels;
  the input gradient alone: the same tiles, 8 output channels per pass, a chain per 8 looped channels;
  backward with dw or db: tiles of 256 voxels up to 8 input channels, of 128 above; 8 output channels per wave, 8 waves, and a
  workgroup walks its run once per BLOCK of 64 output channels; the partial records: at most 64 runs of tiles.
"""
import importlib

import torch
import torch.nn.functional as F

import conv_cases
from conv_cases import FACTOR, FLOOR, REF_ERR_CEILING, bound, same_bits  # noqa: F401

FWD_TILE = 1024
BWD_TILE_8, BWD_TILE_16 = 256, 128
BLOCK = 64
MAX_RUNS = 64

# name: B, Cin, Cout, D x H x W, bias (and the mean of x)
CASES = {
    "one_voxel":          dict(shape=(1, 1, 65, (1, 1, 1), True)),        # one column; the second block holds one channel
    "first_wide":         dict(shape=(1, 2, 65, (3, 3, 3), True)),        # block 1: wave 0 owns one channel, waves 1..7 none
    "odd":                dict(shape=(2, 3, 67, (5, 7, 9), True)),        # batch; n = 315: rows off 16-byte boundaries, single words
    "stem_out_128":       dict(shape=(1, 8, 128, (12, 12, 12), True)),    # conv_out's channels; n = 1728: a whole forward tile and a part
    "stem_out_128_batch": dict(shape=(2, 8, 128, (7, 6, 5), True)),       # the same with a batch, n = 210
    "in_10":              dict(shape=(1, 10, 96, (8, 8, 8), True)),       # the 16-channel forms, 128-voxel tiles, a half-filled second block
    "in_16":              dict(shape=(1, 16, 130, (1, 3, 43), True)),     # Cin at its limit, n = 129 = BWD_TILE_16 + 1, three blocks
    "top":                dict(shape=(1, 4, 256, (4, 4, 4), True)),       # Cout at its limit, four blocks
    "no_bias":            dict(shape=(1, 8, 128, (6, 6, 6), False)),      # null bias, null db
    "seam":               dict(shape=(1, 8, 72, (1, 3, 2731), True)),     # n = 8193 = 8 FWD_TILE + 1 = 32 BWD_TILE_8 + 1
    "seam_vec":           dict(shape=(1, 8, 72, (1, 4, BWD_TILE_8 + 1), True)),   # n = 1028, 16-byte accesses across both seams
    "long_sum_stem":      dict(shape=(1, 8, 128, (40, 40, 40), True), mean=1.0),  # 250 tiles in 63 runs, a shorter last run, 64 000-term sums
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
    gen = torch.Generator().manual_seed(7100 + ALL.index(case))
    x = torch.randn(B, cin, *ext, generator=gen) + c.get("mean", 0.0)
    w = torch.randn(cout, cin, 1, 1, 1, generator=gen) * cin ** -0.5
    b = torch.randn(cout, generator=gen) if bias else None
    g = torch.randn(B, cout, *ext, generator=gen)
    return {"x": x, "w": w, "b": b, "g": g}


def call(case, x, w, b, split=None):
    """The op on a case's tensors; split None: the public op (conv_family.Family's `call`)."""
    m = importlib.import_module("manigaussian_amd.pointwise")
    return m.wide_pointwise_conv3d(x, w, b) if split is None else m._wide_pointwise_conv3d(x, w, b, split)


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
    return conv_cases.reference("pointwise_wide", case, lambda: make_inputs(case), torchs, quantities(case))
