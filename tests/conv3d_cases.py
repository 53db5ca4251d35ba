"""The direct family's cases and inputs for tests/test_conv3d.py and tests/tools/conv_graph_capture_check.py -- TEST INFRASTRUCTURE.
The reference is torch's own F.conv3d / F.conv_transpose3d on the CPU; how it is shared, its yardstick and the bound:
tests/conv_cases.py.

The kernels' own tiles (csrc/mgs_conv3d.hip), which the seam cases straddle:
  forward / backward-weight, and backward-data at stride 1: an OUTPUT tile of 4 x 8 x 32 (D x H x W) at stride 1, 2 x 8 x 32 at stride 2;
  input channels staged 4 (stride 1) or 2 (stride 2) at a time; output channels per workgroup 8 (stride 1) or 16 (stride 2), 4 in
  the weight gradient;
  backward-data at stride 2 (= the transposed convolution's forward): 2 x 4 x 32 blocks of 2x2x2 input voxels, 4 input channels per
  workgroup, 8 output channels staged at a time;
  the weight gradient's partial records: at most 64 runs of output tiles.
"""
import torch
import torch.nn.functional as F

import conv_cases
from conv_cases import FACTOR, FLOOR, REF_ERR_CEILING, bound, same_bits  # noqa: F401

TILE_S1 = (4, 8, 32)
TILE_S2 = (2, 8, 32)
QUANTITIES = ("y", "dx", "dw")

# name: B, Cin, Cout, the input's D x H x W, stride (and the mean of x)
CASES = {
    "one_voxel_s1": dict(shape=(1, 2, 3, (1, 1, 1), 1)),        # the centre tap only
    "one_voxel_s2": dict(shape=(1, 2, 3, (1, 1, 1), 2)),
    "tiny":         dict(shape=(1, 1, 1, (3, 3, 3), 1)),        # every output voxel touches the padding
    "odd_s1":       dict(shape=(2, 3, 5, (5, 7, 9), 1)),        # batch, unequal extents, odd channel counts
    "stem_in":      dict(shape=(1, 10, 8, (12, 12, 12), 1)),    # conv0's channels
    "down_even":    dict(shape=(2, 8, 16, (12, 12, 12), 2)),    # stride 2, even input extent
    "down_odd":     dict(shape=(1, 32, 64, (7, 7, 7), 2)),      # the 25 -> 13 regime
    "down_mixed":   dict(shape=(1, 4, 4, (6, 7, 9), 2)),        # stride 2, mixed even and odd extents
    "wide":         dict(shape=(1, 64, 64, (4, 4, 4), 1)),      # 1728-term sums, several input-channel slabs
    "seam_w":       dict(shape=(1, 4, 4, (9, 17, 33), 1)),      # tile seams along W
    "seam_d":       dict(shape=(1, 4, 4, (33, 17, 9), 1)),      # tile seams along D
    "seam_tile":    dict(shape=(1, 4, 4, tuple(t + 1 for t in TILE_S1), 1)),   # one more than the tile in every dimension
    # the same at stride 2: 3 x 9 x 33 outputs (one more than the 2 x 8 x 32 tile; two blocks of the backward-data tile along D and H)
    "seam_tile_s2": dict(shape=(1, 3, 5, tuple(2 * t + 1 for t in TILE_S2), 2)),
    "long_sum":     dict(shape=(1, 2, 2, (48, 48, 48), 1), mean=3.0),   # the weight gradient's 110 592-term sums and their merge
}
# name: B, Cin, Cout (of the transposed convolution), the input's D x H x W, output_padding
TRANSPOSED = {
    "up_op0": dict(shape=(1, 64, 32, (4, 4, 4), 0)),            # -> 7^3
    "up_op1": dict(shape=(1, 16, 8, (6, 6, 6), 1)),             # -> 12^3
    "up_odd": dict(shape=(2, 5, 3, (3, 4, 5), 1)),              # -> 6 x 8 x 10: batch, unequal extents
}
ALL = list(CASES) + list(TRANSPOSED)


def is_transposed(case):
    return case in TRANSPOSED


def quantities(case):
    return QUANTITIES   # (no bias)


def make_inputs(case):
    """{x, w, g}: fp32 CPU tensors from a seeded generator; weights scaled by (27 Cin)^-1/2."""
    c = TRANSPOSED[case] if is_transposed(case) else CASES[case]
    B, cin, cout, ext, last = c["shape"]
    gen = torch.Generator().manual_seed(5000 + ALL.index(case))
    x = torch.randn(B, cin, *ext, generator=gen) + c.get("mean", 0.0)
    if is_transposed(case):
        w = torch.randn(cin, cout, 3, 3, 3, generator=gen) * (27 * cin) ** -0.5
        out = tuple(2 * i - 1 + last for i in ext)
    else:
        w = torch.randn(cout, cin, 3, 3, 3, generator=gen) * (27 * cin) ** -0.5
        out = tuple((i - 1) // last + 1 for i in ext)
    g = torch.randn(B, cout, *out, generator=gen)
    return {"x": x, "w": w, "g": g}


def torchs(case, t, dtype, device="cpu"):
    """{y, dx, dw} of torch's own op on the inputs t, in dtype on device; loss = sum(y g)."""
    last = (TRANSPOSED[case] if is_transposed(case) else CASES[case])["shape"][4]
    x = t["x"].to(device, dtype).requires_grad_(True)
    w = t["w"].to(device, dtype).requires_grad_(True)
    if is_transposed(case):
        y = F.conv_transpose3d(x, w, None, stride=2, padding=1, output_padding=last)
    else:
        y = F.conv3d(x, w, None, stride=last, padding=1)
    (y * t["g"].to(device, dtype)).sum().backward()
    return {"y": y.detach(), "dx": x.grad, "dw": w.grad}


def reference(case):
    """{x, w, g (float32), y64, dx64, dw64, ref_err: {quantity: yardstick}}, computed once and shared."""
    return conv_cases.reference("conv3d", case, lambda: make_inputs(case), lambda t, dtype: torchs(case, t, dtype), QUANTITIES)
