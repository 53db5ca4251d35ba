"""What the case files of the four Conv3d families share (tests/conv3d_cases.py, pointwise_cases.py, narrow_conv_cases.py,
dense_conv_cases.py) -- TEST INFRASTRUCTURE.

The reference is torch's own op on the CPU, computed at test time, once per case and shared (do not modify what reference()
returns): in float64 -- the truth -- and in float32 -- the yardstick: its largest deviation from the truth over the truth's largest
magnitude.  The bound is abn_cases': error <= 16 x max(yardstick, 2^-23) x max|truth|; a case whose yardstick exceeds
abn_cases.REF_ERR_CEILING is refused, not loosened.

A family's own file keeps its CASES table, make_inputs, torchs, its kernels' tile constants and its exact-integer inputs.
"""
import torch

from abn_cases import FACTOR, FLOOR, REF_ERR_CEILING, bound  # noqa: F401
from numerics import same_bits  # noqa: F401


def has_bias(cases, case):
    """The fifth entry of a case's shape, where the family writes it there."""
    return cases[case]["shape"][4]


def quantities(bias):
    return ("y", "dx", "dw", "db") if bias else ("y", "dx", "dw")


def yardstick(r32, r64):
    """The float32 CPU run's largest deviation from the float64 truth over the truth's largest magnitude."""
    return (r32.double() - r64).abs().max().item() / r64.abs().max().item()


_REFERENCES = {}


def reference(family, case, inputs, torchs, quantities, also=()):
    """{the inputs (float32), <q>64 for q in quantities and in also, ref_err: {quantity: yardstick}} of (family, case), computed once
    and shared.  inputs(): the case's tensors; torchs(t, dtype): torch's results on them; `also`: results of the float64 run kept
    beside the truths, without a yardstick."""
    if (family, case) not in _REFERENCES:
        t = inputs()
        r64, r32 = torchs(t, torch.float64), torchs(t, torch.float32)
        r = dict(t)
        for k in also:
            r[k + "64"] = r64[k]
        r["ref_err"] = {}
        for q in quantities:
            r[q + "64"] = r64[q]
            r["ref_err"][q] = yardstick(r32[q], r64[q])
        _REFERENCES[(family, case)] = r
    return _REFERENCES[(family, case)]
