"""Writes tests/golden/optim/<case>.npz: what the reference's own `Lamb` gives, in float64, for every case of
tests/lamb_cases.py (run where a copy of the reference exists: `python tests/golden/make_golden_lamb.py`).

Inputs are NOT stored: tests regenerate them from the case's seed (lamb_cases.make_inputs / gradients).  Stored per case, all
float64: weight_norm, adam_norm and the recorded trust_ratio of every tensor and step (NaN: the tensor has no state), per-tensor
path = sum_k max |delta p_k|, the per-tensor maxima of |p|, |m|, |v| after the last step (the scales of the bounds), and p, m, v
after the last step -- whole for tensors up to 64 elements, a fixed stride plus the first, last and chunk-boundary elements of
larger ones (lamb_cases.sample_index).  The directory has to stay under 1 MB.

It also measures the reference's OWN float32 run against its float64 run with the comparison the tests use, and prints the
figures: the tests' epsilon (1e-5) is set from these, not from the kernels, and a case whose own float32 error exceeds a quarter
of epsilon has to be shortened.  tests/test_optim.py::test_fixtures_match_the_reference re-runs this file's computation and
requires the committed numbers to match it.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import lamb_cases as lc  # noqa: E402


def main():
    assert lc.have_reference(), "no copy of the reference: nothing to record"
    os.makedirs(lc.GOLDEN_DIR, exist_ok=True)
    total = 0
    for case in lc.CASES:
        inp = lc.make_inputs(case)
        run = lc.reference_run(inp, torch.float64)
        lc.assert_input_classes(case, inp, run)
        fx = lc.to_fixture(run)
        np.savez_compressed(lc.fixture_path(case), **fx)
        size = os.path.getsize(lc.fixture_path(case))
        total += size
        own = lc.compare(case + " (the reference's own float32 run)", lc.reference_run(inp, torch.float32),
                         lc.fixture_of_run(run), inp["K"])
        print(f"{case}: {len(inp['params'])} tensors, {len(fx['p'])} stored elements, {size} bytes")
        assert max(own["stat"], own["m"], own["v"]) <= lc.EPS_REL / 4, "own float32 error above a quarter of epsilon: shorten the case"
    print("total", total)
    assert total < 1_000_000


if __name__ == "__main__":
    main()
