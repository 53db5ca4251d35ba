"""Writes tests/golden/loss/<case>.npz: what the reference's own loss code gives, in float64, for every case of
tests/loss_cases.py (run where a copy of the reference exists: `python tests/golden/make_golden_loss.py`).

Inputs are NOT stored: tests regenerate them from the case's seed (loss_cases.make_inputs).  Stored per case: terms [V,3] =
(mse, embed, psnr) and the loss as float64, and the gradients w.r.t. the rendered colour and feature images rounded to
float32 (6e-8 relative, against a test tolerance of 1e-5) at the pixels listed in `pixels`.  The directory has to stay under
1 MB, and ONE whole float32 gradient of a 128 x 128, F = 3 view is already 393 KB; so the whole gradient is kept for the
single-view case `static_v1`, and every other case keeps a fixed stride of pixels plus all of its special pixels (|e_p| =
1e-9, 2e-8, the zero-norm target pixel).  Where the reference is present the tests compare every pixel against the live
computation instead, and tests/test_losses.py::test_fixtures_match_the_reference re-runs this file's computation and
requires the committed numbers to match it.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import loss_cases as lc  # noqa: E402


def main():
    assert lc.ref_import.have_reference(), "no copy of the reference: nothing to record"
    os.makedirs(lc.GOLDEN_DIR, exist_ok=True)
    total = 0
    for case in lc.CASES:
        inp, special = lc.make_inputs(case)
        lc.assert_input_classes(case, inp, special)
        fx = lc.to_fixture(case, lc.reference(case, inp), special)
        np.savez_compressed(lc.fixture_path(case), **fx)
        size = os.path.getsize(lc.fixture_path(case))
        total += size
        print(f"{case}: {len(fx['pixels'])} pixels, {size} bytes, loss {float(fx['loss']):.9g}")
    print("total", total)
    assert total < 1_000_000


if __name__ == "__main__":
    main()
