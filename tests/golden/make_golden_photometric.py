"""Writes tests/golden/photometric/<case>.npz and window.npz: what the reference's own loss.py gives, in float64, for every
case of tests/photometric_cases.py (run where a copy of the reference exists: `python tests/golden/make_golden_photometric.py`).

Inputs are NOT stored: tests regenerate them from the case's seed (photometric_cases.make_inputs).  Stored per case: terms
[V,4] = (l1, l2, ssim, psnr) and the loss as float64; the gradient with respect to the rendered image rounded to float32 --
whole up to 20 000 elements per view, a fixed stride of about 4 000 elements beyond --; for the case with `ssim_vec` the
gradient of sum_v u[v] ssim[v] as well; and how far the reference's OWN float32 evaluation is from its float64 one
(ref32_value_dev, ref32_grad_dev in units of max |grad|, ref32_grad_abs), from which the tests derive their tolerance.
window.npz holds loss.gaussian(11, 1.5), the eleven float32 window weights.  The directory stays under 1 MB.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import photometric_cases as pc  # noqa: E402


def main():
    assert pc.ref_import.have_reference(), "no copy of the reference: nothing to record"
    os.makedirs(pc.GOLDEN_DIR, exist_ok=True)
    window = pc.reference_module().gaussian(11, 1.5).numpy()
    assert window.dtype == np.float32
    np.savez(os.path.join(pc.GOLDEN_DIR, "window.npz"), window=window)
    total = os.path.getsize(os.path.join(pc.GOLDEN_DIR, "window.npz"))
    for case in pc.CASES:
        inp = pc.make_inputs(case)
        pc.assert_input_classes(case, inp)
        fx = pc.to_fixture(case, inp, pc.reference(case, inp))
        np.savez_compressed(pc.fixture_path(case), **fx)
        size = os.path.getsize(pc.fixture_path(case))
        total += size
        print(f"{case}: {len(fx['elements'])} elements, {size} bytes, loss {float(fx['loss']):.9g}, reference float32 "
              f"against float64: ssim {float(fx['ref32_value_dev']):.3g}, gradient {float(fx['ref32_grad_dev']):.3g} of max "
              f"|grad| ({float(fx['ref32_grad_abs']):.3g} absolute)")
    print("total", total)
    assert total < 1_000_000


if __name__ == "__main__":
    main()
