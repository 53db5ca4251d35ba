"""Writes tests/golden/spatial_softmax/<case>.npz from ManiGaussian's own SpatialSoftmax3D (helpers/network_utils.py:927-963,
loaded unmodified) and nn.AdaptiveMaxPool3d(1), run on the CPU in float32 and float64 (tests/spatial_softmax_cases.py:
reference_case).  Arrays only; every file at most 1 000 000 bytes; every case's yardstick (the float32 reference's own error)
at most 2e-4, asserted.  Run from the repository root on a machine that holds the reference:
    python tests/golden/make_golden_spatial_softmax.py
tests/test_spatial_softmax.py::test_fixtures_match_the_reference re-runs this computation against the committed files."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import spatial_softmax_cases as sc  # noqa: E402


def main():
    assert sc.have_reference(), f"{sc.REF_FILE} not found"
    os.makedirs(sc.GOLDEN_DIR, exist_ok=True)
    for case in sc.CASES:
        arrays = sc.reference_case(case)
        path = sc.fixture_path(case)
        np.savez_compressed(path, **arrays)
        size = os.path.getsize(path)
        assert size <= 1_000_000, (case, size)
        e = [float(arrays["ref_abs_err"])] + arrays["ref_err"].tolist()
        first = sc.first_argmax(sc.make_inputs(case)[0])
        print(f"{case}: {size} bytes, ref_abs_err kp {e[0]:.2e}, ref_err dx {e[1]:.2e}, dx_k {e[2]:.2e}, argmax {first.tolist()}")


if __name__ == "__main__":
    main()
