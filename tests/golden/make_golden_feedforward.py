"""Writes tests/golden/feedforward/<name>.npz from ManiGaussian's own PreNorm and FeedForward (agents/manigaussian_bc/
perceiver_lang_io.py:56-99, loaded unmodified), run on the CPU in float32 and float64 (tests/feedforward_cases.py:
reference_module_case).  Arrays only; every file at most 1 000 000 bytes; every tensor's yardstick (the float32 reference's own
error) at most 1e-5, asserted.  Run from the repository root on a machine that holds the reference:
    python tests/golden/make_golden_feedforward.py
tests/test_feedforward.py::test_module_fixtures_match_the_reference re-runs this computation against the committed files."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import feedforward_cases as fc  # noqa: E402


def main():
    assert fc.have_reference(), "the reference's perceiver_lang_io.py was not found"
    os.makedirs(fc.GOLDEN_DIR, exist_ok=True)
    for name in fc.MODULES:
        arrays = fc.reference_module_case(name)
        path = fc.module_fixture_path(name)
        np.savez_compressed(path, **arrays)
        size = os.path.getsize(path)
        assert size <= 1_000_000, (name, size)
        worst = max(float(v) for k, v in arrays.items() if k.startswith("ref_err."))
        print(f"{name}: {size} bytes, out {arrays['out64'].shape}, largest ref_err {worst:.2e}")


if __name__ == "__main__":
    main()
