"""Writes tests/golden/volume/<name>.npz from ManiGaussian's own Conv3DBlock and Conv3DUpsampleBlock (helpers/network_utils.py:
129-171, 374-391, loaded unmodified), run on the CPU in float32 and float64 (tests/volume_cases.py: reference_module_case).
Arrays only; every file at most 1 000 000 bytes; every tensor's yardstick (the float32 reference's own error) at most 1e-5,
asserted.  Run from the repository root on a machine that holds the reference:
    python tests/golden/make_golden_volume.py
tests/test_volume.py::test_module_fixtures_match_the_reference re-runs this computation against the committed files."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import volume_cases as vc  # noqa: E402


def main():
    assert vc.have_reference(), f"{vc.REF_FILE} not found"
    os.makedirs(vc.GOLDEN_DIR, exist_ok=True)
    for name in vc.MODULES:
        arrays = vc.reference_module_case(name)
        path = vc.module_fixture_path(name)
        np.savez_compressed(path, **arrays)
        size = os.path.getsize(path)
        assert size <= 1_000_000, (name, size)
        worst = max(float(v) for k, v in arrays.items() if k.startswith("ref_err."))
        print(f"{name}: {size} bytes, out {arrays['out64'].shape}, largest ref_err {worst:.2e}")


if __name__ == "__main__":
    main()
