"""Writes tests/golden/voxelize/*.npz: the inputs of every case of tests/voxelize_cases.py and what ManiGaussian's
voxel/voxel_grid.py (loaded unmodified with importlib, run on the CPU) makes of them.  Runs only where a development copy of the
reference exists; tests/test_voxelizer.py::test_fixtures_match_the_reference re-runs the same computation there.

    python tests/golden/make_golden_voxelize.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import voxelize_cases as vc  # noqa: E402


def main():
    assert vc.have_reference(), f"{vc.REF_FILE} not found"
    os.makedirs(vc.GOLDEN_DIR, exist_ok=True)
    for case in vc.CASES:
        coords, features, bounds, V = vc.make_inputs(case)
        vc.assert_case_is_what_it_claims(case, coords, bounds, V)
        grid = vc.reference_run(coords, features, bounds, V)
        again = vc.reference_run(coords, features, bounds, V)
        assert vc.same_bits(grid, again), f"{case}: the reference's CPU grid differs between two runs"
        out = vc.fixture_of_grid(case, coords, features, bounds, V, grid)
        path = os.path.join(vc.GOLDEN_DIR, case + ".npz")
        np.savez_compressed(path, **out)
        kept, voxels, most = vc.census(coords, bounds, V)
        print(f"{case}: {os.path.getsize(path)} bytes, {kept} of {coords.shape[0] * coords.shape[1]} points kept, "
              f"{voxels} voxels, at most {most} points in one")
        assert os.path.getsize(path) <= 1_000_000, path


if __name__ == "__main__":
    main()
