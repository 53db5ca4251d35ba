"""Generate tests/golden/se3/*.npz: inputs, draw tables and the REFERENCE's results for the SE(3) augmentation.

Run where the reference tree is present:  python tests/golden/make_golden_se3.py
The reference (voxel/augmentation.py and helpers/utils.py, unmodified) is executed on the CPU by tests/se3_cases.py, which also
documents the stand-ins.  A file holds data only: the inputs, the draw table, the batch call's actions, clouds, poses and chosen
attempt, the same for one single-sample call per sample (the truth of retry="sample"), and the least margin of its decisions.

Margins.  The stand-in pytorch3d evaluates in float64 what the real one and the kernel evaluate in fp32, so a discretisation
decision can differ where its float64 value lies within fp32 rounding of a boundary: estimated at <= 3e-5 of a voxel for
|x| <= 100 voxels and <= 1e-5 of a rotation bin.  For every decision of every attempt up to the chosen one -- a voxel coordinate
against the nearest integer, euler / resolution against the nearest half-integer -- the float64 distance to the boundary is
recorded, and a case whose least margin is below se3_cases.MARGIN = 1e-4 bins is drawn again with another seed.  The decisions
that close to a boundary (each costs a draw) must stay below 1 % of all decisions examined: a random one is that close with
probability 2e-4, so the reference alone stays far inside the cap.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import se3_cases as sc  # noqa: E402


def main():
    assert sc.reference() is not None, f"the reference tree is not at {sc.REF_ROOT}"
    os.makedirs(sc.GOLDEN, exist_ok=True)
    examined = discarded = 0
    for idx, spec in enumerate(sc.CASES):
        seed = 1000 * (idx + 1)
        while True:
            case = sc.build_case(spec, seed)
            examined += int(case["decisions"])
            if float(case["margin"]) >= sc.MARGIN:
                break
            discarded += int(case["close"])
            print(f"{spec[0]}: seed {seed} has a decision {float(case['margin']):.2e} bins from its boundary, drawn again")
            seed += 1
        want = {"": (0, 0), "low": (2, 2), "never": (-1, -1), "above": (0, 0)}[spec[8]]
        assert want[0] <= int(case["exp_attempt"]) <= want[1], (spec[0], int(case["exp_attempt"]))
        path = os.path.join(sc.GOLDEN, spec[0] + ".npz")
        np.savez_compressed(path, **case)
        print(f"{spec[0]}: attempt {int(case['exp_attempt'])}, per sample {case['s_attempt'].tolist()}, "
              f"{int(case['decisions'])} decisions, least margin {float(case['margin']):.2e} bins, {os.path.getsize(path)} bytes")
    assert discarded <= 0.01 * examined, f"{discarded} of {examined} decisions were within {sc.MARGIN} bins of a boundary: above 1 %"
    print(f"{examined} decisions examined, {discarded} within {sc.MARGIN} bins of a boundary (their cases drawn again)")


if __name__ == "__main__":
    main()
