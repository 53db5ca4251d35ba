"""Writes tests/golden/abn/<case>.npz from ManiGaussian's own InPlaceABN (helpers/network_utils.py:219-231, loaded unmodified), run on
the CPU in float32 and float64 (tests/abn_cases.py: reference_case), and tests/golden/abn/stem_state_dict_names.txt, the 62
state_dict names of its MultiLayer3DEncoderShallow.  Arrays only; every file at most 1 000 000 bytes; every case's yardstick (the
float32 reference's own error) at most 2e-4 and no element within 1e-5 of the activation's kink outside a dead channel, both
asserted (a seed that has one is passed over).  Run from the repository root on a machine that holds the reference:
    python tests/golden/make_golden_abn.py
tests/test_encoder.py::test_fixtures_match_the_reference re-runs this computation against the committed files."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import abn_cases as ac  # noqa: E402


def main():
    assert ac.have_reference(), f"{ac.REF_FILE} not found"
    os.makedirs(ac.GOLDEN_DIR, exist_ok=True)
    for case in ac.CASES:
        arrays = ac.reference_case(case)
        path = ac.fixture_path(case)
        np.savez_compressed(path, **arrays)
        size = os.path.getsize(path)
        assert size <= 1_000_000, (case, size)
        errs = ", ".join(f"{q} {e:.2e}" for q, e in zip(ac.QUANTITIES, arrays["ref_err"].tolist()))
        print(f"{case}: {size} bytes, seed {int(arrays['seed'][0])}, ref_err {errs}")
    names = list(ac.load_reference().MultiLayer3DEncoderShallow().state_dict())
    assert len(names) == 62, len(names)
    with open(ac.NAMES_FILE, "w") as f:
        f.write("\n".join(names) + "\n")
    print(f"{len(names)} state_dict names")


if __name__ == "__main__":
    main()
