"""Writes tests/golden/attention/<case>.npz from ManiGaussian's own Attention class (perceiver_lang_io.py:102-145), loaded
unmodified and run on the CPU in float32 and float64 (tests/attention_cases.py: reference_case).  Arrays only; every file at
most 1 000 000 bytes.  Run from the repository root on a machine that holds the reference:
    python tests/golden/make_golden_attention.py [case ...]
Without arguments only the files that do not exist yet are written: a committed fixture stays byte for byte what it is (the
float64 sums of another CPU may differ in the last bits, and so would the compressed file).  Name a case to write it anew.
tests/test_attention.py::test_fixtures_match_the_reference re-runs this computation against the committed files."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import attention_cases as ac  # noqa: E402


def main():
    assert ac.have_reference(), f"{ac.REF_FILE} not found"
    os.makedirs(ac.GOLDEN_DIR, exist_ok=True)
    unknown = [c for c in sys.argv[1:] if c not in ac.CASES]
    assert not unknown, f"no such case: {unknown}"
    cases = sys.argv[1:] or [c for c in ac.CASES if not os.path.exists(ac.fixture_path(c))]
    for case in cases:
        arrays = ac.reference_case(case)
        path = ac.fixture_path(case)
        np.savez_compressed(path, **arrays)
        size = os.path.getsize(path)
        assert size <= 1_000_000, (case, size)
        err = dict(zip(ac.grad_names(case), arrays["ref_err"]))
        print(f"{case}: {size} bytes, ref_err " + ", ".join(f"{k} {v:.2e}" for k, v in err.items()))


if __name__ == "__main__":
    main()
