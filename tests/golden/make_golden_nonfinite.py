"""Writes tests/golden/nonfinite/<subject>.npz: for every subject of tests/test_nonfinite.py whose truth is a restatement written in
this repository, the classes (uint8: 0 finite, 1 NaN, 2 +inf, 3 -inf) of every result of the REFERENCE's own module, in float64 on
the CPU, for every tainted input of the subject.  Arrays only.  Needs a copy of the reference (tests/ref_import.py says where).

    python tests/golden/make_golden_nonfinite.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import test_nonfinite as tn  # noqa: E402

if __name__ == "__main__":
    os.makedirs(tn.GOLDEN_DIR, exist_ok=True)
    for key in tn.RESTATED:
        s = tn.SUBJECTS[key]
        assert s.have_reference(), f"{key}: no copy of the reference on this machine"
        maps = tn.class_maps(s, s.reference_module)
        np.savez_compressed(tn.golden_path(key), **maps)
        print(key, len(maps), "maps,", os.path.getsize(tn.golden_path(key)), "bytes")
