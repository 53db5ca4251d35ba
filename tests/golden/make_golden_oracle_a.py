"""Writes tests/golden/oracle_a/identity.npz: what oracle_a.forward_backward (float32, record and pin off) returns for the
two cases of tests/gradient_truth.py IDENTITY_CASES, together with the inputs it ran on.  Recorded at the commit BEFORE
oracle_a.py learned to record and to be pinned; tests/test_gradient_truth.py::test_oracle_a_is_bit_identical_with_record_and_pin_off
holds every later oracle_a.py to these bits.  Arrays only.  Run from the repository root:
    python tests/golden/make_golden_oracle_a.py"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import util  # noqa: E402
from gradient_truth import IDENTITY_CASES  # noqa: E402
from oracle import oracle_a  # noqa: E402


def run(case, sc=None):
    """{array name: numpy array} of one case; sc overrides the generated inputs (the stored ones, bit for bit)."""
    gen, cam, kw, dC, dF = util.scene_case(**case)
    sc = gen if sc is None else sc
    c, f, r, g, aux = oracle_a.forward_backward(sc, types.SimpleNamespace(**kw), dC, dF)
    out = {f"in_{k}": v.numpy() for k, v in sc.items()}
    out.update(out_color=c.numpy(), out_feat=f.numpy(), radii=r.numpy(), point_list=aux["point_list"].numpy(),
               n_contrib=aux["n_contrib"].numpy(), final_T=aux["final_T"].numpy())
    out.update({f"grad_{k}": v.numpy() for k, v in g.items()})
    return out


def main():
    arrays = {}
    for name, case in IDENTITY_CASES.items():
        arrays.update({f"{name}/{k}": v for k, v in run(case).items()})
    os.makedirs(os.path.join(HERE, "oracle_a"), exist_ok=True)
    path = os.path.join(HERE, "oracle_a", "identity.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes,", len(arrays), "arrays")


if __name__ == "__main__":
    main()
