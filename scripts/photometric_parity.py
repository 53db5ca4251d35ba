"""Measures how far the fused photometric loss is from the reference's float64 evaluation on every case of
tests/photometric_cases.py, beside the reference's OWN float32 deviation recorded in the fixtures, and writes
profiles/photometric_parity.json (--out).  The tests assert the bounds; this records the figures.  Needs a HIP device."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import photometric_cases as pc  # noqa: E402
from manigaussian_amd import _lib, photometric  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "photometric_parity.json"))
args = ap.parse_args()
dev = torch.device("cuda:0")
doc = {"build_id": _lib.build_id(), "device": torch.cuda.get_device_name(0), "cases": {},
       "units": "ssim_dev: max |ssim - ssim64| over the views; g_dev: max over the views of max |g - g64| / max |g64| (identical "
                "images: g_abs = max |g|); ref32_*: the reference's own float32 evaluation against its float64 one; bound = "
                "max(1e-5, 4 x ref32)"}
for case, c in pc.CASES.items():
    inp = pc.make_inputs(case)
    color = inp["color"].to(dev).requires_grad_(True)
    target = pc.lay_out(inp["target"], "first" if c["layout"] == "view" else c["layout"]).to(dev)
    loss, terms = photometric.photometric_loss(color, target, weights=c["weights"])
    loss.backward()
    got = dict(loss=loss.detach().cpu(), g=color.grad.cpu(),
               terms=torch.stack([terms["l1"], terms["l2"], terms["ssim"], terms["psnr"]], 1).cpu())
    exp = pc.expected(case)
    m = pc.compare(case, got, exp)
    tol_s, tol_g = pc.ssim_bounds(exp)
    doc["cases"][case] = {"source": exp["source"], "elements_compared": int(len(exp["elements"])) * c["V"],
                          "ssim_dev": m["ssim_dev"], "ssim_bound": tol_s, "ref32_value_dev": exp["ref32_value_dev"],
                          "g_dev": m["g_dev"], "g_bound": tol_g, "ref32_grad_dev": exp["ref32_grad_dev"],
                          "g_abs": got["g"].abs().max().item() if c["cls"] == "identical" else None,
                          "ref32_grad_abs": exp["ref32_grad_abs"]}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(doc, f, indent=1)
print(json.dumps(doc))
