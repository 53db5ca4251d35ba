"""The photometric loss (L1 + D-SSIM): the reference formula in torch vs the fused pass (manigaussian_amd.photometric).
For V = 2, 3 x 128^2 (ManiGaussian's step) and V = 8, 3 x 256^2, on leaf images (no render):
  (a)  loss.py's formula restated here -- conv2d with groups = C on an 11 x 11 window, the elementwise SSIM map, mean |x - y|,
       the weighted sum -- and its autograd backward
  (b)  photometric_loss and its backward
  (a2) a second copy of (a): the spread of the comparison itself
forward alone and forward + backward, alternated call by call in one process, hipEvent-timed after warm-up, eager and HIP-graph
replayed; the host's wall time per eager call (the Python enqueue path); the peak allocation of one forward + backward; the
fused pass's algorithmic bytes over its graph-replayed time.
Writes one JSON document to --out (default profiles/photometric_bench.json) and prints it on one line.
PB_STEPS: timed calls per variant (300).  PB_ONLY=a|b: run that variant's eager forward + backward only, untimed, at both
shapes (for `rocprofv3 --kernel-trace --stats`, a run of its own); --kernel-stats CSV merges such a run's per-kernel device
times of the photometric_* kernels into the document."""
import argparse
import csv
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import manigaussian_amd as mg  # noqa: E402
from manigaussian_amd import _lib, photometric  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = int(os.environ.get("PB_STEPS", "300"))
WARM = 20
LAMBDA = 0.2
SHAPES = [(2, 3, 128, 128), (8, 3, 256, 256)]


def merge_kernel_stats(doc_path, csv_path):
    with open(doc_path) as f:
        doc = json.load(f)
    rows = []
    with open(csv_path) as f:
        for r in csv.DictReader(f):
            if "photometric" in r.get("Name", ""):
                rows.append({"kernel": r["Name"].split("(")[0], "calls": int(r["Calls"]),
                             "mean_us": float(r["AverageNs"]) / 1e3, "min_us": float(r["MinNs"]) / 1e3,
                             "max_us": float(r["MaxNs"]) / 1e3})
    doc["kernel_device_times"] = {"source": "rocprofv3 --kernel-trace --stats, PB_ONLY=b (both shapes in one run: the mean is "
                                            "over both, min is the small shape, max the large one)", "kernels": rows}
    with open(doc_path, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc["kernel_device_times"]))


ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "photometric_bench.json"))
ap.add_argument("--kernel-stats", default=None)
args = ap.parse_args()
if args.kernel_stats:
    merge_kernel_stats(args.out, args.kernel_stats)
    sys.exit(0)

dev = torch.device("cuda:0")
torch.autograd.set_multithreading_enabled(False)


def timed(fns, steps):
    """Alternate the functions; ms per call of each by hipEvents around every call, and the host's wall time per call."""
    ev = {k: [] for k in fns}
    host = {k: 0.0 for k in fns}
    for _ in range(steps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t0 = time.perf_counter()
            fn()
            host[k] += time.perf_counter() - t0
            e1.record()
            ev[k].append((e0, e1))
    torch.cuda.synchronize()
    out = {}
    for k, lst in ev.items():
        t = sorted(a.elapsed_time(b) for a, b in lst)
        out[k] = {"median_ms": t[len(t) // 2], "mean_ms": sum(t) / len(t), "host_ms_per_call": 1e3 * host[k] / steps}
    return out


def capture(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph


def torch_window(C):
    g = torch.tensor(photometric.WINDOW, dtype=torch.float32).unsqueeze(1)
    return g.mm(g.t()).float().expand(C, 1, 11, 11).contiguous().to(dev)


def torch_loss(x, y, window, weights):
    """loss.py:9-10 and :48-68 for V views, one batched call (the reference formula, channel-first)."""
    C = x.size(1)
    mu1, mu2 = F.conv2d(x, window, padding=5, groups=C), F.conv2d(y, window, padding=5, groups=C)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1 = F.conv2d(x * x, window, padding=5, groups=C) - mu1_sq
    s2 = F.conv2d(y * y, window, padding=5, groups=C) - mu2_sq
    s12 = F.conv2d(x * y, window, padding=5, groups=C) - mu1_mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    m = ((2 * mu1_mu2 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))
    ssim = m.mean((1, 2, 3))
    l1 = (x - y).abs().mean((1, 2, 3))
    return (weights[:, 0] * l1 + weights[:, 2] * (1 - ssim)).sum()


def shape_block(V, C, H, W):
    gg = torch.Generator().manual_seed(3)
    x = torch.rand(V, C, H, W, generator=gg).to(dev).requires_grad_(True)
    y = torch.rand(V, C, H, W, generator=gg).to(dev)
    w_dev = torch.tensor([[1.0 - LAMBDA, 0.0, LAMBDA]] * V, dtype=torch.float32).to(dev)
    window = torch_window(C)

    def a_fwd():
        with torch.no_grad():
            return torch_loss(x, y, window, w_dev)

    def a_fb():
        return torch.autograd.grad(torch_loss(x, y, window, w_dev), [x])

    def b_fwd():
        with torch.no_grad():
            return photometric.photometric_loss(x, y, weights=w_dev)[0]

    def b_fb():
        return torch.autograd.grad(photometric.photometric_loss(x, y, weights=w_dev)[0], [x])

    only = os.environ.get("PB_ONLY")
    if only:
        fn = {"a": a_fb, "b": b_fb}[only]
        for _ in range(STEPS):
            fn()
        torch.cuda.synchronize()
        return None
    for _ in range(WARM):
        a_fwd(), a_fb(), b_fwd(), b_fb()
    torch.cuda.synchronize()
    out = {"V": V, "C": C, "H": H, "W": W}
    (ga,), (gb,) = a_fb(), b_fb()
    out["loss_a"], out["loss_b"] = a_fwd().item(), b_fwd().item()
    out["max_rel_grad_diff"] = ((gb - ga).abs().max() / ga.abs().max()).item()
    del ga, gb
    peak = {}
    for k, fn in (("a_torch", a_fb), ("b_fused", b_fb)):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        peak[k] = torch.cuda.max_memory_allocated() - base
    out["peak_allocation_bytes_fwd_bwd"] = peak
    for name, fa, fb in (("forward", a_fwd, b_fwd), ("forward_backward", a_fb, b_fb)):
        G = {"a_torch": capture(fa), "b_fused": capture(fb), "a2_torch": capture(fa)}
        for _ in range(WARM):
            for gr in G.values():
                gr.replay()
        r = {"graph": timed({k: gr.replay for k, gr in G.items()}, STEPS),
             "eager": timed({"a_torch": fa, "b_fused": fb, "a2_torch": fa}, STEPS)}
        for mode in ("graph", "eager"):
            t = r[mode]
            r[mode + "_a_over_b"] = t["a_torch"]["median_ms"] / t["b_fused"]["median_ms"]
            r[mode + "_a_a2_spread"] = abs(t["a_torch"]["median_ms"] / t["a2_torch"]["median_ms"] - 1.0)
        out[name] = r
        del G
    # algorithmic bytes of the fused forward + backward: the forward kernel reads x and y and writes three maps,
    # the gradient kernel reads the three maps, x and y and writes the unit gradient, the backward reads it and writes the result
    n = V * C * H * W * 4
    out["fused_bytes_fwd_bwd"] = (2 + 3) * n + (3 + 2 + 1) * n + 2 * n
    out["fused_graph_GBps_fwd_bwd"] = out["fused_bytes_fwd_bwd"] / (out["forward_backward"]["graph"]["b_fused"]["median_ms"] * 1e-3) / 1e9
    return out


res = {"steps": STEPS, "build_id": _lib.build_id(), "device": torch.cuda.get_device_name(0), "lambda_ssim": LAMBDA,
       "note": "a = the reference formula in torch (conv2d, groups = C), b = photometric_loss; leaf images, no render; "
               "median_ms by hipEvents around each call, host_ms_per_call = wall time of the Python call itself"}
blocks = [shape_block(*s) for s in SHAPES]
if os.environ.get("PB_ONLY"):
    sys.exit(0)
res["shapes"] = blocks
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res), flush=True)
