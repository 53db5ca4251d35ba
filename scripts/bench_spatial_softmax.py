"""The Perceiver's aggregated features -- SpatialSoftmax3D plus the global max-pool of the same volume
(helpers/network_utils.py:927-963, agents/manigaussian_bc/perceiver_lang_io.py:384,485,504) -- three ways, at the three shapes
ManiGaussian runs, fp32:
  ours        manigaussian_amd.spatial_softmax3d(x, with_max=True) (csrc/mgs_spatial_softmax.hip)
  torch       the reference's operations written with torch calls: divide by the temperature, softmax over the row, three products
              with the position tables, three sums, then nn.AdaptiveMaxPool3d(1) on the volume (what the reference executes; its
              text is not here)
  torch_amax  the same with x.amax(dim=(2, 3, 4)) in place of the pooling layer: torch's pooling kernel gives every output
              element to ONE thread, which walks the 10^6 voxels alone, and dominates `torch`; this is the stronger baseline
forward alone and forward + backward (both upstream gradients).  The sides are alternated in one process after warm-up; a figure
is the mean of enough back-to-back calls between two device events to fill SS_WINDOW seconds (0.2), and every round of the sides is
repeated SS_REPEATS times (5): min / median / max are reported, and a speed-up or a saving counts only beyond that spread.
Peak memory: torch.cuda.max_memory_allocated() above the inputs during one forward + backward.  Bytes per second: the
algorithmic bytes (forward 4 rows N: one read; backward 8 rows N: one read, one write) over the median, beside the 6.3 TB/s a
streaming kernel reaches on an MI355X.  Prints one JSON line and writes it to --out (default profiles/spatial_softmax_bench.json).
SS_ONLY=ours|torch|torch_amax: that side's forward + backward only, 20 calls, untimed, at the shape SS_SHAPE names (default ss0_d0): for
rocprofv3 --kernel-trace --stats, whose per-kernel rows then belong to one shape.
Needs a HIP device: there is no CPU path."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from manigaussian_amd import _lib, spatial_softmax3d  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spatial_softmax_bench.json"))
args = ap.parse_args()
WINDOW = float(os.environ.get("SS_WINDOW", "0.2"))
REPEATS = int(os.environ.get("SS_REPEATS", "5"))
ONLY = os.environ.get("SS_ONLY", "")
ONLY_SHAPE = os.environ.get("SS_SHAPE", "ss0_d0")
STREAM_TBS = 6.3
T = 0.01
SHAPES = {"ss0_d0": (1, 128, 100, 100, 100), "ss1_latents": (1, 128, 20, 20, 20), "ss_final": (1, 64, 100, 100, 100)}
assert torch.cuda.is_available(), "bench_spatial_softmax.py needs a HIP device"
dev = torch.device("cuda:0")
maxp = torch.nn.AdaptiveMaxPool3d(1)


def tables(D, H, W):
    px, py, pz = np.meshgrid(np.linspace(-1., 1., D), np.linspace(-1., 1., H), np.linspace(-1., 1., W))
    return tuple(torch.from_numpy(p.reshape(D * H * W)).float().to(dev) for p in (px, py, pz))


def torch_seq(x, pos):
    B, C = x.shape[:2]
    f = x.contiguous().view(-1, pos[0].numel())
    p = torch.softmax(f / T, dim=-1)
    e = torch.cat([torch.sum(t * p, dim=1, keepdim=True) for t in pos], 1)
    return e.view(-1, C * 3), maxp(x).view(B, -1)


def torch_amax(x, pos):
    B, C = x.shape[:2]
    f = x.contiguous().view(-1, pos[0].numel())
    p = torch.softmax(f / T, dim=-1)
    e = torch.cat([torch.sum(t * p, dim=1, keepdim=True) for t in pos], 1)
    return e.view(-1, C * 3), x.amax(dim=(2, 3, 4))


def ours(x, pos):
    return spatial_softmax3d(x, T, with_max=True)


def timed(fn, calls):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e-3 / calls


def figure(fn):
    """Seconds per call: calls sized from a first estimate so that the timed window holds at least WINDOW seconds."""
    est = timed(fn, 2)
    return timed(fn, max(3, int(WINDOW / est) + 1))


def spread(v):
    return dict(min=min(v), median=statistics.median(v), max=max(v))


result = {"build_id": _lib.build_id(), "device": torch.cuda.get_device_name(0), "window_s": WINDOW, "repeats": REPEATS,
          "temperature": T, "stream_TBps": STREAM_TBS, "shapes": {}}
for name, shape in SHAPES.items():
    if ONLY and name != ONLY_SHAPE:
        continue
    B, C, D, H, W = shape
    rows, n = B * C, D * H * W
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(*shape, generator=g) * 0.3 + 0.5).to(dev).requires_grad_(True)
    g_k, g_m = torch.randn(B, 3 * C, generator=g).to(dev), torch.randn(B, C, generator=g).to(dev)
    pos = tables(D, H, W)
    sides = {"ours": ours, "torch": torch_seq, "torch_amax": torch_amax}

    def fwd(side):
        with torch.no_grad():
            sides[side](x, pos)

    def fwd_bwd(side):
        x.grad = None
        kp, mx = sides[side](x, pos)
        torch.autograd.backward([kp, mx], [g_k, g_m])

    if ONLY:
        for _ in range(20):
            fwd_bwd(ONLY)
        torch.cuda.synchronize()
        continue
    for side in sides:  # warm-up: code objects, the workspace, the allocator's pools
        for _ in range(3):
            fwd(side)
            fwd_bwd(side)
    torch.cuda.synchronize()
    x.grad = None
    times = {s: {"forward": [], "forward_backward": []} for s in sides}
    peaks = {s: [] for s in sides}
    for _ in range(REPEATS):
        for side in sides:
            times[side]["forward"].append(figure(lambda: fwd(side)))
        for side in sides:
            times[side]["forward_backward"].append(figure(lambda: fwd_bwd(side)))
        for side in sides:
            x.grad = None
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            fwd_bwd(side)
            torch.cuda.synchronize()
            peaks[side].append(torch.cuda.max_memory_allocated() - base)
            x.grad = None
    # the two sides agree (the torch side in fp32 is no truth: a coarse check that both computed the same thing)
    with torch.no_grad():
        a, b = ours(x, pos), torch_seq(x, pos)
    agree = dict(keypoints=(a[0] - b[0]).abs().max().item(), maxpool=(a[1] - b[1]).abs().max().item())
    bytes_f, bytes_fb = 4 * rows * n, 12 * rows * n
    entry = {"shape": list(shape), "rows": rows, "N": n, "algorithmic_bytes": dict(forward=bytes_f, backward=8 * rows * n),
             "agreement_max_abs": agree, "volume_bytes": 4 * rows * n}
    for side in sides:
        f, fb = spread(times[side]["forward"]), spread(times[side]["forward_backward"])
        entry[side] = dict(forward_s=f, forward_backward_s=fb, peak_alloc_bytes=spread(peaks[side]),
                           forward_TBps=bytes_f / f["median"] / 1e12, forward_backward_TBps=bytes_fb / fb["median"] / 1e12,
                           forward_share_of_stream=bytes_f / f["median"] / 1e12 / STREAM_TBS,
                           forward_backward_share_of_stream=bytes_fb / fb["median"] / 1e12 / STREAM_TBS)
    for base in ("torch", "torch_amax"):  # worst: the baseline's fastest repeat over our slowest
        for what in ("forward", "forward_backward"):
            entry[f"speedup_{what}_over_{base}"] = dict(median=entry[base][what + "_s"]["median"] / entry["ours"][what + "_s"]["median"],
                                                        worst=entry[base][what + "_s"]["min"] / entry["ours"][what + "_s"]["max"])
        entry[f"peak_saving_bytes_worst_over_{base}"] = entry[base]["peak_alloc_bytes"]["min"] - entry["ours"]["peak_alloc_bytes"]["max"]
    result["shapes"][name] = entry
    del x, pos
    torch.cuda.empty_cache()

if not ONLY:
    line = json.dumps(result, sort_keys=True)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
