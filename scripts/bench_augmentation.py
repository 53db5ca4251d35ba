"""The SE(3) augmentation (manigaussian_amd.augmentation): the fused op alone, eager and HIP-graph replayed, at B = 1 and B = 8
with 4 cameras of 128 x 128 points and camera poses (ManiGaussian's step), the config's ranges (trans 0.125, rot [0, 0, 45] in
steps of 5, 100 voxels, 10 attempts).

What it times: one call of Se3Augmentation (select + apply + the in-place add that advances the random stream), hipEvent-timed
call by call after warm-up, and the host's wall time of the eager Python call.  Two copies of the same module are alternated so
that the spread of the comparison itself is on record.  What it does NOT time: the reference's sequence -- it needs the
reference tree and pytorch3d, which the GPU box does not have; its cost is a count of synchronisations read from the code
(at least 3 + 2 B device reads per attempt), stated as derived wherever it is quoted.
Writes one JSON document to --out (default profiles/augmentation_bench.json) and prints it on one line.  AB_STEPS: timed calls
per variant (500).  AB_ONLY=1: the eager calls alone, untimed, at both shapes (for `rocprofv3 --kernel-trace --stats`, a run of
its own: profiles/augmentation_kernel_stats.csv holds the se3_* rows of such a run)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from manigaussian_amd import Se3Augmentation, _lib  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = int(os.environ.get("AB_STEPS", "500"))
WARM = 30
CAMS, H, W = 4, 128, 128
BOUNDS = [-0.3, -0.5, 0.6, 0.7, 0.5, 1.6]

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augmentation_bench.json"))
args = ap.parse_args()
dev = torch.device("cuda:0")


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
        out[k] = {"median_ms": t[len(t) // 2], "mean_ms": sum(t) / len(t), "p10_ms": t[len(t) // 10], "p90_ms": t[9 * len(t) // 10],
                  "host_ms_per_call": 1e3 * host[k] / steps}
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


def shape_block(B):
    g = torch.Generator().manual_seed(B)
    lo, hi = torch.tensor(BOUNDS[:3]), torch.tensor(BOUNDS[3:])
    pcd = [(lo.view(1, 3, 1, 1) + (hi - lo).view(1, 3, 1, 1) * torch.rand(B, 3, H, W, generator=g)).to(dev) for _ in range(CAMS)]
    pose = [torch.eye(4).repeat(B, 1, 1).to(dev) for _ in range(CAMS)]
    grip = torch.cat([lo + (hi - lo) * (0.3 + 0.4 * torch.rand(B, 3, generator=g)), torch.tensor([[0.0, 0.0, 0.0, 1.0]]).repeat(B, 1)],
                     1).to(dev)
    a_trans = torch.randint(0, 100, (B, 3), generator=g, dtype=torch.int32).to(dev)
    a_rot = torch.randint(0, 72, (B, 4), generator=g, dtype=torch.int32).to(dev)
    bounds = torch.tensor([BOUNDS], device=dev)
    mods = {k: Se3Augmentation(torch.tensor([0.125] * 3, dtype=torch.float64), [0.0, 0.0, 45.0], 5, 100, 5).to(dev).manual_seed(1)
            for k in ("b_fused", "b2_fused")}
    fns = {k: (lambda m=m: m(pcd, pose, grip, a_trans, a_rot, bounds)) for k, m in mods.items()}
    if os.environ.get("AB_ONLY"):
        for _ in range(STEPS):
            fns["b_fused"]()
        torch.cuda.synchronize()
        return None
    for _ in range(WARM):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    accepted = int(mods["b_fused"].last_info[0]) >= 0
    G = {k: capture(fn) for k, fn in fns.items()}
    for _ in range(WARM):
        for gr in G.values():
            gr.replay()
    out = {"B": B, "cameras": CAMS, "H": H, "W": W, "last_call_accepted": accepted,
           "graph": timed({k: gr.replay for k, gr in G.items()}, STEPS), "eager": timed(fns, STEPS)}
    for mode in ("graph", "eager"):
        t = out[mode]
        out[mode + "_b_b2_spread"] = abs(t["b_fused"]["median_ms"] / t["b2_fused"]["median_ms"] - 1.0)
    # algorithmic bytes: every cloud read once and written once (the actions, poses and the select launch are noise beside them)
    out["cloud_bytes"] = 2 * CAMS * B * 3 * H * W * 4
    out["graph_GBps_of_cloud_bytes"] = out["cloud_bytes"] / (out["graph"]["b_fused"]["median_ms"] * 1e-3) / 1e9
    return out


res = {"steps": STEPS, "build_id": _lib.build_id(), "device": torch.cuda.get_device_name(0),
       "note": "b, b2 = two copies of Se3Augmentation (select + apply + the rng_state add), alternated; median_ms by hipEvents "
               "around each call, host_ms_per_call = wall time of the Python call itself (graph: of replay()).  The reference's "
               "sequence is not timed here (no reference tree, no pytorch3d on the GPU box).",
       "reference_device_reads_per_attempt_derived": "3 + 2 B (voxel/augmentation.py:305,343,347,354,364), up to 10 attempts",
       "shapes": [shape_block(B) for B in (1, 8)]}
if os.environ.get("AB_ONLY"):
    sys.exit(0)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res), flush=True)
