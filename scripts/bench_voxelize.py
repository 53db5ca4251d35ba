"""The agent's voxelizer: the reference's torch op sequence on the GPU vs the fused call (manigaussian_amd.voxelizer).
Shapes: B = 1, V = 100, Fc = 3, N = 16 384 (ManiGaussian: one 128 x 128 camera) and N = 49 152 (three cameras); a depth-map-like
cloud over the scene bounds with about 30 % of the points outside.
  (a)  voxelize(): four launches, both memory layouts (channels_first is what the Perceiver's Conv3d reads without a copy)
  (b)  this script's torch restatement of voxel/voxel_grid.py:168-229 with the reference's op sequence -- zeros, two
       scatter_add_, clamp, divide, crop, the cats -- and the caller's permute + .contiguous() in front of Conv3d.  Its atomics
       are unordered, so it is compared with (a) to 1e-6 before timing, not bit for bit
  (a2) a second copy of (a): the spread of the comparison itself
alternated step by step in one process, hipEvent-timed after warm-up, eager; (a) also replayed from a HIP graph.
Achieved rate = the algorithmic bytes, B V^3 C 4 + B N (Fc + 3) 4, over the graph-replayed call, as a fraction of the 6.29 TB/s
copy peak measured on an MI355X.
Prints one JSON line and writes it to --out (default profiles/voxelize_bench.json).  BV_STEPS: timed steps (300).
BV_ONLY=a|b: that variant's eager calls only at N = 16 384, untimed (for rocprofv3 --kernel-trace --stats).
Needs a HIP device: there is no CPU path."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from manigaussian_amd import _lib  # noqa: E402
from manigaussian_amd.voxelizer import voxelize  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxelize_bench.json"))
args = ap.parse_args()
STEPS = int(os.environ.get("BV_STEPS", "300"))
WARM = 20
COPY_PEAK = 6.29e12  # bytes/s, the measured device-to-device copy rate of an MI355X
SCENE_BOUNDS = (-0.3, -0.5, 0.6, 0.7, 0.5, 1.6)
assert torch.cuda.is_available(), "bench_voxelize.py needs a HIP device"
dev = torch.device("cuda:0")


def timed(fns, steps):
    """Alternate the step functions; ms per step of each by hipEvents around every call, and the host's wall time per call."""
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
        keep = fn()
    return graph, keep


def cloud(B, N, seed):
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(B, N, 2, generator=g)
    z = 0.8 + 0.3 * u[..., :1] + 0.02 * torch.randn(B, N, 1, generator=g)
    xyz = torch.cat([-0.4 + 1.2 * u[..., :1], -0.6 + 1.2 * u[..., 1:], z], -1).float()
    rgb = torch.randint(0, 256, (B, N, 3), generator=g).float() / 255.0 * 2.0 - 1.0
    return xyz.to(dev), rgb.to(dev)


class TorchVoxelGrid:
    """voxel/voxel_grid.py's forward with torch ops on the device, op for op: the flat (V + 2)^3 grid, the two scatter_add_,
    the crop and the cats; constants that the reference keeps as buffers are built once here as well."""

    def __init__(self, V, B, Fc, N):
        self.V, self.B, self.C, self.N = V, B, Fc + 4, N
        w = V + 2
        self.shape = [B, w, w, w, self.C]
        self.flat = B * w ** 3 * self.C
        self.scales = torch.tensor([w ** 3 * self.C, w * w * self.C, w * self.C, self.C], device=dev)
        self.arange = torch.arange(self.C, device=dev)
        self.ones = torch.ones(B, N, 1, device=dev)
        self.batch = torch.arange(B, dtype=torch.int, device=dev).view(B, 1, 1).repeat(1, N, 1)
        self.dims_m_one = torch.full((1, 3), V + 1, dtype=torch.int, device=dev)
        self.zeros3 = torch.zeros(1, 3, dtype=torch.int, device=dev)
        ar = torch.arange(0, w, dtype=torch.float, device=dev)
        self.index_grid = torch.cat([ar.view(w, 1, 1, 1).repeat(1, w, w, 1), ar.view(1, w, 1, 1).repeat(w, 1, w, 1),
                                     ar.view(1, 1, w, 1).repeat(w, w, 1, 1)], -1).unsqueeze(0).repeat(B, 1, 1, 1, 1)

    def __call__(self, coords, feats, bounds):
        mins, maxs = bounds[..., 0:3], bounds[..., 3:6]
        res = (maxs - mins) / (float(self.V) + 1e-12)
        den = res + 1e-12
        shifted = mins - res
        floor = torch.floor((coords - shifted.unsqueeze(1)) / den.unsqueeze(1)).int()
        idx = torch.max(torch.min(floor, self.dims_m_one), self.zeros3)
        values = torch.cat([feats, coords, self.ones], -1)
        all_idx = torch.cat([self.batch, idx], -1).view(-1, 4)
        flat_idx = ((all_idx * self.scales).sum(-1, keepdim=True).view(-1, 1).repeat(1, self.C) + self.arange).view(-1).long()
        out = torch.zeros(self.flat, device=dev).scatter_add_(0, flat_idx, values.view(-1))
        count = torch.zeros(self.flat, device=dev).scatter_add_(0, flat_idx, torch.ones_like(values.view(-1)))
        count.clamp_(1)
        out.true_divide_(count)
        vox = out.view(self.shape)[:, 1:-1, 1:-1, 1:-1]
        occupied = (vox[..., -1:] > 0).float()
        vox = torch.cat([vox[..., :-1], occupied], -1)
        vox = torch.cat([vox[..., :-1], self.index_grid[:, :-2, :-2, :-2] / float(self.V), vox[..., -1:]], -1)
        return vox.permute(0, 4, 1, 2, 3).contiguous()  # what the Perceiver's Conv3d gets from the caller's permute


def bench(N, seed):
    B, V, Fc = 1, 100, 3
    xyz, rgb = cloud(B, N, seed)
    bounds = torch.tensor([SCENE_BOUNDS], device=dev)
    ref = TorchVoxelGrid(V, B, Fc, N)
    fns = {"a_fused_channels_first": lambda: voxelize(xyz, rgb, bounds, V, "channels_first"),
           "b_torch": lambda: ref(xyz, rgb, bounds),
           "a_fused_channels_last": lambda: voxelize(xyz, rgb, bounds, V, "channels_last"),
           "a2_fused_channels_first": lambda: voxelize(xyz, rgb, bounds, V, "channels_first")}
    a = fns["a_fused_channels_first"]().permute(0, 4, 1, 2, 3)
    b = fns["b_torch"]()
    diff = (a - b).abs().max().item()
    assert a.is_contiguous() and a.shape == b.shape and diff <= 1e-6, diff
    assert torch.equal(fns["a_fused_channels_last"](), a.permute(0, 2, 3, 4, 1))
    occupied = int(a[:, -1].sum().item())
    for _ in range(WARM):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    out = {"shape": {"B": B, "N": N, "V": V, "Fc": Fc}, "occupied_voxels": occupied, "max_abs_diff_a_b": diff,
           "eager": timed(fns, STEPS)}
    graphs = {k: capture(fns[k]) for k in ("a_fused_channels_first", "a_fused_channels_last")}
    for _ in range(WARM):
        for gr, _ in graphs.values():
            gr.replay()
    out["graph"] = timed({k: gr.replay for k, (gr, _) in graphs.items()}, STEPS)
    e = out["eager"]
    fa, fb, fa2 = (e[k]["median_ms"] for k in ("a_fused_channels_first", "b_torch", "a2_fused_channels_first"))
    out["eager_b_over_a_channels_first"] = fb / fa
    out["eager_b_over_a_channels_last"] = fb / e["a_fused_channels_last"]["median_ms"]
    out["eager_a_a2_spread"] = abs(fa / fa2 - 1.0)
    out["faster_by_more_than_the_spread"] = bool(fb / max(fa, fa2) > 1.0 + out["eager_a_a2_spread"])
    nbytes = B * V ** 3 * (Fc + 7) * 4 + B * N * (Fc + 3) * 4
    out["graph_rate"] = {}
    for k, v in out["graph"].items():
        bps = nbytes / (v["median_ms"] * 1e-3)
        out["graph_rate"][k] = {"algorithmic_bytes": nbytes, "TBps": bps / 1e12, "of_copy_peak_6.29": bps / COPY_PEAK}
    out["graph_b_over_a_channels_first"] = fb / out["graph"]["a_fused_channels_first"]["median_ms"]
    return out


only = os.environ.get("BV_ONLY")
if only:  # profiling runs (rocprofv3 --kernel-trace --stats): one variant alone, eager
    xyz, rgb = cloud(1, 16384, 1)
    bounds = torch.tensor([SCENE_BOUNDS], device=dev)
    ref = TorchVoxelGrid(100, 1, 3, 16384)
    for _ in range(STEPS):
        if only == "a":
            voxelize(xyz, rgb, bounds, 100, "channels_first")
            voxelize(xyz, rgb, bounds, 100, "channels_last")
        else:
            ref(xyz, rgb, bounds)
    torch.cuda.synchronize()
    sys.exit(0)

res = {"steps": STEPS, "mgs_build_id": _lib.build_id(),
       "note": "device times are hipEvent medians around each call, variants alternated call by call in one process; (b) is the "
               "reference's op sequence in torch plus the caller's permute + contiguous.  Rates: algorithmic bytes over the "
               "graph-replayed call.",
       "mani_16384": bench(16384, 1), "three_cameras_49152": bench(49152, 2)}
line = json.dumps(res)
print(line, flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write(json.dumps(res, indent=1) + "\n")
for k in ("mani_16384", "three_cameras_49152"):
    assert res[k]["faster_by_more_than_the_spread"], (k, res[k]["eager"])
