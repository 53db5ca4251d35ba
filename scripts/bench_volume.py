"""The Perceiver decoder's volume plumbing between its convolutions (agents/manigaussian_bc/perceiver_lang_io.py:388, 488-499),
two ways, at the four shapes ManiGaussian runs, fp32:
  ours   manigaussian_amd.resample_pad(sources, scale, pad) (csrc/mgs_volume.hip)
  torch  F.pad(F.interpolate(torch.cat(sources, 1), scale_factor=scale, mode='trilinear', align_corners=False), (pad,) * 6,
         mode='replicate'): what nn.Upsample and nn.Conv3d(padding_mode='replicate') execute ahead of the convolution
The uses:  up0 (one [1,128,20^3] source, scale 5, pad 2), final ([d0, latents]: two [1,128,100^3] sources, pad 1),
trans_decoder ([1,128,100^3], pad 1) and patchify ([1,128,100^3], pad 2).
Every (use, side, forward | forward + backward) variant is a segment of its own: warm-up calls, then VOLUME_RUNS (default 30, at
least 20) calls timed one by one between device events; the median, minimum and maximum are reported.  The segments of the two
sides alternate.  Per variant also: the device kernels of one call (torch.profiler) and the peak allocation above the inputs.
Bytes: what the fused pass has to move (forward: the sources read and the padded output written; backward: the upstream gradient
read, the source gradients written, and for scale > 1 the x y sums written and read once), and the time those bytes take at 5 TB/s.
Prints one JSON line and writes it to --out (default profiles/volume_bench.json), the library's build id beside every number.
VOLUME_ONLY=<use>: that use only.  Needs a HIP device: a CPU has nothing to time."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from manigaussian_amd import _lib, resample_pad  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volume_bench.json"))
args = ap.parse_args()
RUNS = max(20, int(os.environ.get("VOLUME_RUNS", "30")))
WARMUP = int(os.environ.get("VOLUME_WARMUP", "5"))
ONLY = os.environ.get("VOLUME_ONLY", "")
STREAM_TBS = 5.0
# use: (the sources' shapes, scale, pad)
USES = {"up0": (((1, 128, 20, 20, 20),), 5, 2),
        "final": (((1, 128, 100, 100, 100), (1, 128, 100, 100, 100)), 1, 1),
        "trans_decoder": (((1, 128, 100, 100, 100),), 1, 1),
        "patchify": (((1, 128, 100, 100, 100),), 1, 2)}
assert torch.cuda.is_available(), "bench_volume.py needs a HIP device"
dev = torch.device("cuda:0")


def torch_side(sources, scale, pad):
    x = sources[0] if len(sources) == 1 else torch.cat(sources, 1)
    if scale > 1:
        x = F.interpolate(x, scale_factor=scale, mode="trilinear", align_corners=False)
    return F.pad(x, (pad,) * 6, mode="replicate")


SIDES = {"ours": resample_pad, "torch": torch_side}


def bytes_moved(shapes, scale, pad):
    B, _, D, H, W = shapes[0]
    C = sum(s[1] for s in shapes)
    src, out = 4 * B * C * D * H * W, 4 * B * C * (scale * D + 2 * pad) * (scale * H + 2 * pad) * (scale * W + 2 * pad)
    sums = 4 * B * C * (scale * D + 2 * pad) * H * W if scale > 1 else 0
    return dict(forward=src + out, backward=out + src + 2 * sums)


def segment(fn):
    """Warm-up, then RUNS calls timed one by one: seconds, sorted."""
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(RUNS):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        end.record()
        end.synchronize()
        times.append(start.elapsed_time(end) * 1e-3)
    return sorted(times)


def spread(v):
    return dict(min=v[0], median=statistics.median(v), max=v[-1], runs=len(v))


def kernels_of(fn):
    """Device kernels of one call, by name, or the reason they could not be counted."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = {}
        for e in prof.events():
            if str(e.device_type).endswith("CUDA") and not e.name.lower().startswith(("memcpy", "memset")):
                names[e.name[:80]] = names.get(e.name[:80], 0) + 1
        return dict(count=sum(names.values()), by_name=names)
    except Exception as exc:  # noqa: BLE001  (a profiler that does not run on this machine is no reason to lose the timings)
        return dict(count=None, error=f"{type(exc).__name__}: {exc}"[:200])


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


result = {"build_id": _lib.build_id(), "device": torch.cuda.get_device_name(0), "runs": RUNS, "warmup": WARMUP,
          "assumed_stream_TBps": STREAM_TBS, "uses": {}}
for use, (shapes, scale, pad) in USES.items():
    if ONLY and use != ONLY:
        continue
    gen = torch.Generator(device=dev).manual_seed(21)
    sources = [torch.randn(*s, device=dev, generator=gen).requires_grad_(True) for s in shapes]
    with torch.no_grad():
        shape_out = SIDES["torch"](sources, scale, pad).shape
    upstream = torch.randn(*shape_out, device=dev, generator=gen)

    def fwd(side):
        with torch.no_grad():
            SIDES[side](sources, scale, pad)

    def fwd_bwd(side):
        for t in sources:
            t.grad = None
        SIDES[side](sources, scale, pad).backward(upstream)

    moved = bytes_moved(shapes, scale, pad)
    entry = {"sources": [list(s) for s in shapes], "scale": scale, "pad": pad, "out": list(shape_out), "bytes_moved": moved,
             "seconds_at_stream_rate": {k: v / (STREAM_TBS * 1e12) for k, v in moved.items()}, "build_id": _lib.build_id()}
    for side in SIDES:
        entry[side] = {}
    for what, fn in (("forward", fwd), ("forward_backward", fwd_bwd)):
        for side in SIDES:  # the two sides' segments alternate
            call = (lambda s=side, f=fn: f(s))
            entry[side][what + "_s"] = spread(segment(call))
            entry[side][what + "_kernels"] = kernels_of(call)
            entry[side][what + "_peak_alloc_bytes"] = peak_of(call)
            for t in sources:
                t.grad = None
    with torch.no_grad():
        entry["agreement_max_abs"] = (SIDES["ours"](sources, scale, pad) - SIDES["torch"](sources, scale, pad)).abs().max().item()
    for what in ("forward", "forward_backward"):
        ours, theirs = entry["ours"][what + "_s"], entry["torch"][what + "_s"]
        entry[f"speedup_{what}"] = dict(median=theirs["median"] / ours["median"], worst=theirs["min"] / ours["max"])
    fo, fbo = entry["ours"]["forward_s"]["median"], entry["ours"]["forward_backward_s"]["median"]
    entry["ours"]["forward_over_stream_time"] = fo / entry["seconds_at_stream_rate"]["forward"]
    entry["ours"]["backward_over_stream_time"] = (fbo - fo) / entry["seconds_at_stream_rate"]["backward"]
    result["uses"][use] = entry
    del sources, upstream
    torch.cuda.empty_cache()

line = json.dumps(result, sort_keys=True)
print(line)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(result, f, indent=1, sort_keys=True)
    f.write("\n")
