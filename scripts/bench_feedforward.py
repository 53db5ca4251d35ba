"""What a Perceiver transformer block does beside its attention (agents/manigaussian_bc/perceiver_lang_io.py:56-99), two ways, at
the shapes ManiGaussian runs, fp32:
  ours   manigaussian_amd.layer_norm / bias_geglu / PreNorm(FeedForward) with both ops routed through csrc/mgs_feedforward.hip
  torch  the reference's op sequence on the same GPU: F.layer_norm; (h + bias).chunk(2, -1), a * F.gelu(gates);
         nn.LayerNorm + nn.Sequential(nn.Linear, GEGLU, nn.Linear)
The uses:  ln_latents (layer_norm at [2048, 512]), ln_sequence (layer_norm at [8077, 128]), geglu_hidden (bias_geglu at
[2048, 4096] with the first linear's bias) and block (one whole PreNorm(512, FeedForward(512)) at [1, 2048, 512]; there also
"ours_geglu_only": the same drop-ins with the layer norm left to torch).
Every (use, side, forward | forward + backward) variant is a segment of its own: FEEDFORWARD_WARMUP (5) calls, then
FEEDFORWARD_RUNS (default 30, at least 20) calls timed one by one between device events; the median, minimum and maximum are
reported, and the worst of ours against the best of torch's beside the medians' ratio.  The segments of the two sides alternate.
Per variant also the peak allocation above the inputs.
Bytes (DERIVED from the shapes, not measured): what one fused pass has to move, and the time those bytes take at 5 TB/s.
Without --use, every use runs in a child process of its own under `timeout` (a use that faults, hangs or fails ends the run: no
later use is started); the children's results are merged, printed as one JSON line and written to --out (default
profiles/feedforward_bench.json), the library's build id inside.  Needs a HIP device: a CPU has nothing to time."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

USES = ("ln_latents", "ln_sequence", "geglu_hidden", "block")
STEP_TIMEOUT_S = 240
STREAM_TBS = 5.0
RUNS = max(20, int(os.environ.get("FEEDFORWARD_RUNS", "30")))
WARMUP = int(os.environ.get("FEEDFORWARD_WARMUP", "5"))


def parent(out_path):
    from manigaussian_amd import _lib
    result = {"build_id": _lib.build_id(), "runs": RUNS, "warmup": WARMUP, "assumed_stream_TBps": STREAM_TBS,
              "bytes_are": "derived from the shapes", "uses": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for use in USES:
            part = os.path.join(tmp, use + ".json")
            rc = subprocess.call(["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--use", use,
                                  "--out", part])
            if rc != 0:
                print(f"bench_feedforward: use {use} ended with status {rc}; nothing more is started", file=sys.stderr)
                return rc
            with open(part) as f:
                entry = json.load(f)
            result["device"] = entry.pop("device")
            result["uses"][use] = entry
    print(json.dumps(result, sort_keys=True))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


def child(use, out_path):
    import torch
    import torch.nn.functional as F
    from torch import nn

    from manigaussian_amd import FeedForward, PreNorm, _lib, bias_geglu, feedforward, layer_norm

    assert torch.cuda.is_available(), "bench_feedforward.py needs a HIP device"
    feedforward.ROUTE.update(layer_norm=True, bias_geglu=True)   # "ours" is the kernels, whatever the drop-ins' routing
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(23)

    def randn(*shape):
        return torch.randn(*shape, device=dev, generator=gen)

    def torch_geglu(h, b):
        a, gates = (h + b).chunk(2, dim=-1)
        return a * F.gelu(gates)

    class TorchGEGLU(nn.Module):
        def forward(self, x):
            x, gates = x.chunk(2, dim=-1)
            return x * F.gelu(gates)

    moved = None
    if use in ("ln_latents", "ln_sequence"):
        rows, D = (2048, 512) if use == "ln_latents" else (8077, 128)
        leaves = [randn(rows, D).requires_grad_(True), randn(D).requires_grad_(True), randn(D).requires_grad_(True)]
        sides = {"ours": lambda: layer_norm(*leaves), "torch": lambda: F.layer_norm(leaves[0], (D,), leaves[1], leaves[2])}
        moved = dict(forward=2 * rows * D * 4, backward=3 * rows * D * 4)
        shape = [rows, D]
    elif use == "geglu_hidden":
        rows, M = 2048, 2048
        leaves = [randn(rows, 2 * M).requires_grad_(True), randn(2 * M).requires_grad_(True)]
        sides = {"ours": lambda: bias_geglu(*leaves), "torch": lambda: torch_geglu(*leaves)}
        moved = dict(forward=3 * rows * M * 4, backward=5 * rows * M * 4)
        shape = [rows, 2 * M]
    else:
        torch.manual_seed(24)
        ours = PreNorm(512, FeedForward(512)).to(dev)
        theirs_fn = nn.Sequential(nn.Linear(512, 4096), TorchGEGLU(), nn.Linear(2048, 512))
        theirs_norm = nn.LayerNorm(512)
        theirs_fn.load_state_dict(ours.fn.net.state_dict(), strict=True)
        theirs_norm.load_state_dict(ours.norm.state_dict(), strict=True)
        theirs_fn, theirs_norm = theirs_fn.to(dev), theirs_norm.to(dev)
        x = randn(1, 2048, 512).requires_grad_(True)
        leaves = [x] + list(ours.parameters()) + list(theirs_fn.parameters()) + list(theirs_norm.parameters())

        def geglu_only():   # the block with the layer norm left to torch
            feedforward.ROUTE["layer_norm"] = False
            try:
                return ours(x)
            finally:
                feedforward.ROUTE["layer_norm"] = True

        sides = {"ours": lambda: ours(x), "ours_geglu_only": geglu_only, "torch": lambda: theirs_fn(theirs_norm(x))}
        shape = [1, 2048, 512]
    with torch.no_grad():
        upstream = randn(*sides["torch"]().shape)

    def fwd(side):
        with torch.no_grad():
            sides[side]()

    def fwd_bwd(side):
        for t in leaves:
            t.grad = None
        sides[side]().backward(upstream)

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

    def peak_of(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    entry = {"device": torch.cuda.get_device_name(0), "shape": shape, "build_id": _lib.build_id()}
    entry.update({side: {} for side in sides})
    if moved is not None:
        entry["bytes_moved_derived"] = moved
        entry["seconds_at_stream_rate_derived"] = {k: v / (STREAM_TBS * 1e12) for k, v in moved.items()}
    for what, fn in (("forward", fwd), ("forward_backward", fwd_bwd)):
        for side in sides:  # the two sides' segments alternate
            call = (lambda s=side, f=fn: f(s))
            entry[side][what + "_s"] = spread(segment(call))
            entry[side][what + "_peak_alloc_bytes"] = peak_of(call)
            for t in leaves:
                t.grad = None
    with torch.no_grad():
        entry["agreement_max_abs"] = (sides["ours"]() - sides["torch"]()).abs().max().item()
    for side in sides:
        if side == "torch":
            continue
        for what in ("forward", "forward_backward"):
            a, b = entry[side][what + "_s"], entry["torch"][what + "_s"]
            entry[side][f"speedup_{what}"] = dict(median=b["median"] / a["median"], worst=b["min"] / a["max"])
        entry[side]["below_torch"] = all(entry[side][w + "_s"]["median"] < entry["torch"][w + "_s"]["median"]
                                         for w in ("forward", "forward_backward"))
    if moved is not None:
        fo, fbo = entry["ours"]["forward_s"]["median"], entry["ours"]["forward_backward_s"]["median"]
        entry["ours"]["forward_over_stream_time"] = fo / entry["seconds_at_stream_rate_derived"]["forward"]
        entry["ours"]["backward_over_stream_time"] = (fbo - fo) / entry["seconds_at_stream_rate_derived"]["backward"]
    with open(out_path, "w") as f:
        json.dump(entry, f, sort_keys=True)
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feedforward_bench.json"))
    ap.add_argument("--use", choices=USES, default=None, help="run this use alone, in this process, and write its entry to --out")
    args = ap.parse_args()
    sys.exit(child(args.use, args.out) if args.use else parent(args.out))
