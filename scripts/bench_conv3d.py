"""The voxel encoder stem's ten 3x3x3 convolution sites (helpers/network_utils.py:248-306), two ways, at the shapes ManiGaussian runs
(B = 1, a 100^3 grid), fp32:
  op     manigaussian_amd.conv3d / conv_transpose3d (csrc/mgs_conv3d.hip)
  torch  F.conv3d / F.conv_transpose3d on the same GPU, with torch.backends.cudnn.benchmark off (`torch`) and on (`torch_benchmark`)
Per site, in ONE process, the sides alternating:
  passes_us         the three passes on their own, eager: forward, backward_data and backward_weight of the SITE'S op (for a
                    transposed site the library's backward_data / forward / backward_weight kernels, in that order); torch's through
                    aten.convolution_backward with one output asked for, cudnn.benchmark off;
  forward, forward_backward   as in a training step (autograd recording; gradients towards x and the weight), each EAGER (calls from
                    Python) and GRAPH-REPLAYED (one call captured into a HIP graph), three sides;
  peak_bytes        the peak allocation of one eager forward + backward above what was held before.
A sample is `inner` consecutive calls between two device events, `inner` chosen so that a sample lasts about SAMPLE_MS; CONV_RUNS
(default 7) samples per side; reported: median, quartiles, minimum, maximum, in microseconds per call.
`op_wins`: in all four (pass, form) pairs the op's third quartile lies below the first quartile of torch's faster setting (the one with
the lower median) -- encoder.fused_site()'s criterion.  manigaussian_amd/encoder.py's conv_site() is set from these.
Then the whole stem, forward + backward at [1, 10, 100^3]: CONV following the rule (`rule`), forced on (`conv_on`) and off (`conv_off`),
and the parent commit's two figures re-measured in the same run: every normalisation site fused and the convolutions torch's
(`parent_fused`: encoder.FORCE = True, CONV = False) and everything torch's (`parent_torch`: FORCE = False).
FLOP and byte counts are DERIVED from the shapes (taps that fall into the padding are counted), not measured; times are measured.
Every site, and the stem, is timed in a child process of its own under `timeout`; the first child that fails ends the run.
Writes --out (default profiles/conv3d_bench.json) and prints it as one JSON line.  Needs a HIP device: a CPU has nothing to time."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# site, channels in and out OF THE SITE'S OP, levels below the grid of its input and output (100, 50, 25, 13), transposed, output padding
SITES = (("conv0", 10, 8, 0, 0, False, 0), ("conv1", 8, 16, 0, 1, False, 0), ("conv2", 16, 16, 1, 1, False, 0),
         ("conv3", 16, 32, 1, 2, False, 0), ("conv4", 32, 32, 2, 2, False, 0), ("conv5", 32, 64, 2, 3, False, 0),
         ("conv6", 64, 64, 3, 3, False, 0), ("conv7", 64, 32, 3, 2, True, 0), ("conv9", 32, 16, 2, 1, True, 1),
         ("conv11", 16, 8, 1, 0, True, 1))
RUNS = max(5, int(os.environ.get("CONV_RUNS", "7")))
WARMUP = 2
SAMPLE_MS = 4.0
MAX_INNER = 100
SITE_TIMEOUT_S = int(os.environ.get("CONV_SITE_TIMEOUT", "240"))
STEM_TIMEOUT_S = int(os.environ.get("CONV_STEM_TIMEOUT", "420"))
PARENT_MS = {"parent_fused": 343.9, "parent_torch": 343.1}   # profiles/encoder_bench.json, the stem's eager medians at the parent commit


def say(msg):
    print("bench_conv3d:", msg, file=sys.stderr, flush=True)


def side_of(grid, level):
    for _ in range(level):
        grid = (grid + 1) // 2
    return grid


def site_shape(site, grid):
    """What conv_site() and the derived counts look at: the convolution the site runs or transposes."""
    name, ci, co, lin, lout, transposed, op = site
    s_in, s_out = side_of(grid, lin), side_of(grid, lout)
    stride = 1 if lin == lout else 2
    big, small = (s_out, s_in) if transposed else (s_in, s_out)     # the convolution's input and output sides
    cin, cout = (co, ci) if transposed else (ci, co)                # ... and channels
    flop = 2 * 27 * cin * cout * small ** 3
    volumes = 4 * (cin * big ** 3 + cout * small ** 3)
    return {"cin": cin, "cout": cout, "side": big, "voxels": big ** 3, "stride": stride, "transposed": transposed, "output_padding": op,
            "op_shape": {"x": [1, ci, s_in, s_in, s_in], "y": [1, co, s_out, s_out, s_out]},
            "derived": {"flop_per_pass": flop, "flop_forward_backward": 3 * flop, "bytes_volumes": volumes,
                        "bytes_weight": 4 * 27 * cin * cout, "note": "derived from the shapes, not measured"}}


def summary(samples):
    s = sorted(samples)
    q = statistics.quantiles(s, n=4, method="inclusive")
    return {"median_us": round(statistics.median(s), 2), "q1_us": round(q[0], 2), "q3_us": round(q[2], 2), "min_us": round(s[0], 2),
            "max_us": round(s[-1], 2)}


def op_wins(entry, benchmark_may_be_missing=False):
    """benchmark_may_be_missing (bench_dense.py): a torch_benchmark side that did not finish is not compared."""
    for p in ("forward", "forward_backward"):
        for f in ("eager", "graph"):
            sides = entry[p][f]
            torchs = ("torch", "torch_benchmark")
            if benchmark_may_be_missing:
                torchs = [s for s in torchs if s in sides and "median_us" in sides[s]]
            t = min((sides[s] for s in torchs), key=lambda s: s["median_us"])
            if not sides["op"]["q3_us"] < t["q1_us"]:
                return False
    return True


class Timer:
    def __init__(self, torch):
        self.torch = torch

    def sample(self, call, inner):
        torch = self.torch
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(inner):
            call()
        end.record()
        end.synchronize()
        return start.elapsed_time(end) * 1000.0 / inner

    def inner_for(self, call):
        for _ in range(WARMUP):
            call()
        self.torch.cuda.synchronize()
        est = self.sample(call, 2)
        return max(1, min(MAX_INNER, int(SAMPLE_MS * 1000.0 / max(est, 1.0))))

    def peak_of(self, call):
        torch = self.torch
        call()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        call()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    def captured(self, call):
        torch = self.torch
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(WARMUP):
                call()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            call()
        torch.cuda.synchronize()
        return graph

    def alternate(self, run):
        """{side: callable} -> {side: summary + inner}; the sides' samples alternate."""
        inner = {k: self.inner_for(c) for k, c in run.items()}
        samples = {k: [] for k in run}
        for _ in range(RUNS):
            for k, c in run.items():
                samples[k].append(self.sample(c, inner[k]))
        return {k: dict(summary(v), inner=inner[k]) for k, v in samples.items()}

    def compare(self, calls, peak=False):
        """{side: callable} -> {form: {side: summary}}"""
        out = {"eager": self.alternate(calls)}
        if peak:
            for k, c in calls.items():
                out["eager"][k]["peak_bytes"] = self.peak_of(c)
        graphs = {k: self.captured(c) for k, c in calls.items()}
        out["graph"] = self.alternate({k: g.replay for k, g in graphs.items()})
        return out


def benchmark_on(torch, call):
    def wrapped():
        torch.backends.cudnn.benchmark = True
        try:
            return call()
        finally:
            torch.backends.cudnn.benchmark = False
    return wrapped


def measure_site(site, grid):
    import importlib

    import torch
    import torch.nn.functional as F

    cv = importlib.import_module("manigaussian_amd.conv3d")
    dev = torch.device("cuda:0")
    torch.backends.cudnn.benchmark = False
    tm = Timer(torch)
    name, ci, co, lin, lout, transposed, op = site
    shape = site_shape(site, grid)
    stride = 2 if transposed else shape["stride"]
    gen = torch.Generator().manual_seed(9)
    x = torch.randn(*shape["op_shape"]["x"], generator=gen).to(dev).requires_grad_(True)
    g = torch.randn(*shape["op_shape"]["y"], generator=gen).to(dev)
    wshape = (ci, co, 3, 3, 3) if transposed else (co, ci, 3, 3, 3)
    w = (torch.randn(*wshape, generator=gen) * (27 * ci) ** -0.5).to(dev).requires_grad_(True)

    if transposed:
        def fwd_torch():
            return F.conv_transpose3d(x, w, None, stride=2, padding=1, output_padding=op)

        def fwd_op():
            return cv.conv_transpose3d(x, w, op)
    else:
        def fwd_torch():
            return F.conv3d(x, w, None, stride=stride, padding=1)

        def fwd_op():
            return cv.conv3d(x, w, stride)

    def both(fwd):
        return lambda: torch.autograd.grad(fwd(), [x, w], g)

    # the three passes on their own
    xd, wd = x.detach(), w.detach()
    y_buf, dx_buf, dw_buf = torch.empty_like(g), torch.empty_like(xd), torch.empty_like(wd)
    cin, cout, ext = shape["cin"], shape["cout"], (shape["side"],) * 3
    if transposed:
        op_passes = {"forward": lambda: cv._backward_data(xd, wd, y_buf, 1, cin, cout, ext, 2),
                     "backward_data": lambda: cv._forward(g, wd, dx_buf, 1, cin, cout, ext, 2),
                     "backward_weight": lambda: cv._backward_weight(g, xd, dw_buf, 1, cin, cout, ext, 2, 0)}
    else:
        op_passes = {"forward": lambda: cv._forward(xd, wd, y_buf, 1, cin, cout, ext, stride),
                     "backward_data": lambda: cv._backward_data(g, wd, dx_buf, 1, cin, cout, ext, stride),
                     "backward_weight": lambda: cv._backward_weight(xd, g, dw_buf, 1, cin, cout, ext, stride, 0)}

    def torch_backward(mask):
        return lambda: torch.ops.aten.convolution_backward(g, xd, wd, None, [stride] * 3, [1] * 3, [1] * 3, transposed, [op] * 3, 1, mask)

    def torch_forward():
        with torch.no_grad():
            return fwd_torch()

    torch_passes = {"forward": torch_forward, "backward_data": torch_backward([True, False, False]),
                    "backward_weight": torch_backward([False, True, False])}
    entry = dict(shape)
    entry["passes_us"] = {"op": {}, "torch": {}}
    for p in ("forward", "backward_data", "backward_weight"):
        r = tm.alternate({"op": op_passes[p], "torch": torch_passes[p]})
        entry["passes_us"]["op"][p], entry["passes_us"]["torch"][p] = r["op"], r["torch"]
        say(f"{name} {p}: op {r['op']['median_us']} us, torch {r['torch']['median_us']} us")
    # the results agree (the tests hold the bound; this guards the table against timing something else)
    want = torch.autograd.grad(fwd_torch(), [x, w], g)
    got = torch.autograd.grad(fwd_op(), [x, w], g)
    with torch.no_grad():
        entry["max_abs_difference"] = {"y": float((fwd_op() - fwd_torch()).abs().max()), "dx": float((got[0] - want[0]).abs().max()),
                                       "dw": float((got[1] - want[1]).abs().max())}
    entry["forward"] = tm.compare({"op": fwd_op, "torch": fwd_torch, "torch_benchmark": benchmark_on(torch, fwd_torch)})
    entry["forward_backward"] = tm.compare({"op": both(fwd_op), "torch": both(fwd_torch),
                                            "torch_benchmark": benchmark_on(torch, both(fwd_torch))}, peak=True)
    entry["op_wins"] = op_wins(entry)
    say(name + " " + json.dumps({p: {f: {k: entry[p][f][k]["median_us"] for k in entry[p][f]} for f in ("eager", "graph")}
                                 for p in ("forward", "forward_backward")}) + f" op_wins={entry['op_wins']}")
    return entry


def measure_stem(grid):
    import torch

    from manigaussian_amd import encoder as enc

    dev = torch.device("cuda:0")
    torch.backends.cudnn.benchmark = False
    tm = Timer(torch)
    torch.manual_seed(3)
    stem = enc.MultiLayer3DEncoderShallow().to(dev).train()
    gen = torch.Generator().manual_seed(8)
    x = torch.randn(1, 10, grid, grid, grid, generator=gen).to(dev)
    g = torch.randn(1, 64, grid, grid, grid, generator=gen).to(dev)
    params = list(stem.parameters())
    saved = (enc.FORCE, enc.CONV)

    def step(force, conv):
        def call():
            enc.FORCE, enc.CONV = force, conv
            try:
                out, _ = stem(x)
                return torch.autograd.grad(out, params, g)
            finally:
                enc.FORCE, enc.CONV = saved
        return call

    calls = {"rule": step(None, None), "conv_on": step(None, True), "conv_off": step(None, False),
             "parent_fused": step(True, False), "parent_torch": step(False, None)}
    entry = {"shape": [1, 10, grid, grid, grid], "forward_backward": tm.compare(calls, peak=True),
             "parent_commit_eager_median_ms": PARENT_MS}
    say("stem " + json.dumps({f: {k: v["median_us"] for k, v in entry["forward_backward"][f].items()} for f in ("eager", "graph")}))
    return entry


def child(args):
    import torch
    if not torch.cuda.is_available():
        print("bench_conv3d: no HIP device; nothing is timed on a CPU", file=sys.stderr)
        return 2
    if args.stem:
        part = measure_stem(args.grid)
    else:
        part = measure_site(next(s for s in SITES if s[0] == args.site), args.grid)
    with open(args.part, "w") as f:
        json.dump(part, f)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv3d_bench.json"))
    ap.add_argument("--no-stem", action="store_true", help="the ten sites only")
    ap.add_argument("--grid", type=int, default=100, help="the voxel grid's side (100: ManiGaussian's)")
    ap.add_argument("--site", help="(child) measure this site into --part")
    ap.add_argument("--stem", action="store_true", help="(child) measure the stem into --part")
    ap.add_argument("--part", help="(child) where the part goes")
    args = ap.parse_args()
    if args.part:
        return child(args)

    import torch

    from manigaussian_amd import _lib
    from manigaussian_amd import encoder as enc

    if not torch.cuda.is_available():
        print("bench_conv3d: no HIP device; nothing is timed on a CPU", file=sys.stderr)
        return 2
    result = {"device": torch.cuda.get_device_name(0), "build_id": _lib.build_id(), "runs": RUNS, "sample_ms": SAMPLE_MS,
              "grid": args.grid, "times_are": "measured, microseconds per call",
              "flop_and_bytes_are": "derived from the shapes", "sites": {}}
    tmp = tempfile.mkdtemp(prefix="bench_conv3d_")
    steps = [(s[0], ["--site", s[0]], SITE_TIMEOUT_S) for s in SITES] + ([] if args.no_stem else [("stem", ["--stem"], STEM_TIMEOUT_S)])
    for name, flags, limit in steps:
        part = os.path.join(tmp, name + ".json")
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--grid", str(args.grid), "--part", part] + flags
        say(f"{name} (limit {limit} s)")
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            say(f"{name}: exit {rc}; nothing more is started")
            return 1
        with open(part) as f:
            if name == "stem":
                result["stem"] = json.load(f)
            else:
                result["sites"][name] = json.load(f)

    result["routing_as_measured"] = {k: v["op_wins"] for k, v in result["sites"].items()}
    result["routing_in_the_package"] = {k: bool(enc.conv_site(v["cin"], v["cout"], v["voxels"], v["stride"], v["transposed"]))
                                        for k, v in result["sites"].items()}
    result["routed_sites"] = sorted(k for k, v in result["routing_in_the_package"].items() if v)
    print(json.dumps(result, sort_keys=True))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
