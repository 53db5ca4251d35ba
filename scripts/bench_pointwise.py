"""The voxel encoder stem's 1x1x1 conv_out (helpers/network_utils.py:248-306: nn.Conv3d(8, 64, 1, bias=True)), two ways, fp32, B = 1,
at ManiGaussian's 100^3 grid and at 50^3 and 25^3 (so that the routing rule has more than one point):
  op     manigaussian_amd.pointwise_conv3d (csrc/mgs_pointwise.hip)
  torch  F.conv3d on the same GPU, with torch.backends.cudnn.benchmark off (`torch`) and on (`torch_benchmark`)
Per shape, in ONE process, the sides alternating (scripts/bench_conv3d.py's protocol and its Timer):
  passes_us         the passes on their own, eager: forward, backward_data (dx alone) and backward_weight_bias (dw and db alone);
                    torch's through aten.convolution_backward with those outputs asked for, cudnn.benchmark off -- torch's conv_out
                    on its own, which DESIGN.md 7m had by subtraction only; `op_backward_fused_us`: the op's dx, dw and db together;
  forward, forward_backward   as in a training step (autograd recording; gradients towards x, weight and bias), each EAGER and
                    GRAPH-REPLAYED, three sides; peak_bytes: the peak allocation of one eager forward + backward;
  achieved          the op's algorithmic bytes (DERIVED from the shape) over its measured medians, beside the 8 TB/s roofline.
`op_wins`: in all four (pass, form) pairs the op's third quartile lies below the first quartile of torch's faster setting --
encoder.fused_site()'s criterion.  manigaussian_amd/encoder.py's pointwise_site() is set from these.
Then the whole stem, forward + backward at [1, 10, 100^3], in one process: POINTWISE following the rule (`rule`), forced on
(`pointwise_on`) and off (`pointwise_off`: the parent commit's behaviour, compared with the stem's figure in
profiles/conv3d_bench.json), and everything torch's (`all_torch`: encoder.FORCE = False); peak allocations beside them.
Then a side measurement, torch only: the Perceiver's patchify, nn.Conv3d(64, 64, 5, stride 5) on [1, 64, 100^3], which reads the same
volume next: forward and both gradients on their own.
FLOP and byte counts are DERIVED from the shapes, not measured; times are measured.
Every shape, the stem and patchify are timed in a child process of their own under `timeout`; the first child that fails ends the run.
Writes --out (default profiles/pointwise_bench.json) and prints it as one JSON line.  Needs a HIP device: a CPU has nothing to time."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_conv3d import RUNS, SAMPLE_MS, Timer, benchmark_on, op_wins  # noqa: E402

CIN, COUT = 8, 64
SHAPES = {"conv_out_100": 100, "conv_out_50": 50, "conv_out_25": 25}
SHAPE_TIMEOUT_S = int(os.environ.get("POINTWISE_SHAPE_TIMEOUT", "240"))
STEM_TIMEOUT_S = int(os.environ.get("POINTWISE_STEM_TIMEOUT", "420"))
ROOFLINE_BYTES_PER_S = 8.0e12
PASSES = ("forward", "backward_data", "backward_weight_bias")


def say(msg):
    print("bench_pointwise:", msg, file=sys.stderr, flush=True)


def shape_entry(side):
    n = side ** 3
    flop = 2 * CIN * COUT * n
    return {"cin": CIN, "cout": COUT, "side": side, "values_per_channel": n,
            "derived": {"flop_per_pass": flop, "flop_forward_backward": 3 * flop,
                        "bytes_forward": 4 * n * (CIN + COUT), "bytes_backward": 4 * n * (COUT + CIN + CIN),
                        "bytes_parameters": 4 * (COUT * CIN + COUT),
                        "note": "derived from the shapes, not measured: forward reads x and writes y; backward reads g and x and writes dx"}}


def measure_shape(side):
    import importlib

    import torch
    import torch.nn.functional as F

    from manigaussian_amd import _lib, _ops
    pw = importlib.import_module("manigaussian_amd.pointwise")
    dev = torch.device("cuda:0")
    torch.backends.cudnn.benchmark = False
    tm = Timer(torch)
    entry = shape_entry(side)
    n = side ** 3
    gen = torch.Generator().manual_seed(9)
    x = torch.randn(1, CIN, side, side, side, generator=gen).to(dev).requires_grad_(True)
    g = torch.randn(1, COUT, side, side, side, generator=gen).to(dev)
    w = (torch.randn(COUT, CIN, 1, 1, 1, generator=gen) * CIN ** -0.5).to(dev).requires_grad_(True)
    b = torch.randn(COUT, generator=gen).to(dev).requires_grad_(True)

    def fwd_torch():
        return F.conv3d(x, w, b)

    def fwd_op():
        return pw.pointwise_conv3d(x, w, b)

    def both(fwd):
        return lambda: torch.autograd.grad(fwd(), [x, w, b], g)

    xd, wd, bd = x.detach(), w.detach(), b.detach()
    y_buf, dx_buf, dw_buf, db_buf = torch.empty_like(g), torch.empty_like(xd), torch.empty_like(wd), torch.empty_like(bd)
    ws = _ops.workspace(dev, _lib.lib().mgs_pointwise_workspace_bytes(1, CIN, COUT, n))

    def op_backward(dx, dw, db):
        return lambda: _ops.call("mgs_pointwise_backward", dev, 1, CIN, COUT, n, xd.data_ptr(), g.data_ptr(), wd.data_ptr(), _ops.ptr(dx),
                                 _ops.ptr(dw), _ops.ptr(db), ws.data_ptr(), ws.numel(), 0)

    op_passes = {"forward": lambda: _ops.call("mgs_pointwise_forward", dev, 1, CIN, COUT, n, xd.data_ptr(), wd.data_ptr(), bd.data_ptr(),
                                              y_buf.data_ptr()),
                 "backward_data": op_backward(dx_buf, None, None), "backward_weight_bias": op_backward(None, dw_buf, db_buf)}

    def torch_backward(mask):
        return lambda: torch.ops.aten.convolution_backward(g, xd, wd, [COUT], [1] * 3, [0] * 3, [1] * 3, False, [0] * 3, 1, mask)

    def torch_forward():
        with torch.no_grad():
            return fwd_torch()

    torch_passes = {"forward": torch_forward, "backward_data": torch_backward([True, False, False]),
                    "backward_weight_bias": torch_backward([False, True, True])}
    entry["passes_us"] = {"op": {}, "torch": {}}
    for p in PASSES:
        r = tm.alternate({"op": op_passes[p], "torch": torch_passes[p]})
        entry["passes_us"]["op"][p], entry["passes_us"]["torch"][p] = r["op"], r["torch"]
        say(f"{side}^3 {p}: op {r['op']['median_us']} us, torch {r['torch']['median_us']} us")
    entry["op_backward_fused_us"] = tm.alternate({"op": op_backward(dx_buf, dw_buf, db_buf)})["op"]
    # the results agree (the tests hold the bound; this guards the table against timing something else)
    want = torch.autograd.grad(fwd_torch(), [x, w, b], g)
    got = torch.autograd.grad(fwd_op(), [x, w, b], g)
    with torch.no_grad():
        entry["max_abs_difference"] = {"y": float((fwd_op() - fwd_torch()).abs().max()), "dx": float((got[0] - want[0]).abs().max()),
                                       "dw": float((got[1] - want[1]).abs().max()), "db": float((got[2] - want[2]).abs().max())}
    entry["forward"] = tm.compare({"op": fwd_op, "torch": fwd_torch, "torch_benchmark": benchmark_on(torch, fwd_torch)})
    entry["forward_backward"] = tm.compare({"op": both(fwd_op), "torch": both(fwd_torch),
                                            "torch_benchmark": benchmark_on(torch, both(fwd_torch))}, peak=True)
    entry["op_wins"] = op_wins(entry)
    d = entry["derived"]
    f_us, b_us = entry["passes_us"]["op"]["forward"]["median_us"], entry["op_backward_fused_us"]["median_us"]
    entry["achieved"] = {"forward_bytes_per_s": round(d["bytes_forward"] / (f_us * 1e-6)),
                         "backward_fused_bytes_per_s": round(d["bytes_backward"] / (b_us * 1e-6)),
                         "roofline_bytes_per_s": ROOFLINE_BYTES_PER_S,
                         "note": "derived bytes over the measured eager medians of the passes on their own"}
    say(f"{side}^3 " + json.dumps({p: {f: {k: entry[p][f][k]["median_us"] for k in entry[p][f]} for f in ("eager", "graph")}
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
    saved = (enc.FORCE, enc.POINTWISE)

    def step(force, pointwise):
        def call():
            enc.FORCE, enc.POINTWISE = force, pointwise
            try:
                out, _ = stem(x)
                return torch.autograd.grad(out, params, g)
            finally:
                enc.FORCE, enc.POINTWISE = saved
        return call

    calls = {"rule": step(None, None), "pointwise_on": step(None, True), "pointwise_off": step(None, False), "all_torch": step(False, None)}
    entry = {"shape": [1, 10, grid, grid, grid], "forward_backward": tm.compare(calls, peak=True)}
    with open(os.path.join(ROOT, "profiles", "conv3d_bench.json")) as f:
        parent_us = json.load(f)["stem"]["forward_backward"]["eager"]["rule"]["median_us"]
    off = entry["forward_backward"]["eager"]["pointwise_off"]
    entry["parent_commit"] = {"eager_median_us_in_conv3d_bench": parent_us, "pointwise_off_eager_median_us": off["median_us"],
                              "ratio": round(off["median_us"] / parent_us, 4),
                              "agree": bool(abs(off["median_us"] / parent_us - 1.0) <= 0.05),
                              "note": "pointwise_off is the parent commit's behaviour; agree: within 5 % of the figure measured there"}
    say("stem " + json.dumps({f: {k: v["median_us"] for k, v in entry["forward_backward"][f].items()} for f in ("eager", "graph")}))
    return entry


def measure_patchify(grid):
    """torch only: the Perceiver's patchify reads conv_out's output next."""
    import torch

    dev = torch.device("cuda:0")
    torch.backends.cudnn.benchmark = False
    tm = Timer(torch)
    torch.manual_seed(4)
    conv = torch.nn.Conv3d(64, 64, 5, stride=5).to(dev)
    gen = torch.Generator().manual_seed(10)
    x = torch.randn(1, 64, grid, grid, grid, generator=gen).to(dev)
    wd, bd = conv.weight.detach(), conv.bias.detach()
    with torch.no_grad():
        y = conv(x)
    g = torch.randn(*y.shape, generator=gen).to(dev)

    def forward():
        with torch.no_grad():
            return conv(x)

    def backward(mask):
        return lambda: torch.ops.aten.convolution_backward(g, x, wd, [64], [5] * 3, [0] * 3, [1] * 3, False, [0] * 3, 1, mask)

    calls = {"forward": forward, "backward_data": backward([True, False, False]), "backward_weight_bias": backward([False, True, True])}
    out = y.numel()
    entry = {"module": "nn.Conv3d(64, 64, 5, stride=5)", "x": list(x.shape), "y": list(y.shape), "side": "torch, cudnn.benchmark off",
             "passes_us": {p: tm.alternate({"torch": c})["torch"] for p, c in calls.items()},
             "derived": {"flop_per_pass": 2 * 64 * 64 * 125 * out, "bytes_x": 4 * x.numel(), "bytes_y": 4 * out,
                         "bytes_weight": 4 * wd.numel(), "note": "derived from the shapes, not measured"}}
    say("patchify " + json.dumps({p: v["median_us"] for p, v in entry["passes_us"].items()}))
    return entry


def child(args):
    import torch
    if not torch.cuda.is_available():
        print("bench_pointwise: no HIP device; nothing is timed on a CPU", file=sys.stderr)
        return 2
    if args.stem:
        part = measure_stem(args.grid)
    elif args.patchify:
        part = measure_patchify(args.grid)
    else:
        part = measure_shape(SHAPES[args.shape])
    with open(args.part, "w") as f:
        json.dump(part, f)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pointwise_bench.json"))
    ap.add_argument("--grid", type=int, default=100, help="the voxel grid's side for the stem and patchify (100: ManiGaussian's)")
    ap.add_argument("--shape", help="(child) measure this shape into --part")
    ap.add_argument("--stem", action="store_true", help="(child) measure the stem into --part")
    ap.add_argument("--patchify", action="store_true", help="(child) measure torch's patchify into --part")
    ap.add_argument("--part", help="(child) where the part goes")
    args = ap.parse_args()
    if args.part:
        return child(args)

    import torch

    from manigaussian_amd import _lib
    from manigaussian_amd import encoder as enc

    if not torch.cuda.is_available():
        print("bench_pointwise: no HIP device; nothing is timed on a CPU", file=sys.stderr)
        return 2
    result = {"device": torch.cuda.get_device_name(0), "build_id": _lib.build_id(), "runs": RUNS, "sample_ms": SAMPLE_MS,
              "grid": args.grid, "times_are": "measured, microseconds per call",
              "flop_and_bytes_are": "derived from the shapes", "shapes": {}}
    tmp = tempfile.mkdtemp(prefix="bench_pointwise_")
    steps = [(name, ["--shape", name], SHAPE_TIMEOUT_S) for name in SHAPES]
    steps += [("stem", ["--stem"], STEM_TIMEOUT_S), ("patchify", ["--patchify"], SHAPE_TIMEOUT_S)]
    for name, flags, limit in steps:
        part = os.path.join(tmp, name + ".json")
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--grid", str(args.grid), "--part", part] + flags
        say(f"{name} (limit {limit} s)")
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            say(f"{name}: exit {rc}; nothing more is started")
            return 1
        with open(part) as f:
            if name in SHAPES:
                result["shapes"][name] = json.load(f)
            else:
                result[name] = json.load(f)

    result["routing_as_measured"] = {k: v["op_wins"] for k, v in result["shapes"].items()}
    result["routing_in_the_package"] = {k: bool(enc.pointwise_site(v["cin"], v["cout"], v["values_per_channel"]))
                                        for k, v in result["shapes"].items()}
    result["routed_shapes"] = sorted(k for k, v in result["routing_in_the_package"].items() if v)
    print(json.dumps(result, sort_keys=True))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
