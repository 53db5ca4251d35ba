"""The voxel encoder stem's 1x1x1 conv_out at final_dim = 128 (conf/method/ManiGaussian_BC.yaml:35: nn.Conv3d(8, 128, 1, bias=True)),
four ways, fp32, B = 1, at ManiGaussian's 100^3 grid and at 50^3 and 25^3 (so that the routing rule has more than one point):
  op      manigaussian_amd.wide_pointwise_conv3d (csrc/mgs_pointwise.hip: mgs_pointwise_wide_*)
  torch   F.conv3d on the same GPU, with torch.backends.cudnn.benchmark off (`torch`) and on (`torch_benchmark`)
  halves  what a caller could do without the wide op: two mgs_pointwise_* calls on the weight's halves (64 output channels each),
          writing into the two halves of ONE y (B = 1 makes them contiguous) and reading the two halves of g; the two dx are added by
          torch.  An autograd function of this script over the library's narrow entry points; recorded beside the others, NOT part of
          `op_wins`.
Per shape, in ONE process, the sides alternating (scripts/bench_pointwise.py's protocol, scripts/bench_conv3d.py's Timer):
  passes_us         the passes on their own, eager: forward, backward_data (dx alone) and backward_weight_bias (dw and db alone);
                    torch's through aten.convolution_backward with those outputs asked for, cudnn.benchmark off;
                    `op_backward_fused_us` / `halves_backward_fused_us`: dx, dw and db together;
  forward, forward_backward   as in a training step (autograd recording; gradients towards x, weight and bias), each EAGER and
                    GRAPH-REPLAYED, four sides; peak_bytes: the peak allocation of one eager forward + backward;
  achieved          the op's algorithmic bytes (DERIVED from the shape and the kernel's passes) over its measured medians, beside the
                    8 TB/s roofline: a record, not a gate.
`op_wins`: in all four (pass, form) pairs the op's third quartile lies below the first quartile of torch's faster setting --
encoder.fused_site()'s criterion.  manigaussian_amd/encoder.py's wide_pointwise_site() is set from these.
Then the whole stem with out_channels = 128, forward + backward at [1, 10, 100^3], in one process: following the rule (`rule`), the wide
route forced on (`wide_on`) and off (`wide_off`: POINTWISE = False, which at 128 output channels is the parent commit's behaviour --
conv_out on torch, every other site by its rule -- and what every speed-up is quoted against), and everything torch's (`all_torch`:
encoder.FORCE = False); peak allocations beside them.
FLOP and byte counts are DERIVED from the shapes, not measured; times are measured.
Every shape and the stem are timed in a child process of their own under `timeout`; the first child that fails ends the run.
Writes --out (default profiles/wide_pointwise_bench.json) and prints it as one JSON line.  Needs a HIP device."""
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

CIN, COUT, HALF = 8, 128, 64
SHAPES = {"conv_out128_100": 100, "conv_out128_50": 50, "conv_out128_25": 25}
SHAPE_TIMEOUT_S = int(os.environ.get("WIDE_POINTWISE_SHAPE_TIMEOUT", "300"))
STEM_TIMEOUT_S = int(os.environ.get("WIDE_POINTWISE_STEM_TIMEOUT", "420"))
ROOFLINE_BYTES_PER_S = 8.0e12
PASSES = ("forward", "backward_data", "backward_weight_bias")
SIDES = ("op", "torch", "halves")


def say(msg):
    print("bench_wide_pointwise:", msg, file=sys.stderr, flush=True)


def shape_entry(side):
    n = side ** 3
    flop = 2 * CIN * COUT * n
    blocks = (COUT + 63) // 64
    return {"cin": CIN, "cout": COUT, "side": side, "values_per_channel": n,
            "derived": {"flop_per_pass": flop, "flop_forward_backward": 3 * flop,
                        "bytes_forward": 4 * n * (CIN + COUT),
                        "bytes_backward": 4 * n * (COUT + blocks * CIN + blocks * CIN + (blocks - 1) * CIN),
                        "bytes_backward_ideal": 4 * n * (COUT + CIN + CIN),
                        "bytes_parameters": 4 * (COUT * CIN + COUT),
                        "note": "derived from the shapes, not measured: forward reads x and writes y; the fused backward reads g once, "
                                "x once per block of 64 output channels, writes dx once per block and reads it back once per block "
                                "after the first; ideal: g, x and dx once"}}


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
    ws = _ops.workspace(dev, _lib.lib().mgs_pointwise_wide_workspace_bytes(1, CIN, COUT, n))   # (no smaller than the narrow op's)
    assert ws.numel() >= _lib.lib().mgs_pointwise_workspace_bytes(1, CIN, HALF, n)

    # the two halves through the narrow entry points, on pointers into the whole tensors (B = 1: a half of y or g is contiguous)
    def halves_forward(xt, wt, bt, yt):
        for h in (0, 1):
            _ops.call("mgs_pointwise_forward", dev, 1, CIN, HALF, n, xt.data_ptr(), wt[h * HALF:].data_ptr(), bt[h * HALF:].data_ptr(),
                      yt[:, h * HALF:].data_ptr())

    def halves_backward(xt, gt, wt, dx, dw, db, dx_second):
        for h in (0, 1):
            part = None if dx is None else (dx, dx_second)[h]
            _ops.call("mgs_pointwise_backward", dev, 1, CIN, HALF, n, xt.data_ptr(), gt[:, h * HALF:].data_ptr(),
                      wt[h * HALF:].data_ptr(), _ops.ptr(part), _ops.ptr(None if dw is None else dw[h * HALF:]),
                      _ops.ptr(None if db is None else db[h * HALF:]), ws.data_ptr(), ws.numel(), 0)
        if dx is not None:
            dx.add_(dx_second)

    class Halves(torch.autograd.Function):
        @staticmethod
        def forward(ctx, xt, wt, bt):
            y = torch.empty_like(g)
            halves_forward(xt, wt, bt, y)
            ctx.save_for_backward(xt, wt)
            return y

        @staticmethod
        def backward(ctx, gt):
            xt, wt = ctx.saved_tensors
            gt = gt.contiguous()
            dx, dw, db = torch.empty_like(xt), torch.empty_like(wt), torch.empty(COUT, dtype=torch.float32, device=dev)
            halves_backward(xt, gt, wt, dx, dw, db, torch.empty_like(xt))
            return dx, dw, db

    def fwd_torch():
        return F.conv3d(x, w, b)

    def fwd_op():
        return pw.wide_pointwise_conv3d(x, w, b)

    def fwd_halves():
        return Halves.apply(x, w, b)

    def both(fwd):
        return lambda: torch.autograd.grad(fwd(), [x, w, b], g)

    xd, wd, bd = x.detach(), w.detach(), b.detach()
    y_buf, dx_buf, dx2_buf = torch.empty_like(g), torch.empty_like(xd), torch.empty_like(xd)
    dw_buf, db_buf = torch.empty_like(wd), torch.empty_like(bd)

    def op_backward(dx, dw, db):
        return lambda: _ops.call("mgs_pointwise_wide_backward", dev, 1, CIN, COUT, n, xd.data_ptr(), g.data_ptr(), wd.data_ptr(),
                                 _ops.ptr(dx), _ops.ptr(dw), _ops.ptr(db), ws.data_ptr(), ws.numel(), 0)

    def torch_backward(mask):
        return lambda: torch.ops.aten.convolution_backward(g, xd, wd, [COUT], [1] * 3, [0] * 3, [1] * 3, False, [0] * 3, 1, mask)

    def torch_forward():
        with torch.no_grad():
            return fwd_torch()

    passes = {
        "op": {"forward": lambda: _ops.call("mgs_pointwise_wide_forward", dev, 1, CIN, COUT, n, xd.data_ptr(), wd.data_ptr(),
                                            bd.data_ptr(), y_buf.data_ptr()),
               "backward_data": op_backward(dx_buf, None, None), "backward_weight_bias": op_backward(None, dw_buf, db_buf)},
        "torch": {"forward": torch_forward, "backward_data": torch_backward([True, False, False]),
                  "backward_weight_bias": torch_backward([False, True, True])},
        "halves": {"forward": lambda: halves_forward(xd, wd, bd, y_buf),
                   "backward_data": lambda: halves_backward(xd, g, wd, dx_buf, None, None, dx2_buf),
                   "backward_weight_bias": lambda: halves_backward(xd, g, wd, None, dw_buf, db_buf, None)},
    }
    entry["passes_us"] = {s: {} for s in SIDES}
    for p in PASSES:
        r = tm.alternate({s: passes[s][p] for s in SIDES})
        for s in SIDES:
            entry["passes_us"][s][p] = r[s]
        say(f"{side}^3 {p}: " + ", ".join(f"{s} {r[s]['median_us']} us" for s in SIDES))
    fused = tm.alternate({"op": op_backward(dx_buf, dw_buf, db_buf),
                          "halves": lambda: halves_backward(xd, g, wd, dx_buf, dw_buf, db_buf, dx2_buf)})
    entry["op_backward_fused_us"], entry["halves_backward_fused_us"] = fused["op"], fused["halves"]
    # the results agree (the tests hold the bound; this guards the table against timing something else)
    want = torch.autograd.grad(fwd_torch(), [x, w, b], g)
    with torch.no_grad():
        y_want = fwd_torch()
        entry["max_abs_difference"] = {}
        for name, fwd in (("op", fwd_op), ("halves", fwd_halves)):
            with torch.enable_grad():
                got = torch.autograd.grad(fwd(), [x, w, b], g)
            entry["max_abs_difference"][name] = {"y": float((fwd() - y_want).abs().max()), "dx": float((got[0] - want[0]).abs().max()),
                                                 "dw": float((got[1] - want[1]).abs().max()), "db": float((got[2] - want[2]).abs().max())}
    entry["forward"] = tm.compare({"op": fwd_op, "torch": fwd_torch, "torch_benchmark": benchmark_on(torch, fwd_torch),
                                   "halves": fwd_halves})
    entry["forward_backward"] = tm.compare({"op": both(fwd_op), "torch": both(fwd_torch),
                                            "torch_benchmark": benchmark_on(torch, both(fwd_torch)), "halves": both(fwd_halves)},
                                           peak=True)
    entry["op_wins"] = op_wins(entry)
    fb = entry["forward_backward"]
    entry["op_beats_halves_forward_backward"] = {f: bool(fb[f]["op"]["q3_us"] < fb[f]["halves"]["q1_us"]) for f in ("eager", "graph")}
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
    stem = enc.MultiLayer3DEncoderShallow(out_channels=COUT).to(dev).train()
    gen = torch.Generator().manual_seed(8)
    x = torch.randn(1, 10, grid, grid, grid, generator=gen).to(dev)
    g = torch.randn(1, COUT, grid, grid, grid, generator=gen).to(dev)
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

    calls = {"rule": step(None, None), "wide_on": step(None, True), "wide_off": step(None, False), "all_torch": step(False, None)}
    entry = {"shape": [1, 10, grid, grid, grid], "out_channels": COUT, "forward_backward": tm.compare(calls, peak=True),
             "note": "wide_off (POINTWISE = False; the narrow route does not take 128 output channels) is the parent commit's behaviour"}
    say("stem " + json.dumps({f: {k: v["median_us"] for k, v in entry["forward_backward"][f].items()} for f in ("eager", "graph")}))
    return entry


def child(args):
    import torch
    if not torch.cuda.is_available():
        print("bench_wide_pointwise: no HIP device; nothing is timed on a CPU", file=sys.stderr)
        return 2
    part = measure_stem(args.grid) if args.stem else measure_shape(SHAPES[args.shape])
    with open(args.part, "w") as f:
        json.dump(part, f)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_pointwise_bench.json"))
    ap.add_argument("--grid", type=int, default=100, help="the voxel grid's side for the stem (100: ManiGaussian's)")
    ap.add_argument("--shape", help="(child) measure this shape into --part")
    ap.add_argument("--stem", action="store_true", help="(child) measure the stem into --part")
    ap.add_argument("--part", help="(child) where the part goes")
    args = ap.parse_args()
    if args.part:
        return child(args)

    import torch

    from manigaussian_amd import _lib
    from manigaussian_amd import encoder as enc

    if not torch.cuda.is_available():
        print("bench_wide_pointwise: no HIP device; nothing is timed on a CPU", file=sys.stderr)
        return 2
    result = {"device": torch.cuda.get_device_name(0), "build_id": _lib.build_id(), "runs": RUNS, "sample_ms": SAMPLE_MS,
              "grid": args.grid, "times_are": "measured, microseconds per call",
              "flop_and_bytes_are": "derived from the shapes", "shapes": {}}
    tmp = tempfile.mkdtemp(prefix="bench_wide_pointwise_")
    steps = [(name, ["--shape", name], SHAPE_TIMEOUT_S) for name in SHAPES] + [("stem", ["--stem"], STEM_TIMEOUT_S)]
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
    result["routing_in_the_package"] = {k: bool(enc.wide_pointwise_site(v["cin"], v["cout"], v["values_per_channel"]))
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
