"""The Perceiver decoder's trans_decoder (agents/manigaussian_bc/perceiver_lang_io.py:322: Conv3DBlock(128, 1, 3) = nn.Conv3d(128, 1, 3,
padding=1, padding_mode='replicate') with bias), fp32, B = 1, at ManiGaussian's 100^3 grid and at 50^3 and 25^3 (so that the routing
rule has more than one point), three ways:
  op      manigaussian_amd.narrow_conv3d (csrc/mgs_narrow.hip): the pad folded into the addressing
  torch   the parent commit's path, volume.resample_pad(x, 1, 1) + F.conv3d(padding=0), with torch.backends.cudnn.benchmark off
          (`torch`) and on (`torch_benchmark`)
  module  for information: plain nn.Conv3d(padding_mode='replicate'), which pads with F.pad
Per shape, in ONE process, the sides alternating (scripts/bench_conv3d.py's protocol and its Timer):
  passes_us         the passes on their own, eager: forward, backward_data (dx alone) and backward_weight_bias (dw and db alone);
                    torch's forward is pad + convolution; its backward passes are aten.convolution_backward on the padded volume
                    with those outputs asked for, backward_data followed by resample_pad's own backward, cudnn.benchmark off;
                    `op_backward_all_us`: the op's dx, dw and db in one call;
  forward, forward_backward   as in a training step (autograd recording; gradients towards x, weight and bias), each EAGER and
                    GRAPH-REPLAYED; peak_bytes: the peak allocation of one eager forward + backward;
  achieved          the op's algorithmic FLOP and bytes (DERIVED from the shape) over its measured medians, beside the derived floors.
`op_wins`: in all four (pass, form) pairs the op's third quartile lies below the first quartile of torch's faster setting --
encoder.fused_site()'s criterion.  manigaussian_amd/volume.py's narrow_site() is set from these.
FLOP and byte counts are DERIVED from the shapes, not measured; times are measured.
Every shape is timed in a child process of its own under `timeout`; the first child that fails ends the run.
Writes --out (default profiles/narrow_conv_bench.json) and prints it as one JSON line.  Needs a HIP device: a CPU has nothing to time.
--refresh-routing rewrites only `routing_in_the_package` and `routed_shapes` of an existing --out from the package's rule as it
stands (no device needed): they state what the package does with the measured shapes, and the rule is set after the measurement."""
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

CIN, COUT = 128, 1
SHAPES = {"trans_decoder_100": 100, "trans_decoder_50": 50, "trans_decoder_25": 25}
SHAPE_TIMEOUT_S = int(os.environ.get("NARROW_SHAPE_TIMEOUT", "420"))
ROOFLINE_BYTES_PER_S = 8.0e12
PACKED_FP32_FLOP_PER_S = 157.3e12
PASSES = ("forward", "backward_data", "backward_weight_bias")


def say(msg):
    print("bench_narrow:", msg, file=sys.stderr, flush=True)


def shape_entry(side):
    n = side ** 3
    flop = 2 * 27 * CIN * COUT * n
    return {"cin": CIN, "cout": COUT, "side": side, "voxels": n,
            "derived": {"flop_per_pass": flop, "flop_forward_backward": 3 * flop,
                        "bytes_forward": 4 * n * (CIN + COUT), "bytes_backward": 4 * n * (CIN + CIN + 2 * COUT),
                        "bytes_parameters": 4 * (27 * COUT * CIN + COUT), "bytes_padded_copy": 4 * CIN * (side + 2) ** 3,
                        "note": "derived from the shapes, not measured: forward reads x and writes y; backward reads x once for dw, "
                                "writes dx and reads g once per kernel; the padded copy is what the parent's path writes and reads back"}}


def measure_shape(side):
    import importlib

    import torch
    import torch.nn.functional as F

    from manigaussian_amd import _lib, _ops
    from manigaussian_amd import volume as vol
    nw = importlib.import_module("manigaussian_amd.narrow")
    dev = torch.device("cuda:0")
    torch.backends.cudnn.benchmark = False
    tm = Timer(torch)
    entry = shape_entry(side)
    ext = (side, side, side)
    gen = torch.Generator().manual_seed(9)
    x = torch.randn(1, CIN, *ext, generator=gen).to(dev).requires_grad_(True)
    g = torch.randn(1, COUT, *ext, generator=gen).to(dev)
    w = (torch.randn(COUT, CIN, 3, 3, 3, generator=gen) * (27 * CIN) ** -0.5).to(dev).requires_grad_(True)
    b = torch.randn(COUT, generator=gen).to(dev).requires_grad_(True)
    module = torch.nn.Conv3d(CIN, COUT, 3, padding=1, padding_mode="replicate").to(dev)
    with torch.no_grad():
        module.weight.copy_(w)
        module.bias.copy_(b)

    def fwd_torch():   # the parent commit's Conv3DBlock.forward
        return F.conv3d(vol.resample_pad(x, 1, 1), w, b)

    def fwd_op():
        return nw.narrow_conv3d(x, w, b)

    def both(fwd):
        return lambda: torch.autograd.grad(fwd(), [x, w, b], g)

    def both_module():
        return torch.autograd.grad(module(x), [x, module.weight, module.bias], g)

    xd, wd, bd = x.detach(), w.detach(), b.detach()
    y_buf, dx_buf, dw_buf, db_buf = torch.empty_like(g), torch.empty_like(xd), torch.empty_like(wd), torch.empty_like(bd)
    ws = _ops.workspace(dev, _lib.lib().mgs_narrow_conv3d_workspace_bytes(1, CIN, COUT, *ext))

    def op_backward(dx, dw, db):
        return lambda: _ops.call("mgs_narrow_conv3d_backward", dev, 1, CIN, COUT, *ext, 0, xd.data_ptr(), g.data_ptr(), wd.data_ptr(),
                                 _ops.ptr(dx), _ops.ptr(dw), _ops.ptr(db), ws.data_ptr(), ws.numel(), 0)

    op_passes = {"forward": lambda: _ops.call("mgs_narrow_conv3d_forward", dev, 1, CIN, COUT, *ext, 0, xd.data_ptr(), wd.data_ptr(),
                                              bd.data_ptr(), y_buf.data_ptr()),
                 "backward_data": op_backward(dx_buf, None, None), "backward_weight_bias": op_backward(None, dw_buf, db_buf)}

    with torch.no_grad():
        padded = vol.resample_pad(xd, 1, 1)

    def conv_backward(mask):
        return torch.ops.aten.convolution_backward(g, padded, wd, [COUT], [1] * 3, [0] * 3, [1] * 3, False, [0] * 3, 1, mask)

    pad_probe = vol.resample_pad(x, 1, 1)   # (its autograd node turns a padded gradient into x's)

    def torch_forward():
        with torch.no_grad():
            return F.conv3d(vol.resample_pad(xd, 1, 1), wd, bd)

    def torch_backward_data():
        gp = conv_backward([True, False, False])[0]
        return torch.autograd.grad(pad_probe, x, gp, retain_graph=True)

    torch_passes = {"forward": torch_forward, "backward_data": torch_backward_data,
                    "backward_weight_bias": lambda: conv_backward([False, True, True])}
    entry["passes_us"] = {"op": {}, "torch": {}}
    for p in PASSES:
        r = tm.alternate({"op": op_passes[p], "torch": torch_passes[p]})
        entry["passes_us"]["op"][p], entry["passes_us"]["torch"][p] = r["op"], r["torch"]
        say(f"{side}^3 {p}: op {r['op']['median_us']} us, torch {r['torch']['median_us']} us")
    entry["op_backward_all_us"] = tm.alternate({"op": op_backward(dx_buf, dw_buf, db_buf)})["op"]
    del pad_probe, padded
    # the results agree (the tests hold the bound; this guards the table against timing something else)
    want = torch.autograd.grad(fwd_torch(), [x, w, b], g)
    got = torch.autograd.grad(fwd_op(), [x, w, b], g)
    with torch.no_grad():
        entry["max_abs_difference"] = {"y": float((fwd_op() - fwd_torch()).abs().max()), "dx": float((got[0] - want[0]).abs().max()),
                                       "dw": float((got[1] - want[1]).abs().max()), "db": float((got[2] - want[2]).abs().max())}
    del want, got
    entry["forward"] = tm.compare({"op": fwd_op, "torch": fwd_torch, "torch_benchmark": benchmark_on(torch, fwd_torch),
                                   "module": lambda: module(x)})
    entry["forward_backward"] = tm.compare({"op": both(fwd_op), "torch": both(fwd_torch),
                                            "torch_benchmark": benchmark_on(torch, both(fwd_torch)), "module": both_module}, peak=True)
    entry["op_wins"] = op_wins(entry)
    d = entry["derived"]
    po = entry["passes_us"]["op"]
    entry["achieved"] = {
        "forward_bytes_per_s": round(d["bytes_forward"] / (po["forward"]["median_us"] * 1e-6)),
        "forward_flop_per_s": round(d["flop_per_pass"] / (po["forward"]["median_us"] * 1e-6)),
        "backward_data_flop_per_s": round(d["flop_per_pass"] / (po["backward_data"]["median_us"] * 1e-6)),
        "backward_weight_bias_flop_per_s": round(d["flop_per_pass"] / (po["backward_weight_bias"]["median_us"] * 1e-6)),
        "backward_all_bytes_per_s": round(d["bytes_backward"] / (entry["op_backward_all_us"]["median_us"] * 1e-6)),
        "roofline_bytes_per_s": ROOFLINE_BYTES_PER_S, "packed_fp32_flop_per_s": PACKED_FP32_FLOP_PER_S,
        "note": "derived FLOP and bytes over the measured eager medians of the passes on their own; the kernels issue unpacked "
                "fused multiply-adds, whose peak is half the packed one"}
    say(f"{side}^3 " + json.dumps({p: {f: {k: entry[p][f][k]["median_us"] for k in entry[p][f]} for f in ("eager", "graph")}
                                  for p in ("forward", "forward_backward")}) + f" op_wins={entry['op_wins']}")
    return entry


def child(args):
    import torch
    if not torch.cuda.is_available():
        print("bench_narrow: no HIP device; nothing is timed on a CPU", file=sys.stderr)
        return 2
    part = measure_shape(SHAPES[args.shape])
    with open(args.part, "w") as f:
        json.dump(part, f)
    return 0


def routing(result):
    from manigaussian_amd import volume as vol
    result["routing_in_the_package"] = {k: bool(vol.narrow_site(v["cin"], v["cout"], v["voxels"])) for k, v in result["shapes"].items()}
    result["routed_shapes"] = sorted(k for k, v in result["routing_in_the_package"].items() if v)


def write(result, out):
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "narrow_conv_bench.json"))
    ap.add_argument("--refresh-routing", action="store_true", help="rewrite the routing fields of --out from the package's rule; no device")
    ap.add_argument("--shape", help="(child) measure this shape into --part")
    ap.add_argument("--part", help="(child) where the part goes")
    args = ap.parse_args()
    if args.part:
        return child(args)
    if args.refresh_routing:
        with open(args.out) as f:
            result = json.load(f)
        routing(result)
        write(result, args.out)
        return 0

    import torch

    from manigaussian_amd import _lib

    if not torch.cuda.is_available():
        print("bench_narrow: no HIP device; nothing is timed on a CPU", file=sys.stderr)
        return 2
    result = {"device": torch.cuda.get_device_name(0), "build_id": _lib.build_id(), "runs": RUNS, "sample_ms": SAMPLE_MS,
              "times_are": "measured, microseconds per call", "flop_and_bytes_are": "derived from the shapes", "shapes": {}}
    tmp = tempfile.mkdtemp(prefix="bench_narrow_")
    steps = [(name, ["--shape", name], SHAPE_TIMEOUT_S) for name in SHAPES]
    for name, flags, limit in steps:
        part = os.path.join(tmp, name + ".json")
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--part", part] + flags
        say(f"{name} (limit {limit} s)")
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            say(f"{name}: exit {rc}; nothing more is started")
            return 1
        with open(part) as f:
            result["shapes"][name] = json.load(f)

    result["routing_as_measured"] = {k: v["op_wins"] for k, v in result["shapes"].items()}
    routing(result)
    print(json.dumps(result, sort_keys=True))
    write(result, args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
