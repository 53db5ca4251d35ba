"""The Perceiver decoder's dense convolutions (agents/manigaussian_bc/perceiver_lang_io.py: up0 = Conv3DUpsampleBlock(256, 128, 5) and
final = Conv3DBlock(256, 128, 3), both lrelu), fp32, B = 1, on the volume resample_pad already padded, at ManiGaussian's sizes and at
half of them (so that the routing rule has more than one point per site).  A shape is named by the unpadded side:
  up0_first_20                 256 -> 128, 5x5x5, [1,256,24^3]  -> [1,128,20^3]
  up0_last_100, up0_last_50    128 -> 128, 5x5x5, [1,128,104^3] -> [1,128,100^3]
  final_100, final_50          256 -> 128, 3x3x3, [1,256,102^3] -> [1,128,100^3]
two ways:
  op      manigaussian_amd.dense_conv3d (csrc/mgs_dense.hip): convolution, bias and leaky ReLU on the exact-f32 MFMA
  torch   F.leaky_relu(F.conv3d(x, w, b), 0.02), MIOpen's convolution, with torch.backends.cudnn.benchmark off (`torch`) and on
          (`torch_benchmark`)
Per shape, in ONE process, the sides alternating (scripts/bench_conv3d.py's protocol and its Timer):
  passes_us         the passes on their own, eager: forward, backward_data (dx alone) and backward_weight_bias (dw and db alone);
                    torch's backward passes are aten.convolution_backward with those outputs asked for, cudnn.benchmark off
  forward, forward_backward   as in a training step (autograd recording; gradients towards x, weight and bias), each EAGER and
                    GRAPH-REPLAYED; peak_bytes: the peak allocation of one eager forward + backward
  achieved_tflops   the DERIVED FLOP of a pass (2 Cin Cout k^3 output voxels) over the op's measured median, beside the 157.3
                    TFLOP/s fp32 matrix peak; `torch`: the same over torch's medians
`torch_benchmark` runs in children of its own AFTER everything else, smallest shape first, each under a limit sized from the shape's
main child (MIOpen's search at 100^3 may take minutes); one that does not finish is recorded as such, the comparison then uses
`torch` alone, and nothing more is started.
`op_wins`: in all four (pass, form) pairs the op's third quartile lies below the first quartile of torch's faster setting --
encoder.fused_site()'s criterion.  manigaussian_amd/volume.py's dense_site() is set from these.
`decoder_segment`: up0 -> final([d0, .]) -> trans_decoder, forward + backward at [1,256,20^3] + [1,128,100^3], with volume.DENSE
following the rule, forced on and forced off (forced off is the parent commit's behaviour), in this same run, with the peak
allocations.
FLOP counts are DERIVED from the shapes, not measured; times are measured.
Every shape is timed in a child process of its own under `timeout` (the 100^3 children's limits sized from the 50^3 children, which
run first); the first main child that fails ends the run.
Writes --out (default profiles/dense_conv_bench.json) and prints it as one JSON line.  Needs a HIP device: a CPU has nothing to time.
`agreement`: at the two 50^3 shapes, the op against torch WITHOUT the activation (max |difference| of y, dx, dw and db beside each
one's largest magnitude), and with it the number of outputs whose sign differs between the two fp32 runs: such an element takes the
other branch of the leaky ReLU in the backward, which is where the shapes' `max_abs_difference` of the gradients comes from.
--resume takes up an existing --out of the same build: it runs what that run did not (torch_benchmark children it recorded as not
started, the agreement) and leaves every other figure as it is.
--refresh-routing rewrites only `routing_in_the_package` and `routed_shapes` of an existing --out from the package's rule as it
stands (no device needed): they state what the package does with the measured shapes, and the rule is set after the measurement."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_conv3d import RUNS, SAMPLE_MS, Timer, benchmark_on, op_wins  # noqa: E402

SLOPE = 0.02
# name: cin, cout, k, unpadded side; in the order they run (a site's smaller size first)
SHAPES = {"up0_first_20": (256, 128, 5, 20), "up0_last_50": (128, 128, 5, 50), "final_50": (256, 128, 3, 50),
          "up0_last_100": (128, 128, 5, 100), "final_100": (256, 128, 3, 100)}
SIZED_FROM = {"up0_last_100": "up0_last_50", "final_100": "final_50"}
FIRST_LIMIT_S = int(os.environ.get("DENSE_SHAPE_TIMEOUT", "240"))
MAX_LIMIT_S = int(os.environ.get("DENSE_MAX_TIMEOUT", "420"))
FP32_MATRIX_FLOP_PER_S = 157.3e12
PASSES = ("forward", "backward_data", "backward_weight_bias")


def say(msg):
    print("bench_dense:", msg, file=sys.stderr, flush=True)


def shape_entry(name):
    cin, cout, k, side = SHAPES[name]
    n = side ** 3
    flop = 2 * k ** 3 * cin * cout * n
    return {"cin": cin, "cout": cout, "k": k, "side": side, "voxels": n, "x": [1, cin] + [side + k - 1] * 3, "y": [1, cout] + [side] * 3,
            "derived": {"flop_per_pass": flop, "flop_forward_backward": 3 * flop,
                        "bytes_padded_gradient": 4 * cout * (side + 2 * (k - 1)) ** 3,
                        "note": "derived from the shapes, not measured: 2 Cin Cout k^3 FLOP per output voxel and pass; the padded "
                                "gradient is the op's one temporary"}}


def tensors(torch, name):
    cin, cout, k, side = SHAPES[name]
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(9)
    x = torch.randn(1, cin, *[side + k - 1] * 3, generator=gen).to(dev).requires_grad_(True)
    g = torch.randn(1, cout, *[side] * 3, generator=gen).to(dev)
    w = (torch.randn(cout, cin, k, k, k, generator=gen) * (cin * k ** 3) ** -0.5).to(dev).requires_grad_(True)
    b = torch.randn(cout, generator=gen).to(dev).requires_grad_(True)
    return x, w, b, g


def measure_shape(name):
    import torch
    import torch.nn.functional as F

    from manigaussian_amd import _lib, _ops, dense_conv3d
    dev = torch.device("cuda:0")
    torch.backends.cudnn.benchmark = False
    tm = Timer(torch)
    entry = shape_entry(name)
    cin, cout, k, side = SHAPES[name]
    ext = (side + k - 1,) * 3
    x, w, b, g = tensors(torch, name)

    def fwd_torch():
        return F.leaky_relu(F.conv3d(x, w, b), SLOPE)

    def fwd_op():
        return dense_conv3d(x, w, b, SLOPE)

    def both(fwd):
        return lambda: torch.autograd.grad(fwd(), [x, w, b], g)

    xd, wd, bd = x.detach(), w.detach(), b.detach()
    y_buf, dx_buf, dw_buf, db_buf = torch.empty_like(g), torch.empty_like(xd), torch.empty_like(wd), torch.empty_like(bd)
    scratch = torch.empty(1, cout, *[side + 2 * (k - 1)] * 3, device=dev)
    ws = _ops.workspace(dev, _lib.lib().mgs_dense_conv3d_workspace_bytes(1, cin, cout, k, *ext))

    def op_forward():
        _ops.call("mgs_dense_conv3d_forward", dev, 1, cin, cout, k, *ext, SLOPE, xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y_buf.data_ptr(),
                  ws.data_ptr(), ws.numel())

    def op_backward(dx, dw, db):
        return lambda: _ops.call("mgs_dense_conv3d_backward", dev, 1, cin, cout, k, *ext, SLOPE, xd.data_ptr(), y_buf.data_ptr(), g.data_ptr(),
                                 wd.data_ptr(), _ops.ptr(dx), _ops.ptr(dw), _ops.ptr(db), scratch.data_ptr() if dx is not None else None,
                                 ws.data_ptr(), ws.numel(), 0)

    op_forward()   # (y_buf holds the op's y from here on: the backward passes read its sign)
    op_passes = {"forward": op_forward, "backward_data": op_backward(dx_buf, None, None),
                 "backward_weight_bias": op_backward(None, dw_buf, db_buf)}

    def conv_backward(mask):   # (the gradient of the convolution alone: torch's leaky ReLU backward is one more elementwise launch)
        return torch.ops.aten.convolution_backward(g, xd, wd, [cout], [1] * 3, [0] * 3, [1] * 3, False, [0] * 3, 1, mask)

    def torch_forward():
        with torch.no_grad():
            return F.leaky_relu(F.conv3d(xd, wd, bd), SLOPE)

    torch_passes = {"forward": torch_forward, "backward_data": lambda: conv_backward([True, False, False]),
                    "backward_weight_bias": lambda: conv_backward([False, True, True])}
    entry["passes_us"] = {"op": {}, "torch": {}}
    for p in PASSES:
        r = tm.alternate({"op": op_passes[p], "torch": torch_passes[p]})
        entry["passes_us"]["op"][p], entry["passes_us"]["torch"][p] = r["op"], r["torch"]
        say(f"{name} {p}: op {r['op']['median_us']} us, torch {r['torch']['median_us']} us")
    entry["op_backward_all_us"] = tm.alternate({"op": op_backward(dx_buf, dw_buf, db_buf)})["op"]
    del scratch, dx_buf, dw_buf
    # the results agree (the tests hold the bound; this guards the table against timing something else)
    want = torch.autograd.grad(fwd_torch(), [x, w, b], g)
    got = torch.autograd.grad(fwd_op(), [x, w, b], g)
    with torch.no_grad():
        entry["max_abs_difference"] = {"y": float((fwd_op() - fwd_torch()).abs().max()), "dx": float((got[0] - want[0]).abs().max()),
                                       "dw": float((got[1] - want[1]).abs().max()), "db": float((got[2] - want[2]).abs().max())}
    del want, got
    entry["forward"] = tm.compare({"op": fwd_op, "torch": fwd_torch})
    entry["forward_backward"] = tm.compare({"op": both(fwd_op), "torch": both(fwd_torch)}, peak=True)
    flop = entry["derived"]["flop_per_pass"]
    entry["achieved_tflops"] = {p: round(flop / (entry["passes_us"]["op"][p]["median_us"] * 1e-6) / 1e12, 2) for p in PASSES}
    entry["achieved_tflops"]["torch"] = {p: round(flop / (entry["passes_us"]["torch"][p]["median_us"] * 1e-6) / 1e12, 2) for p in PASSES}
    entry["achieved_tflops"]["fp32_matrix_peak"] = FP32_MATRIX_FLOP_PER_S / 1e12
    entry["achieved_tflops"]["note"] = "derived FLOP over the measured eager medians of the passes on their own"
    say(f"{name} " + json.dumps({p: {f: {s: entry[p][f][s]["median_us"] for s in entry[p][f]} for f in ("eager", "graph")}
                                 for p in ("forward", "forward_backward")}) + " TFLOP/s " + json.dumps({p: entry["achieved_tflops"][p] for p in PASSES}))
    return entry


def measure_benchmark(name):
    """torch's side alone with cudnn.benchmark on: {pass: {form: summary}}"""
    import torch
    import torch.nn.functional as F
    torch.backends.cudnn.benchmark = False
    tm = Timer(torch)
    x, w, b, g = tensors(torch, name)

    def fwd_torch():
        return F.leaky_relu(F.conv3d(x, w, b), SLOPE)

    fwd = benchmark_on(torch, fwd_torch)
    both = benchmark_on(torch, lambda: torch.autograd.grad(fwd_torch(), [x, w, b], g))
    out = {"forward": tm.compare({"torch_benchmark": fwd}), "forward_backward": tm.compare({"torch_benchmark": both}, peak=True)}
    say(f"{name} torch_benchmark " + json.dumps({p: {f: out[p][f]["torch_benchmark"]["median_us"] for f in out[p]} for p in out}))
    return out


def measure_segment():
    import torch

    from manigaussian_amd import volume as vol
    dev = torch.device("cuda:0")
    torch.backends.cudnn.benchmark = False
    tm = Timer(torch)
    torch.manual_seed(5)
    up0 = vol.Conv3DUpsampleBlock(256, 128, 5, kernel_sizes=5, norm=None, activation="lrelu").to(dev)
    final = vol.Conv3DBlock(256, 128, kernel_sizes=3, strides=1, norm=None, activation="lrelu").to(dev)
    trans = vol.Conv3DBlock(128, 1, kernel_sizes=3, strides=1, norm=None, activation=None).to(dev)
    params = [p for m in (up0, final, trans) for p in m.parameters()]
    gen = torch.Generator().manual_seed(6)
    latents = torch.randn(1, 256, 20, 20, 20, generator=gen).to(dev).requires_grad_(True)
    d0 = torch.randn(1, 128, 100, 100, 100, generator=gen).to(dev).requires_grad_(True)
    g = torch.randn(1, 1, 100, 100, 100, generator=gen).to(dev)
    saved = vol.DENSE

    def step(dense):
        def call():
            vol.DENSE = dense
            try:
                out = trans(final([d0, up0(latents)]))
                return torch.autograd.grad(out, [latents, d0] + params, g)
            finally:
                vol.DENSE = saved
        return call

    calls = {"rule": step(None), "forced_on": step(True), "forced_off": step(False)}
    entry = {"shapes": {"latents": [1, 256, 20, 20, 20], "d0": [1, 128, 100, 100, 100]}, "forward_backward": tm.compare(calls, peak=True),
             "note": "forced_off is the parent commit's behaviour, measured in this same run"}
    entry.update({k: entry["forward_backward"]["eager"][k] for k in calls})
    say("segment " + json.dumps({f: {k: v["median_us"] for k, v in entry["forward_backward"][f].items()} for f in ("eager", "graph")}))
    return entry


def measure_agreement():
    import torch
    import torch.nn.functional as F

    from manigaussian_amd import dense_conv3d
    out = {}
    for name in ("final_50", "up0_last_50"):
        x, w, b, g = tensors(torch, name)
        want = torch.autograd.grad(F.conv3d(x, w, b), [x, w, b], g)
        got = torch.autograd.grad(dense_conv3d(x, w, b), [x, w, b], g)
        with torch.no_grad():
            y_t, y_o = F.conv3d(x, w, b), dense_conv3d(x, w, b)
            e = {"without_activation": {q: {"max_abs_difference": float((a - c).abs().max()), "max_abs": float(c.abs().max())}
                                        for q, a, c in zip(("y", "dx", "dw", "db"), (y_o,) + got, (y_t,) + want)}}
            y_t, y_o = F.leaky_relu(y_t, SLOPE), dense_conv3d(x, w, b, SLOPE)
            e["outputs"] = y_t.numel()
            e["outputs_whose_sign_differs"] = int(((y_t > 0) != (y_o > 0)).sum())
            e["outputs_within_1e-5_of_zero"] = int((F.conv3d(x, w, b).abs() < 1e-5).sum())
        out[name] = e
        say(f"{name} agreement " + json.dumps(e))
        del want, got, y_t, y_o
    return out


def child(args):
    import torch
    if not torch.cuda.is_available():
        print("bench_dense: no HIP device; nothing is timed on a CPU", file=sys.stderr)
        return 2
    if args.segment:
        part = measure_segment()
    elif args.agreement:
        part = measure_agreement()
    elif args.benchmark:
        part = measure_benchmark(args.shape)
    else:
        part = measure_shape(args.shape)
    with open(args.part, "w") as f:
        json.dump(part, f)
    return 0


def routing(result):
    from manigaussian_amd import volume as vol
    result["routing_in_the_package"] = {k: bool(vol.dense_site(v["cin"], v["cout"], v["k"], v["voxels"])) for k, v in result["shapes"].items()}
    result["routed_shapes"] = sorted(k for k, v in result["routing_in_the_package"].items() if v)


def write(result, out):
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_conv_bench.json"))
    ap.add_argument("--refresh-routing", action="store_true", help="rewrite the routing fields of --out from the package's rule; no device")
    ap.add_argument("--budget-s", type=int, default=1000, help="the torch_benchmark children start only while this many seconds are not used up")
    ap.add_argument("--shape", help="(child) measure this shape into --part")
    ap.add_argument("--benchmark", action="store_true", help="(child) torch with cudnn.benchmark on alone")
    ap.add_argument("--segment", action="store_true", help="(child) the decoder segment")
    ap.add_argument("--agreement", action="store_true", help="(child) the op against torch without the activation")
    ap.add_argument("--resume", action="store_true", help="take up an existing --out of the same build: run only what it lacks")
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
        print("bench_dense: no HIP device; nothing is timed on a CPU", file=sys.stderr)
        return 2
    began = time.time()
    result = {"device": torch.cuda.get_device_name(0), "build_id": _lib.build_id(), "runs": RUNS, "sample_ms": SAMPLE_MS,
              "times_are": "measured, microseconds per call", "flop_are": "derived from the shapes", "shapes": {}}
    if args.resume:
        with open(args.out) as f:
            earlier = json.load(f)
        if earlier["build_id"] != result["build_id"]:
            say(f"--resume: {args.out} is of build {earlier['build_id']}, the library of {result['build_id']}")
            return 1
        result = earlier
    tmp = tempfile.mkdtemp(prefix="bench_dense_")

    def run_child(tag, flags, limit):
        part = os.path.join(tmp, tag + ".json")
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--part", part] + flags
        say(f"{tag} (limit {limit} s)")
        t0 = time.time()
        rc = subprocess.run(cmd).returncode
        took = time.time() - t0
        if rc != 0:
            return rc, took, None
        with open(part) as f:
            return 0, took, json.load(f)

    took = {}
    for name in SHAPES:
        if name in result["shapes"]:
            took[name] = result["shapes"][name]["child_seconds"]
            continue
        limit = FIRST_LIMIT_S
        if name in SIZED_FROM:   # 8 x the voxels of the half-size child, with as much again to spare
            limit = int(min(MAX_LIMIT_S, max(120, 16 * took[SIZED_FROM[name]])))
        rc, took[name], part = run_child(name, ["--shape", name], limit)
        if rc != 0:
            say(f"{name}: exit {rc}; nothing more is started")
            return 1
        part["child_seconds"] = round(took[name], 1)
        result["shapes"][name] = part
        write(result, args.out)   # (what is measured so far survives a later child's failure)
    for key, flag in (("decoder_segment", "--segment"), ("agreement", "--agreement")):
        if key in result:
            continue
        rc, _, part = run_child(key, [flag], MAX_LIMIT_S)
        if rc != 0:
            say(f"{key}: exit {rc}; nothing more is started")
            return 1
        result[key] = part
        write(result, args.out)

    # torch with cudnn.benchmark on: last, smallest first; the first one that does not finish ends the run
    stopped = None
    for name in sorted(SHAPES, key=lambda n: SHAPES[n][3] ** 3 * SHAPES[n][0] * SHAPES[n][2] ** 3):
        entry = result["shapes"][name]
        have = entry["forward"]["eager"].get("torch_benchmark")
        if have is not None and not str(have.get("why", "")).startswith("not started"):
            continue
        left = args.budget_s - (time.time() - began)
        limit = int(min(MAX_LIMIT_S, max(60, 3 * took[name]), left))
        if stopped is not None or limit < 60:
            note = {"did_not_finish": True, "why": f"not started: {stopped}" if stopped else "not started: the run's time budget was used up"}
        else:
            rc, _, part = run_child(name + "_torch_benchmark", ["--shape", name, "--benchmark"], limit)
            if rc != 0:
                stopped = f"{name}'s child did not finish within {limit} s (exit {rc})"
                say(stopped + "; nothing more is started")
                note = {"did_not_finish": True, "why": f"exit {rc} under a limit of {limit} s", "limit_s": limit}
            else:
                note = None
                for p in ("forward", "forward_backward"):
                    for f in ("eager", "graph"):
                        entry[p][f]["torch_benchmark"] = part[p][f]["torch_benchmark"]
        if note is not None:
            for p in ("forward", "forward_backward"):
                for f in ("eager", "graph"):
                    entry[p][f]["torch_benchmark"] = note
        entry["op_wins"] = op_wins(entry, benchmark_may_be_missing=True)   # (a torch_benchmark child may not have finished)

    result["routing_as_measured"] = {k: v["op_wins"] for k, v in result["shapes"].items()}
    routing(result)
    print(json.dumps(result, sort_keys=True))
    write(result, args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
