"""The Perceiver's patch embedding (agents/manigaussian_bc/perceiver_lang_io.py:235: patchify = Conv3DBlock(128, 128, kernel_sizes=5,
strides=5, activation='relu') = nn.Conv3d(128, 128, 5, stride=5, padding=2, padding_mode='replicate') + ReLU), fp32, B = 1, at
ManiGaussian's 100^3 grid and at 50^3 and 25^3 (so that the routing rule has more than one point), and at PerAct's 64 -> 64 at 100^3:
  patchify_100, patchify_50, patchify_25    128 -> 128, k = stride = 5, pad 2, [1,128,side^3] -> [1,128,(side/5)^3]
  peract_100                                64 -> 64, the same at 100^3
two ways:
  op      manigaussian_amd.patch_conv3d (csrc/mgs_patch.hip): pad, convolution, bias and ReLU in one op on the unpadded volume
  torch   the parent commit's path, F.relu(F.conv3d(volume.resample_pad(x, 1, 2), w, b, stride=5)), with
          torch.backends.cudnn.benchmark off (`torch`) and on (`torch_benchmark`)
Per shape, in ONE process, the sides alternating (scripts/bench_conv3d.py's protocol and its Timer):
  passes_us         the passes on their own, eager: forward, backward_data (dx alone) and backward_weight_bias (dw and db alone);
                    torch's forward is pad + convolution + ReLU; its backward passes are aten.convolution_backward on the padded
                    volume with those outputs asked for, backward_data followed by resample_pad's own backward, cudnn.benchmark off
                    (torch's ReLU backward, one more elementwise launch over y, is not in them; the op's passes include it);
                    `op_backward_all_us`: the op's dx, dw and db in one call
  forward, forward_backward   as in a training step (autograd recording; gradients towards x, weight and bias), each EAGER and
                    GRAPH-REPLAYED; peak_bytes: the peak allocation of one eager forward + backward above the inputs
  achieved_tflops   the DERIVED FLOP of a pass (2 Cin Cout k^3 per patch) over the op's measured median, beside the 157.3 TFLOP/s fp32
                    matrix peak; `torch`: the same over torch's medians
`torch_benchmark` runs in children of its own AFTER everything else, smallest shape first, each under a limit sized from the shape's
main child (MIOpen's search may take minutes); one that does not finish is recorded as such, the comparison then uses `torch` alone,
and nothing more is started.
`op_wins`: in all four (pass, form) pairs the op's third quartile lies below the first quartile of torch's faster setting --
encoder.fused_site()'s criterion.  manigaussian_amd/volume.py's PATCH_MIN_VOXELS is set from these.
`patchify_block`: the whole Conv3DBlock(128, 128, 5, 5, 'relu') forward + backward at [1,128,100^3] with volume.PATCH following the
rule, forced on and forced off (forced off is the parent commit's behaviour), in this same run, with the peak allocations.
FLOP and byte counts are DERIVED from the shapes, not measured; times are measured.
Every shape is timed in a child process of its own under `timeout`; the first main child that fails ends the run.
Writes --out (default profiles/patch_conv_bench.json) and prints it as one JSON line.  Needs a HIP device: a CPU has nothing to time.
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

K, PAD = 5, 2
# name: cin, cout, side; in the order they run (smallest first)
SHAPES = {"patchify_25": (128, 128, 25), "patchify_50": (128, 128, 50), "peract_100": (64, 64, 100), "patchify_100": (128, 128, 100)}
SHAPE_LIMIT_S = int(os.environ.get("PATCH_SHAPE_TIMEOUT", "240"))
FP32_MATRIX_FLOP_PER_S = 157.3e12
ROOFLINE_BYTES_PER_S = 8.0e12
PASSES = ("forward", "backward_data", "backward_weight_bias")


def say(msg):
    print("bench_patch:", msg, file=sys.stderr, flush=True)


def shape_entry(name):
    cin, cout, side = SHAPES[name]
    out = (side + 2 * PAD - K) // K + 1
    patches = out ** 3
    flop = 2 * K ** 3 * cin * cout * patches
    return {"cin": cin, "cout": cout, "k": K, "pad": PAD, "side": side, "voxels": side ** 3, "x": [1, cin] + [side] * 3, "y": [1, cout] + [out] * 3,
            "derived": {"flop_per_pass": flop, "flop_forward_backward": 3 * flop,
                        "bytes_forward": 4 * (cin * side ** 3 + cout * patches + cout * cin * K ** 3 + cout),
                        "bytes_padded_copy": 4 * cin * (side + 2 * PAD) ** 3,
                        "floor_us": {"matrix": round(flop / FP32_MATRIX_FLOP_PER_S * 1e6, 1),
                                     "memory_forward": round(4 * cin * side ** 3 / ROOFLINE_BYTES_PER_S * 1e6, 1)},
                        "note": "derived from the shapes, not measured: 2 Cin Cout k^3 FLOP per patch and pass; the forward reads x once; "
                                "the padded copy is what the parent's path writes and reads back"}}


def tensors(torch, name):
    cin, cout, side = SHAPES[name]
    out = (side + 2 * PAD - K) // K + 1
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(9)
    x = torch.randn(1, cin, side, side, side, generator=gen).to(dev).requires_grad_(True)
    g = torch.randn(1, cout, out, out, out, generator=gen).to(dev)
    w = (torch.randn(cout, cin, K, K, K, generator=gen) * (cin * K ** 3) ** -0.5).to(dev).requires_grad_(True)
    b = torch.randn(cout, generator=gen).to(dev).requires_grad_(True)
    return x, w, b, g


def measure_shape(name):
    import torch
    import torch.nn.functional as F

    from manigaussian_amd import _lib, _ops, patch_conv3d
    from manigaussian_amd import volume as vol
    dev = torch.device("cuda:0")
    torch.backends.cudnn.benchmark = False
    tm = Timer(torch)
    entry = shape_entry(name)
    cin, cout, side = SHAPES[name]
    ext = (side,) * 3
    x, w, b, g = tensors(torch, name)

    def fwd_torch():   # the parent commit's Conv3DBlock.forward
        return F.relu(F.conv3d(vol.resample_pad(x, 1, PAD), w, b, stride=K))

    def fwd_op():
        return patch_conv3d(x, w, b, PAD, "replicate", 0.0)

    def both(fwd):
        return lambda: torch.autograd.grad(fwd(), [x, w, b], g)

    xd, wd, bd = x.detach(), w.detach(), b.detach()
    y_buf, dx_buf, dw_buf, db_buf = torch.empty_like(g), torch.empty_like(xd), torch.empty_like(wd), torch.empty_like(bd)
    ws = _ops.workspace(dev, _lib.lib().mgs_patch_conv3d_workspace_bytes(1, cin, cout, K, PAD, *ext))

    def op_forward():
        _ops.call("mgs_patch_conv3d_forward", dev, 1, cin, cout, K, PAD, *ext, 0, 0.0, xd.data_ptr(), wd.data_ptr(), bd.data_ptr(),
                  y_buf.data_ptr(), ws.data_ptr(), ws.numel())

    def op_backward(dx, dw, db):
        need_ws = dw is not None or db is not None
        return lambda: _ops.call("mgs_patch_conv3d_backward", dev, 1, cin, cout, K, PAD, *ext, 0, 0.0, xd.data_ptr(), y_buf.data_ptr(),
                                 g.data_ptr(), wd.data_ptr(), _ops.ptr(dx), _ops.ptr(dw), _ops.ptr(db), ws.data_ptr() if need_ws else None,
                                 ws.numel() if need_ws else 0, 0)

    op_forward()   # (y_buf holds the op's y from here on: the backward passes read its sign)
    op_passes = {"forward": op_forward, "backward_data": op_backward(dx_buf, None, None),
                 "backward_weight_bias": op_backward(None, dw_buf, db_buf)}

    with torch.no_grad():
        padded = vol.resample_pad(xd, 1, PAD)

    def conv_backward(mask):   # (the gradient of the convolution alone)
        return torch.ops.aten.convolution_backward(g, padded, wd, [cout], [K] * 3, [0] * 3, [1] * 3, False, [0] * 3, 1, mask)

    pad_probe = vol.resample_pad(x, 1, PAD)   # (its autograd node turns a padded gradient into x's)

    def torch_forward():
        with torch.no_grad():
            return F.relu(F.conv3d(vol.resample_pad(xd, 1, PAD), wd, bd, stride=K))

    def torch_backward_data():
        gp = conv_backward([True, False, False])[0]
        return torch.autograd.grad(pad_probe, x, gp, retain_graph=True)

    torch_passes = {"forward": torch_forward, "backward_data": torch_backward_data,
                    "backward_weight_bias": lambda: conv_backward([False, True, True])}
    entry["passes_us"] = {"op": {}, "torch": {}}
    for p in PASSES:
        r = tm.alternate({"op": op_passes[p], "torch": torch_passes[p]})
        entry["passes_us"]["op"][p], entry["passes_us"]["torch"][p] = r["op"], r["torch"]
        say(f"{name} {p}: op {r['op']['median_us']} us, torch {r['torch']['median_us']} us")
    entry["op_backward_all_us"] = tm.alternate({"op": op_backward(dx_buf, dw_buf, db_buf)})["op"]
    del pad_probe, padded, dx_buf, dw_buf
    # the results agree (the tests hold the bound; this guards the table against timing something else)
    want = torch.autograd.grad(fwd_torch(), [x, w, b], g)
    got = torch.autograd.grad(fwd_op(), [x, w, b], g)
    with torch.no_grad():
        y_t, y_o = fwd_torch(), fwd_op()
        entry["max_abs_difference"] = {"y": float((y_o - y_t).abs().max()), "dx": float((got[0] - want[0]).abs().max()),
                                       "dw": float((got[1] - want[1]).abs().max()), "db": float((got[2] - want[2]).abs().max())}
        entry["outputs_whose_sign_differs"] = int(((y_t > 0) != (y_o > 0)).sum())
    del want, got, y_t, y_o
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

    from manigaussian_amd import volume as vol
    torch.backends.cudnn.benchmark = False
    tm = Timer(torch)
    x, w, b, g = tensors(torch, name)

    def fwd_torch():
        return F.relu(F.conv3d(vol.resample_pad(x, 1, PAD), w, b, stride=K))

    fwd = benchmark_on(torch, fwd_torch)
    both = benchmark_on(torch, lambda: torch.autograd.grad(fwd_torch(), [x, w, b], g))
    out = {"forward": tm.compare({"torch_benchmark": fwd}), "forward_backward": tm.compare({"torch_benchmark": both}, peak=True)}
    say(f"{name} torch_benchmark " + json.dumps({p: {f: out[p][f]["torch_benchmark"]["median_us"] for f in out[p]} for p in out}))
    return out


def measure_block():
    import torch

    from manigaussian_amd import volume as vol
    dev = torch.device("cuda:0")
    torch.backends.cudnn.benchmark = False
    tm = Timer(torch)
    torch.manual_seed(5)
    block = vol.Conv3DBlock(128, 128, kernel_sizes=K, strides=K, norm=None, activation="relu").to(dev)
    with torch.no_grad():
        block.conv3d.bias.normal_()
    params = list(block.parameters())
    gen = torch.Generator().manual_seed(6)
    x = torch.randn(1, 128, 100, 100, 100, generator=gen).to(dev).requires_grad_(True)
    g = torch.randn(1, 128, 20, 20, 20, generator=gen).to(dev)
    saved = vol.PATCH

    def step(patch):
        def call():
            vol.PATCH = patch
            try:
                return torch.autograd.grad(block(x), [x] + params, g)
            finally:
                vol.PATCH = saved
        return call

    calls = {"rule": step(None), "forced_on": step(True), "forced_off": step(False)}
    entry = {"shapes": {"x": [1, 128, 100, 100, 100]}, "forward_backward": tm.compare(calls, peak=True),
             "note": "forced_off is the parent commit's behaviour, measured in this same run"}
    entry.update({k: entry["forward_backward"]["eager"][k] for k in calls})
    say("block " + json.dumps({f: {k: v["median_us"] for k, v in entry["forward_backward"][f].items()} for f in ("eager", "graph")}))
    return entry


def child(args):
    import torch
    if not torch.cuda.is_available():
        print("bench_patch: no HIP device; nothing is timed on a CPU", file=sys.stderr)
        return 2
    if args.block:
        part = measure_block()
    elif args.benchmark:
        part = measure_benchmark(args.shape)
    else:
        part = measure_shape(args.shape)
    with open(args.part, "w") as f:
        json.dump(part, f)
    return 0


def routing(result):
    from manigaussian_amd import volume as vol
    result["routing_in_the_package"] = {k: bool(vol.patch_site(v["cin"], v["cout"], v["k"], v["voxels"])) for k, v in result["shapes"].items()}
    result["routed_shapes"] = sorted(k for k, v in result["routing_in_the_package"].items() if v)


def write(result, out):
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "patch_conv_bench.json"))
    ap.add_argument("--refresh-routing", action="store_true", help="rewrite the routing fields of --out from the package's rule; no device")
    ap.add_argument("--budget-s", type=int, default=700, help="the torch_benchmark children start only while this many seconds are not used up")
    ap.add_argument("--shape", help="(child) measure this shape into --part")
    ap.add_argument("--benchmark", action="store_true", help="(child) torch with cudnn.benchmark on alone")
    ap.add_argument("--block", action="store_true", help="(child) the patchify block")
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
        print("bench_patch: no HIP device; nothing is timed on a CPU", file=sys.stderr)
        return 2
    began = time.time()
    result = {"device": torch.cuda.get_device_name(0), "build_id": _lib.build_id(), "runs": RUNS, "sample_ms": SAMPLE_MS,
              "times_are": "measured, microseconds per call", "flop_and_bytes_are": "derived from the shapes", "shapes": {}}
    tmp = tempfile.mkdtemp(prefix="bench_patch_")

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
        rc, took[name], part = run_child(name, ["--shape", name], SHAPE_LIMIT_S)
        if rc != 0:
            say(f"{name}: exit {rc}; nothing more is started")
            return 1
        part["child_seconds"] = round(took[name], 1)
        result["shapes"][name] = part
        write(result, args.out)   # (what is measured so far survives a later child's failure)
    rc, _, part = run_child("patchify_block", ["--block"], SHAPE_LIMIT_S)
    if rc != 0:
        say(f"patchify_block: exit {rc}; nothing more is started")
        return 1
    result["patchify_block"] = part
    write(result, args.out)

    # torch with cudnn.benchmark on: last, smallest first; the first one that does not finish ends the run
    stopped = None
    for name in SHAPES:
        entry = result["shapes"][name]
        left = args.budget_s - (time.time() - began)
        limit = int(min(SHAPE_LIMIT_S, max(60, 4 * took[name]), left))
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
