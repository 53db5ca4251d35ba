"""The voxel encoder stem's ten normalisation sites (helpers/network_utils.py:248-306), two ways, at the shapes ManiGaussian runs
(B = 1, a 100^3 grid), fp32, in one process:
  fused  manigaussian_amd.batch_norm_act (csrc/mgs_abn.hip)
  torch  the reference's sequence on the same GPU: nn.BatchNorm3d (training mode) -> nn.LeakyReLU(inplace=True) (-> skip + y)
Sites of one shape share a measurement (conv1 and conv2; conv3 and conv4; conv5 and conv6).  Per shape: forward (with autograd
recording, as in a training step) and forward + backward, each EAGER (calls from Python) and GRAPH-REPLAYED (one call captured into
a HIP graph).  A sample is `inner` consecutive calls between two device events, `inner` chosen so that a sample lasts about
SAMPLE_MS; ENCODER_RUNS (default 9, at least 7) samples per side, the two sides alternating.  The whole list of shapes is gone
through ENCODER_ROUNDS (default 2) times, one round after the other, with fresh tensors, modules and graphs: an eager call that is
bound by the host's enqueue path can settle at another speed from one minute to the next, and only a second round shows it.
Reported per (shape, pass, form, side), over the samples of all rounds: the median, the quartiles, the minimum and the maximum, in
microseconds per call, the rounds' own medians (`round_medians_us`), and the peak allocation of one call above what was held before.
`fused_wins`: in all four (pass, form) pairs the fused side's third quartile lies below torch's first quartile -- faster by more
than the run-to-run spread of either, rounds included.  manigaussian_amd/encoder.py's fused_site() is set from these.
Then the whole stem, forward + backward at [1, 10, 100^3], with every site fused (encoder.FORCE = True) and none (False), reported
the same way.
Bytes are DERIVED from the shapes (what the passes of each side have to move), not measured; times are measured.
Writes --out (default profiles/encoder_bench.json) and prints it as one JSON line.  Needs a HIP device: a CPU has nothing to time."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# site, channels, level (the grid's side halved, rounding up, that many times: 100, 50, 25, 13), followed by a skip add
SITES = (("conv0", 8, 0, False), ("conv1", 16, 1, False), ("conv2", 16, 1, False), ("conv3", 32, 2, False),
         ("conv4", 32, 2, False), ("conv5", 64, 3, False), ("conv6", 64, 3, False), ("conv7", 32, 2, True),
         ("conv9", 16, 1, True), ("conv11", 8, 0, True))
RUNS = max(7, int(os.environ.get("ENCODER_RUNS", "9")))
ROUNDS = max(1, int(os.environ.get("ENCODER_ROUNDS", "2")))
WARMUP = 3
SAMPLE_MS = 4.0
MAX_INNER = 200


def say(msg):
    print("bench_encoder:", msg, file=sys.stderr, flush=True)


def summary(samples):
    s = sorted(samples)
    q = statistics.quantiles(s, n=4, method="inclusive")
    return {"median_us": round(statistics.median(s), 2), "q1_us": round(q[0], 2), "q3_us": round(q[2], 2), "min_us": round(s[0], 2),
            "max_us": round(s[-1], 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encoder_bench.json"))
    ap.add_argument("--no-stem", action="store_true", help="the ten sites only")
    ap.add_argument("--grid", type=int, default=100, help="the voxel grid's side (100: ManiGaussian's)")
    args = ap.parse_args()

    import torch
    from torch import nn

    from manigaussian_amd import _lib, batch_norm_act
    from manigaussian_amd import encoder as enc

    if not torch.cuda.is_available():
        print("bench_encoder: no HIP device; nothing is timed on a CPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda:0")

    def sample(call, inner):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(inner):
            call()
        end.record()
        end.synchronize()
        return start.elapsed_time(end) * 1000.0 / inner

    def inner_for(call):
        for _ in range(WARMUP):
            call()
        torch.cuda.synchronize()
        est = sample(call, 3)
        return max(3, min(MAX_INNER, int(SAMPLE_MS * 1000.0 / max(est, 1.0))))

    def peak_of(call):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        call()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    def captured(call):
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

    def compare(calls):
        """calls: {side: callable} -> {form: {side: {"samples": [...], "inner", "peak_bytes"}}}; the sides' samples alternate."""
        out = {}
        for form in ("eager", "graph"):
            run = dict(calls)
            graphs = None
            if form == "graph":
                graphs = {k: captured(c) for k, c in calls.items()}
                run = {k: g.replay for k, g in graphs.items()}
            inner = {k: inner_for(c) for k, c in run.items()}
            samples = {k: [] for k in run}
            for _ in range(RUNS):
                for k, c in run.items():
                    samples[k].append(sample(c, inner[k]))
            out[form] = {k: {"samples": v, "inner": inner[k]} for k, v in samples.items()}
            if form == "eager":
                for k, c in calls.items():
                    out[form][k]["peak_bytes"] = peak_of(c)
            del graphs
        return out

    def pooled(rounds):
        """[compare() of every round] -> {form: {side: summary over all rounds' samples}}"""
        out = {}
        for form in rounds[0]:
            out[form] = {}
            for k in rounds[0][form]:
                every = [t for r in rounds for t in r[form][k]["samples"]]
                e = dict(summary(every), inner=rounds[0][form][k]["inner"],
                         round_medians_us=[round(statistics.median(r[form][k]["samples"]), 2) for r in rounds])
                if "peak_bytes" in rounds[0][form][k]:
                    e["peak_bytes"] = max(r[form][k]["peak_bytes"] for r in rounds)
                out[form][k] = e
        return out

    def wins(entry, a, b):
        return all(entry[form][a]["q3_us"] < entry[form][b]["q1_us"] for form in ("eager", "graph"))

    result = {"device": torch.cuda.get_device_name(0), "build_id": _lib.build_id(), "runs": RUNS, "rounds": ROUNDS,
              "sample_ms": SAMPLE_MS, "grid": args.grid, "times_are": "measured, microseconds per call",
              "bytes_are": "derived from the shapes", "shapes": {}}
    shapes = {}   # key -> (C, side, skip), in the sites' order
    for name, C, level, with_res in SITES:
        S = args.grid
        for _ in range(level):
            S = (S + 1) // 2
        key = f"C{C}_{S}^3" + ("_skip" if with_res else "")
        if key not in shapes:
            shapes[key] = (C, S, with_res)
            vol = 4 * C * S ** 3
            result["shapes"][key] = {"sites": [], "C": C, "side": S, "skip": with_res, "volume_bytes": vol,
                                     "derived_bytes": {"fused_forward": vol * (4 if with_res else 3), "fused_backward": vol * 5,
                                                       "torch_forward": vol * (8 if with_res else 5), "torch_backward": vol * 8}}
        result["shapes"][key]["sites"].append(name)

    def one_shape(C, S, with_res):
        gen = torch.Generator().manual_seed(7)
        x = torch.randn(1, C, S, S, S, generator=gen).to(dev).requires_grad_(True)
        g = torch.randn(1, C, S, S, S, generator=gen).to(dev)
        res = torch.randn(1, C, S, S, S, generator=gen).to(dev).requires_grad_(True) if with_res else None
        bn = {k: nn.BatchNorm3d(C).to(dev).train() for k in ("fused", "torch")}
        act = nn.LeakyReLU(inplace=True)

        def fwd_torch():
            y = act(bn["torch"](x))
            return y if res is None else res + y

        def fwd_fused():
            b = bn["fused"]
            return batch_norm_act(x, b.weight, b.bias, b.running_mean, b.running_var, b.num_batches_tracked, training=True,
                                  momentum=b.momentum, eps=b.eps, residual=res)

        def both(fwd, b):
            leaves = [x, b.weight, b.bias] + ([res] if res is not None else [])
            return lambda: torch.autograd.grad(fwd(), leaves, g)

        return {"forward": compare({"fused": fwd_fused, "torch": fwd_torch}),
                "forward_backward": compare({"fused": both(fwd_fused, bn["fused"]), "torch": both(fwd_torch, bn["torch"])})}

    def one_stem():
        S = args.grid
        torch.manual_seed(3)
        stem = enc.MultiLayer3DEncoderShallow().to(dev).train()
        gen = torch.Generator().manual_seed(8)
        x = torch.randn(1, 10, S, S, S, generator=gen).to(dev)
        g = torch.randn(1, 64, S, S, S, generator=gen).to(dev)
        params = list(stem.parameters())
        saved = enc.FORCE

        def step(force):
            def call():
                enc.FORCE = force
                try:
                    out, _ = stem(x)
                    return torch.autograd.grad(out, params, g)
                finally:
                    enc.FORCE = saved
            return call

        return {"forward_backward": compare({"fused": step(True), "torch": step(False)})}

    raw = {key: [] for key in shapes}
    raw_stem = []
    for rnd in range(ROUNDS):
        for key, (C, S, with_res) in shapes.items():
            say(f"round {rnd + 1}: {key}")
            raw[key].append(one_shape(C, S, with_res))
            torch.cuda.empty_cache()
        if not args.no_stem:
            say(f"round {rnd + 1}: stem")
            raw_stem.append(one_stem())
            torch.cuda.empty_cache()

    passes = ("forward", "forward_backward")
    for key, rounds in raw.items():
        entry = result["shapes"][key]
        for p in passes:
            entry[p] = pooled([r[p] for r in rounds])
        entry["fused_wins"] = all(wins(entry[p], "fused", "torch") for p in passes)
        say(key + " " + json.dumps({p: {f: {k: entry[p][f][k]["round_medians_us"] for k in ("fused", "torch")} for f in ("eager", "graph")}
                                    for p in passes}) + f" fused_wins={entry['fused_wins']}")
    if raw_stem:
        entry = {"shape": [1, 10, args.grid, args.grid, args.grid], "forward_backward": pooled([r["forward_backward"] for r in raw_stem])}
        entry["fused_wins"] = wins(entry["forward_backward"], "fused", "torch")
        result["stem"] = entry
        say("stem " + json.dumps({f: {k: entry["forward_backward"][f][k]["round_medians_us"] for k in ("fused", "torch")}
                                  for f in ("eager", "graph")}))

    result["routing_as_measured"] = {k: v["fused_wins"] for k, v in result["shapes"].items()}
    result["routing_in_the_package"] = {k: bool(enc.fused_site(v["side"] ** 3, v["C"])) for k, v in result["shapes"].items()}
    print(json.dumps(result, sort_keys=True))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
