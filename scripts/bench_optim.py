"""The optimizer step of ManiGaussian: the reference's per-tensor LAMB loop vs the fused step (manigaussian_amd.optim.FusedLamb).
The NeuralRenderer's trainable part: 62 tensors / 5 725 407 fp32 parameters (encoder ResnetFC(39 -> 26), the 26 x 26 regressor,
the deformation field's ResnetFC(73 -> 7); hidden width 512), lr 5e-4, weight decay 1e-6, fixed random gradients.
  (a)  this script's torch restatement of helpers/optim/lamb.py:47-111: a Python loop over the tensors, a dozen small kernels
       each, and the reference's two device reads per tensor (`if weight_norm == 0 or adam_norm == 0`, the tensor-valued alpha of
       the final add_) -- what a caller has without this module
  (b)  FusedLamb.step(): two launches
  (a2) a second copy of (a): the spread of the comparison itself
alternated step by step in one process, hipEvent-timed after warm-up, eager; (b) also replayed from a HIP graph, alone and
behind ManiGaussian's own step (two sets of 16 384 Gaussians, set-batch render + fused losses + backward, as
scripts/bench_loss.py builds it: the graph with and without the optimizer).  (a) cannot be captured: it reads the device.
Then a second size where the Gaussians themselves are the parameters (BASELINE configs[2]: six tensors of 100 000 rows,
3 + 1 + 12 + 3 + 4 + 32 floats per row): few, large, oddly shaped tensors.
Achieved rate = 40 bytes per parameter (moments pass 16 read + 8 written, apply pass 12 + 4) over the graph-replayed step.
Prints one JSON line and writes it to --out (default profiles/optim_bench.json).  BO_STEPS: timed steps (300).
BO_ONLY=a|b|gaussians: that variant's eager step only, untimed (for rocprofv3 --kernel-trace --stats)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import manigaussian_amd as mg  # noqa: E402
from manigaussian_amd import GaussianRasterizationSettings, GaussianRasterizerBatch, _lib, deform  # noqa: E402
from manigaussian_amd import synthetic as syn  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_bench.json"))
args = ap.parse_args()
STEPS = int(os.environ.get("BO_STEPS", "300"))
WARM = 20
HYPER = dict(lr=5e-4, betas=(0.9, 0.999), eps=1e-6, weight_decay=1e-6)
dev = torch.device("cuda:0")
torch.autograd.set_multithreading_enabled(False)


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
        fn()
    return graph


class LoopLamb:
    """LAMB as ManiGaussian's optimizer runs it, tensor by tensor with torch ops: moments without bias correction, weight norm
    clamped to [0, 10], the update m / (sqrt(v) + eps) + wd p, trust ratio 1 where a norm is zero (a device read), the final
    add_ with a tensor-valued alpha (a second device read)."""

    def __init__(self, params, lr, betas, eps, weight_decay):
        self.params, self.lr, self.betas, self.eps, self.wd = params, lr, betas, eps, weight_decay
        self.m = [torch.zeros_like(p) for p in params]
        self.v = [torch.zeros_like(p) for p in params]

    @torch.no_grad()
    def step(self):
        b1, b2 = self.betas
        for p, m, v in zip(self.params, self.m, self.v):
            g = p.grad
            if g is None:
                continue
            m.mul_(b1).add_(g, alpha=1 - b1)
            v.mul_(b2).addcmul_(g, g, value=1 - b2)
            weight_norm = p.pow(2).sum().sqrt().clamp(0, 10)
            u = m / v.sqrt().add(self.eps)
            if self.wd != 0:
                u.add_(p, alpha=self.wd)
            adam_norm = u.pow(2).sum().sqrt()
            trust = 1 if (weight_norm == 0 or adam_norm == 0) else weight_norm / adam_norm
            p.add_(u, alpha=-self.lr * trust)


def mani_params(hidden=512):
    """The 62 tensors (the repository's own modules, their default initialisation: Kaiming weights, zero biases and fc_1.weight)."""
    torch.manual_seed(0)
    mods = [deform.ResnetFC(39, d_out=26, n_blocks=5, d_latent=128, d_hidden=hidden, combine_layer=3), torch.nn.Linear(26, 26),
            deform.ResnetFC(73, d_out=7, n_blocks=5, d_latent=128, d_hidden=hidden, combine_layer=3)]
    return [p.detach().clone().to(dev).requires_grad_(True) for m in mods for p in m.parameters()]


def gaussian_params(P=100_000):
    g = torch.Generator().manual_seed(2)
    return [(0.1 * torch.randn(P, *s, generator=g)).to(dev).requires_grad_(True) for s in ((3,), (1,), (4, 3), (3,), (4,), (32,))]


def with_grads(params, seed):
    g = torch.Generator().manual_seed(seed)
    for p in params:
        p.grad = (0.02 * torch.randn(p.shape, generator=g)).to(dev)
    return params


def rates(n_params, ms):
    bps = 40.0 * n_params / (ms * 1e-3)
    return {"bytes": 40 * n_params, "TBps": bps / 1e12, "of_achievable_6.3": bps / 6.3e12, "of_peak_8.0": bps / 8e12}


def optimizer_bench(make, label):
    base = make()
    n = sum(p.numel() for p in base)
    sets = {k: with_grads([p.detach().clone().requires_grad_(True) for p in base], 3) for k in ("a", "b", "a2")}
    loop_a, loop_a2 = LoopLamb(sets["a"], **HYPER), LoopLamb(sets["a2"], **HYPER)
    fused = mg.FusedLamb(sets["b"], **HYPER)  # adopts the gradients into its flat buffer
    fns = {"a_torch_loop": loop_a.step, "b_fused": fused.step, "a2_torch_loop": loop_a2.step}
    for _ in range(WARM):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    diff = max(((x - y).abs().max() / y.abs().max().clamp_min(1e-30)).item() for x, y in zip(sets["b"], sets["a"]))
    out = {"set": label, "tensors": len(base), "parameters": n, "chunks": fused._layout["total_chunks"],
           "max_rel_param_diff_after_warmup": diff, "eager": timed(fns, STEPS)}
    G = capture(fused.step)
    for _ in range(WARM):
        G.replay()
    out["graph"] = timed({"b_fused": G.replay}, STEPS)
    e = out["eager"]
    out["eager_a_over_b_device"] = e["a_torch_loop"]["median_ms"] / e["b_fused"]["median_ms"]
    out["eager_a_over_b_host"] = e["a_torch_loop"]["host_ms_per_call"] / e["b_fused"]["host_ms_per_call"]
    out["eager_a_a2_spread_device"] = abs(e["a_torch_loop"]["median_ms"] / e["a2_torch_loop"]["median_ms"] - 1.0)
    out["eager_a_a2_spread_host"] = abs(e["a_torch_loop"]["host_ms_per_call"] / e["a2_torch_loop"]["host_ms_per_call"] - 1.0)
    out["graph_rate"] = rates(n, out["graph"]["b_fused"]["median_ms"])
    return out, fused


only = os.environ.get("BO_ONLY")
if only:  # profiling runs (rocprofv3 --kernel-trace --stats): one variant alone, eager
    ps = with_grads(gaussian_params() if only == "gaussians" else mani_params(), 3)
    opt = LoopLamb(ps, **HYPER) if only == "a" else mg.FusedLamb(ps, **HYPER)
    for _ in range(STEPS):
        opt.step()
    torch.cuda.synchronize()
    sys.exit(0)

res = {"steps": STEPS, "build_id": _lib.build_id(), "hyper": {k: list(v) if isinstance(v, tuple) else v for k, v in HYPER.items()},
       "note": "device times are hipEvent medians around each call; (a) reads the device twice per tensor, so its events also "
               "span the host's stalls -- which is what a caller waits for.  Rates: 40 B per parameter over the graph-replayed step."}
res["mani"], fused_mani = optimizer_bench(mani_params, "NeuralRenderer: 62 tensors, hidden 512")
assert res["mani"]["tensors"] == 62 and res["mani"]["parameters"] == 5_725_407
res["gaussians"], _ = optimizer_bench(gaussian_params, "100 000 Gaussians as parameters: six tensors, 55 floats per row")

# ---- behind ManiGaussian's own step --------------------------------------------------------------------------------------
P, F, W = 16384, 3, 128
sc0 = syn.make_scene(P, F=F, M=4, seed=0)
g = torch.Generator().manual_seed(1)
sc1 = dict(sc0)
sc1["means3D"] = sc0["means3D"] + 0.02 * torch.randn(P, 3, generator=g)
sc1["rotations"] = sc0["rotations"] + 0.05 * torch.randn(P, 4, generator=g)
KEYS = ("means3D", "opacities", "shs", "language_feature", "scales", "rotations")
d = {k: torch.stack([sc0[k], sc1[k]]).to(dev).requires_grad_(True) for k in KEYS}
plist = [d[k] for k in KEYS]
cams = syn.circle_cameras(4, W, W, negative_focal=True)
batch = GaussianRasterizerBatch([GaussianRasterizationSettings(**syn.camera_settings_kwargs(c, 1, True, device=dev))
                                 for c in (cams[0], cams[2])], view_sets=[0, 1])
gt_rgb = torch.rand(2, W, W, 3, generator=g).to(dev)
gt_embed = torch.randn(1, F, W, W, generator=g).to(dev)


def mani_step():
    c, f, r = batch(d["means3D"], None, d["opacities"], shs=d["shs"], language_feature_precomp=d["language_feature"],
                    scales=d["scales"], rotations=d["rotations"])
    loss, _ = mg.manigaussian_losses(None, None, gt_rgb, gt_embed, None, lambda_embed=0.01, lambda_dyna=0.01,
                                     stacked={"render": c, "render_embed": f})
    return torch.autograd.grad(loss, plist) + (loss.detach(),)


def mani_step_and_optimizer():
    out = mani_step()
    fused_mani.step()
    return out


old = mg.set_forward_mode("async")
try:
    for _ in range(WARM):
        mani_step_and_optimizer()
    torch.cuda.synchronize()
    mg.check_status(dev)
    G = {"step": capture(mani_step), "step_and_fused_lamb": capture(mani_step_and_optimizer), "step_2": capture(mani_step)}
    for _ in range(WARM):
        for gr in G.values():
            gr.replay()
    t = timed({k: gr.replay for k, gr in G.items()}, STEPS)
    mg.check_status(dev)
finally:
    mg.set_forward_mode(old)
res["behind_the_step"] = {"shape": {"P": P, "F": F, "W": W, "sets": 2, "views": 2}, "graph": t,
                          "optimizer_ms_behind_the_step": t["step_and_fused_lamb"]["median_ms"] - t["step"]["median_ms"],
                          "step_step2_spread_ms": abs(t["step"]["median_ms"] - t["step_2"]["median_ms"])}
line = json.dumps(res)
print(line, flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write(json.dumps(res, indent=1) + "\n")
