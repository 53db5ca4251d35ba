"""The rendering losses in ManiGaussian's step: torch's chain of small kernels vs the fused pass (manigaussian_amd.losses).
Two Gaussian sets of 16 384 (current frame, deformed next frame), one 128 x 128 view each, SH degree 1, F = 3, negative focal,
rendered in one set-batch call; forward + loss + backward.
  (a)  render + the loss block in torch (this script's restatement of neural_rendering.py:299-329 on the batch outputs:
       l2(rgb), PSNR, cosine(embed), l2(next rgb), the weighted sum) + backward -- what a caller had before
  (b)  render + manigaussian_losses (stacked form) + backward
  (a2) a second copy of (a): the spread of the comparison itself
alternated step by step in one process, hipEvent-timed after warm-up, eager and HIP-graph replayed (async forward mode).
PSNR_torch's `if mse == 0` reads the device: the eager (a) keeps it (it is what the reference runs), the captured (a) cannot and
computes the PSNR without the branch.  Neither variant calls .item() on the logged terms (six more host reads per step in the
reference; the caller's choice here).  Then the loss block alone (forward + backward on leaf images, no render) at V = 2 /
128^2 / F = 3 and V = 8 / 256^2 / F = 32, with the fused pass's achieved memory rate over 3 (3 + F) N V 4 bytes.
Prints one JSON line.  BL_STEPS: timed steps (300).  BL_ONLY=a|b: run that variant's eager step only, untimed (for rocprofv3)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import manigaussian_amd as mg  # noqa: E402
from manigaussian_amd import GaussianRasterizationSettings, GaussianRasterizerBatch, _lib  # noqa: E402
from manigaussian_amd import synthetic as syn  # noqa: E402

STEPS = int(os.environ.get("BL_STEPS", "300"))
WARM = 20
LAMBDA_EMBED, LAMBDA_DYNA = 0.01, 0.01
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


def torch_losses(color, feature, gt_rgb, gt_embed, weights, psnr_branch):
    """neural_rendering.py:299-329 for V views: channel-last views with a batch of 1, l2, PSNR_torch, cosine, `loss +=`."""
    loss, psnr = 0., []
    for v, (w_rgb, w_emb) in enumerate(weights):
        x = color[v:v + 1].permute(0, 2, 3, 1)
        l_rgb = ((x - gt_rgb[v:v + 1]) ** 2).mean()
        if v == 0:  # PSNR_torch (the reference logs it for the current frame)
            mse = torch.mean((x - gt_rgb[v:v + 1]) ** 2)
            if psnr_branch and mse == 0:
                psnr.append(torch.tensor(100.0).to(color.device))
            else:
                psnr.append(20 * torch.log10(1 / torch.sqrt(mse)))
        loss = loss + w_rgb * l_rgb
        if w_emb != 0:
            e = feature[v:v + 1].permute(0, 2, 3, 1)
            loss = loss + w_emb * (1 - torch.nn.functional.cosine_similarity(e, gt_embed[v:v + 1], dim=-1).mean())
    return loss, psnr


# ---- ManiGaussian's step ----------------------------------------------------------------------------------------------
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
gt_rgb = torch.rand(2, W, W, 3, generator=g).to(dev)            # both frames' targets, channel-last
gt_embed_cf = torch.randn(1, F, W, W, generator=g).to(dev)      # channel-first, as the foundation model returns it
gt_embed_cl = gt_embed_cf.permute(0, 2, 3, 1)                   # the reference's view of it
MANI_W = [(1.0, LAMBDA_EMBED), (LAMBDA_DYNA, 0.0)]


def render():
    return batch(d["means3D"], None, d["opacities"], shs=d["shs"], language_feature_precomp=d["language_feature"],
                 scales=d["scales"], rotations=d["rotations"])


def step_a(psnr_branch=True):
    c, f, r = render()
    loss, psnr = torch_losses(c, f, gt_rgb, gt_embed_cl.expand(2, W, W, F), MANI_W, psnr_branch)
    # (detached: a kept loss would keep its autograd graph, and with it the leaves' AccumulateGrad nodes bound to the default
    #  stream, alive into the capture on another stream)
    return torch.autograd.grad(loss, plist) + (loss.detach(),)


def step_b():
    c, f, r = render()
    loss, terms = mg.manigaussian_losses(None, None, gt_rgb, gt_embed_cf, None, lambda_embed=LAMBDA_EMBED,
                                         lambda_dyna=LAMBDA_DYNA, stacked={"render": c, "render_embed": f})
    return torch.autograd.grad(loss, plist) + (loss.detach(),)


only = os.environ.get("BL_ONLY")
if only:  # profiling runs (rocprofv3 --kernel-trace --stats): one variant alone, eager, default forward mode
    fn = {"a": step_a, "b": step_b}[only]
    for _ in range(STEPS):
        fn()
    torch.cuda.synchronize()
    sys.exit(0)

res = {"shape": {"P": P, "F": F, "W": W, "sets": 2, "views": 2}, "steps": STEPS, "build_id": _lib.build_id(),
       "note": "graph (a) computes the PSNR without PSNR_torch's `if mse == 0` (a device read cannot be captured); eager (a) "
               "keeps it.  No variant calls .item() on the logged terms."}
old = mg.set_forward_mode("async")
try:
    for _ in range(WARM):
        step_a()
        step_b()
    torch.cuda.synchronize()
    mg.check_status(dev)
    (*ga, la), (*gb, lb) = step_a(), step_b()
    res["loss_a"], res["loss_b"] = la.item(), lb.item()
    res["max_rel_grad_diff"] = max(((x - y).abs().max() / y.abs().max().clamp_min(1e-30)).item() for x, y in zip(gb, ga))
    a_graph = lambda: step_a(False)  # noqa: E731
    G = {"a_torch_losses": capture(a_graph), "b_fused_losses": capture(step_b), "a2_torch_losses": capture(a_graph)}
    for _ in range(WARM):
        for gr in G.values():
            gr.replay()
    res["graph"] = timed({k: gr.replay for k, gr in G.items()}, STEPS)
    mg.check_status(dev)
    res["eager"] = timed({"a_torch_losses": step_a, "b_fused_losses": step_b, "a2_torch_losses": step_a}, STEPS)
    mg.check_status(dev)
finally:
    mg.set_forward_mode(old)
for mode in ("graph", "eager"):
    t = res[mode]
    res[mode + "_a_over_b"] = t["a_torch_losses"]["median_ms"] / t["b_fused_losses"]["median_ms"]
    res[mode + "_a_a2_spread"] = abs(t["a_torch_losses"]["median_ms"] / t["a2_torch_losses"]["median_ms"] - 1.0)


# ---- the loss block alone -------------------------------------------------------------------------------------------------
def block(V, H, Fb):
    gg = torch.Generator().manual_seed(3)
    color = torch.rand(V, 3, H, H, generator=gg).to(dev).requires_grad_(True)
    feat = torch.randn(V, Fb, H, H, generator=gg)
    feat = (feat * (torch.rand(V, 1, H, H, generator=gg) >= 0.3)).to(dev).requires_grad_(True)
    t_rgb, t_emb = torch.rand(V, H, H, 3, generator=gg).to(dev), torch.randn(V, H, H, Fb, generator=gg).to(dev)
    w = MANI_W if V == 2 else [(1.0, LAMBDA_EMBED)] * V

    def a():
        loss, _ = torch_losses(color, feat, t_rgb, t_emb, w, False)
        return torch.autograd.grad(loss, [color, feat])

    def b():
        loss, _ = mg.rendering_loss(color, t_rgb, feat, t_emb, weights=w)
        return torch.autograd.grad(loss, [color, feat])

    for _ in range(WARM):
        a()
        b()
    torch.cuda.synchronize()
    G = {"a_torch": capture(a), "b_fused": capture(b)}
    for _ in range(WARM):
        for gr in G.values():
            gr.replay()
    out = {"V": V, "H": H, "W": H, "F": Fb, "graph": timed({k: gr.replay for k, gr in G.items()}, STEPS),
           "eager": timed({"a_torch": a, "b_fused": b}, STEPS)}
    nbytes = 3 * (3 + Fb) * H * H * V * 4
    out["fused_bytes"] = nbytes
    out["fused_graph_GBps"] = nbytes / (out["graph"]["b_fused"]["median_ms"] * 1e-3) / 1e9
    return out


res["loss_block"] = [block(2, 128, 3), block(8, 256, 32)]
res["loss_block_note"] = ("fused_graph_GBps = 3 (3 + F) N V 4 bytes over the graph-replayed forward + backward (3 launches); at "
                          "V = 2 / 128^2 / F = 3 the pass is launch latency, not bandwidth")
print(json.dumps(res), flush=True)
