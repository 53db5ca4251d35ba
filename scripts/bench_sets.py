"""Set batch vs per-render calls at ManiGaussian's step shape: the current frame and the deformed next frame (two Gaussian sets
of 16 384, one 128 x 128 view each, SH degree 1, F = 3, negative focal), fwd + bwd.
  (a) two GaussianRasterizer calls + backward (today's step)
  (b) one GaussianRasterizerBatch call on the stacked sets + backward (the caller's torch.stack included)
both HIP-graph captured (async forward mode, as bench.py's headline) and eager, alternated in one process, hipEvent-timed after
warm-up; plus BASELINE configs[3]'s rendering part (100 000 Gaussians, F = 32, 4 sets x 4 views): one set call vs four
view-batch calls (eager).  Prints one JSON line.  BS_STEPS: timed steps (300); BS_ONLY_B=1: run step (b) only, untimed (for
rocprofv3)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import manigaussian_amd as mg  # noqa: E402
from manigaussian_amd import GaussianRasterizationSettings, GaussianRasterizer, GaussianRasterizerBatch, _lib  # noqa: E402
from manigaussian_amd import synthetic as syn  # noqa: E402

STEPS = int(os.environ.get("BS_STEPS", "300"))
WARM = 20
dev = torch.device("cuda:0")
torch.autograd.set_multithreading_enabled(False)


def settings_of(cams, F):
    return [GaussianRasterizationSettings(**syn.camera_settings_kwargs(c, 1, True, device=dev)) for c in cams]


def timed(fns, steps):
    """Alternate the step functions; ms per step of each by hipEvents around every call."""
    ev = {k: [] for k in fns}
    for _ in range(steps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            ev[k].append((e0, e1))
    torch.cuda.synchronize()
    out = {}
    for k, lst in ev.items():
        t = sorted(a.elapsed_time(b) for a, b in lst)
        out[k] = {"median_ms": t[len(t) // 2], "mean_ms": sum(t) / len(t)}
    return out


# ---- ManiGaussian's step ----------------------------------------------------------------------------------------------
P, F, W = 16384, 3, 128
sc0 = syn.make_scene(P, F=F, M=4, seed=0)
g = torch.Generator().manual_seed(1)
sc1 = dict(sc0)
sc1["means3D"] = sc0["means3D"] + 0.02 * torch.randn(P, 3, generator=g)
sc1["rotations"] = sc0["rotations"] + 0.05 * torch.randn(P, 4, generator=g)
d = [{k: v.to(dev).clone().requires_grad_(True) for k, v in sc.items()} for sc in (sc0, sc1)]
cams = syn.circle_cameras(4, W, W, negative_focal=True)
sets = settings_of([cams[0], cams[2]], F)
dC, dF = torch.randn(2, 3, W, W, generator=g).to(dev), torch.randn(2, F, W, W, generator=g).to(dev)
singles = [GaussianRasterizer(s) for s in sets]
batch = GaussianRasterizerBatch(sets, view_sets=[0, 1])
KEYS = ("means3D", "opacities", "shs", "language_feature", "scales", "rotations")
plist = [d[s][k] for s in range(2) for k in KEYS]


def step_a():
    outs, grads = [], []
    for s in range(2):
        c, f, r = singles[s](d[s]["means3D"], torch.zeros(0), d[s]["opacities"], shs=d[s]["shs"],
                             language_feature_precomp=d[s]["language_feature"], scales=d[s]["scales"],
                             rotations=d[s]["rotations"])
        outs += [c, f]
        grads += list(torch.autograd.grad([c, f], [d[s][k] for k in KEYS], [dC[s], dF[s]]))
    return outs, grads


def step_b():
    st = {k: torch.stack([d[0][k], d[1][k]]) for k in KEYS}
    c, f, r = batch(st["means3D"], None, st["opacities"], shs=st["shs"], language_feature_precomp=st["language_feature"],
                    scales=st["scales"], rotations=st["rotations"])
    gs = torch.autograd.grad([c, f], plist, [dC, dF])
    return [c[0], f[0], c[1], f[1]], [gs[s * len(KEYS) + i] for s in range(2) for i in range(len(KEYS))]


def max_diff():
    oa, ga = step_a()
    ob, gb = step_b()
    torch.cuda.synchronize()
    img = max((a - b).abs().max().item() for a, b in zip(oa, ob))
    grad = max(((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item() for a, b in zip(ga, gb))
    return img, grad


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


if os.environ.get("BS_ONLY_B"):  # profiling runs (rocprofv3 --kernel-trace --stats): the one-call step (b) alone, eager
    for _ in range(STEPS):
        step_b()
    torch.cuda.synchronize()
    sys.exit(0)
res = {"shape": {"P": P, "F": F, "W": W, "sets": 2, "views": 2}, "steps": STEPS, "build_id": _lib.build_id()}
old = mg.set_forward_mode("async")
try:
    for _ in range(WARM):
        step_a()
        step_b()
    torch.cuda.synchronize()
    mg.check_status(dev)
    res["max_abs_image_diff"], res["max_rel_grad_diff"] = max_diff()
    ga, gb = capture(step_a), capture(step_b)
    for _ in range(WARM):
        ga.replay()
        gb.replay()
    t = timed({"a_two_calls": ga.replay, "b_one_set_call": gb.replay}, STEPS)
    mg.check_status(dev)
    res["graph"] = t
    t = timed({"a_two_calls": step_a, "b_one_set_call": step_b}, STEPS)
    mg.check_status(dev)
    res["eager"] = t
finally:
    mg.set_forward_mode(old)

# ---- BASELINE configs[3]'s rendering part: 4 timesteps (sets) x 4 views of 100 000 Gaussians, F = 32 -------------------
P3, F3, S3, V3 = 100000, 32, 4, 4
scs = [syn.make_scene(P3, F=F3, M=4, seed=10 + s) for s in range(S3)]
d3 = {k: torch.stack([sc[k] for sc in scs]).to(dev).requires_grad_(True) for k in KEYS}
cams3 = syn.circle_cameras(V3, W, W, negative_focal=True)
sets3 = settings_of(cams3, F3)
dC3, dF3 = torch.randn(S3 * V3, 3, W, W, generator=g).to(dev), torch.randn(S3 * V3, F3, W, W, generator=g).to(dev)
one = GaussianRasterizerBatch(sets3 * S3, view_sets=[s for s in range(S3) for _ in range(V3)])
per = GaussianRasterizerBatch(sets3)
p3 = [d3[k] for k in KEYS]


def c3_one():
    c, f, r = one(d3["means3D"], None, d3["opacities"], shs=d3["shs"], language_feature_precomp=d3["language_feature"],
                  scales=d3["scales"], rotations=d3["rotations"])
    return torch.autograd.grad([c, f], p3, [dC3, dF3])


def c3_four():
    out = []
    for s in range(S3):
        c, f, r = per(d3["means3D"][s], None, d3["opacities"][s], shs=d3["shs"][s],
                      language_feature_precomp=d3["language_feature"][s], scales=d3["scales"][s],
                      rotations=d3["rotations"][s])
        out.append(torch.autograd.grad([c, f], p3, [dC3[s * V3:(s + 1) * V3], dF3[s * V3:(s + 1) * V3]]))
    return out


for _ in range(5):
    c3_one()
    c3_four()
torch.cuda.synchronize()
res["configs3_eager"] = timed({"four_view_batch_calls": c3_four, "one_set_call": c3_one}, max(STEPS // 3, 50))
res["graph_speedup_b_over_a"] = res["graph"]["a_two_calls"]["median_ms"] / res["graph"]["b_one_set_call"]["median_ms"]
print(json.dumps(res), flush=True)
