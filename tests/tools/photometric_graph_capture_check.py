"""Run in its OWN process by
tests/test_photometric.py::test_render_photometric_loss_backward_captured_into_a_hip_graph_follows_targets_and_weights
(stream capture is process-wide state; a capture that goes wrong takes the process with it, not the test session).

render_sets_stacked (two sets of 16 384 Gaussians, F = 3) -> photometric_loss on the batch's colour images with DEVICE-side
weights -> backward -- captured with torch.cuda.graph after eager warm-up steps (async forward mode).  The graph is replayed
after the target images and the weights were overwritten in place; the replay must equal the eager step on the new targets
and weights: loss and terms bit for bit (the loss kernels are deterministic and the images are), parameter gradients to
float-atomic order (the rasterizer backward).  Prints GRAPH_OK on success."""
import faulthandler
import os
import sys

faulthandler.enable()
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import manigaussian_amd as mg  # noqa: E402

mg.set_forward_mode("async")  # graph capture needs forwards that never synchronise
from manigaussian_amd import synthetic as syn  # noqa: E402
from manigaussian_amd.gaussian_renderer import render_sets_stacked  # noqa: E402

dev = torch.device("cuda:0")
P, F, W = 16384, 3, 128
sc = syn.make_scene(P, F=F, M=4, seed=5)
cams = syn.circle_cameras(4, W, W, negative_focal=True)


def data_of(cam):
    kw = syn.camera_settings_kwargs(cam, 1, True, device=dev)
    return {"novel_view": {"tanfov_host": [(kw["tanfovx"], kw["tanfovy"])], "size_host": [(W, W)],
                           "world_view_transform": kw["viewmatrix"][None], "full_proj_transform": kw["projmatrix"][None],
                           "camera_center": kw["campos"][None]}}


g = torch.Generator().manual_seed(6)
dxyz, drot = (0.01 * torch.randn(P, 3, generator=g)).to(dev), (0.05 * torch.randn(P, 4, generator=g)).to(dev)
gt_rgb = torch.rand(2, W, W, 3, generator=g).to(dev)  # both frames' targets, channel-last
new_rgb = torch.rand(2, W, W, 3, generator=g).to(dev)
weights = torch.tensor([[1.0, 0.0, 0.2], [0.0, 0.0, 0.0]]).to(dev)  # before the warm-up: nothing on the next frame
new_weights = torch.tensor([[0.8, 0.1, 0.2], [0.01, 0.0, 0.05]]).to(dev)
leaves = {k: v.to(dev).clone().requires_grad_(True) for k, v in sc.items()}
datas = [data_of(cams[0]), data_of(cams[2])]
bg = torch.zeros(3, device=dev)


def step():
    cur = (datas[0], 0, leaves["means3D"], leaves["rotations"], leaves["scales"], leaves["opacities"], None, leaves["shs"],
           leaves["language_feature"])
    nxt = (datas[1], 0, leaves["means3D"] + dxyz, leaves["rotations"] + drot, leaves["scales"].detach(),
           leaves["opacities"].detach(), None, leaves["shs"].detach(), leaves["language_feature"].detach())
    outs, batch = render_sets_stacked([cur, nxt], bg)
    loss, t = mg.photometric_loss(batch["render"], gt_rgb, weights=weights)
    grads = torch.autograd.grad(loss, list(leaves.values()), allow_unused=True)
    grads = tuple(x for x in grads if x is not None)
    return (loss, t["l1"], t["l2"], t["ssim"], t["psnr"], batch["render"]) + grads


def stage(msg):
    print("stage:", msg, flush=True)


NV = 6  # values that must replay bit for bit; the rest are parameter gradients
for _ in range(3):
    eager = [t.detach().clone() for t in step()]
    mg.check_status(dev)
stage("eager steps done")
side = torch.cuda.Stream()
side.wait_stream(torch.cuda.current_stream())
with torch.cuda.stream(side):
    step()
torch.cuda.current_stream().wait_stream(side)
torch.cuda.synchronize()
stage("side-stream warm-up done")
graph = torch.cuda.CUDAGraph()
with torch.cuda.graph(graph):
    out = step()
stage("captured")
for _ in range(3):
    graph.replay()
torch.cuda.synchronize()
mg.check_status(dev)
stage("replayed")


def same(got, want, what):
    assert len(got) == len(want) and len(got) > NV
    for i, (a, b) in enumerate(zip(got[:NV], want[:NV])):
        assert torch.equal(a, b), f"{what}: value {i} differs"
    for a, b in zip(got[NV:], want[NV:]):
        assert (a - b).abs().max().item() <= 2e-5 * b.abs().max().item() + 1e-12, f"{what}: gradients differ"


same(out, eager, "replay vs eager")
stage("replays equal the eager step")
with torch.no_grad():  # new targets and weights, in place: the graph reads them where they live
    gt_rgb.copy_(new_rgb)
    weights.copy_(new_weights)
torch.cuda.synchronize()
graph.replay()
torch.cuda.synchronize()
replayed = [t.detach().clone() for t in out]
moved = [t.detach().clone() for t in step()]
torch.cuda.synchronize()
mg.check_status(dev)
same(replayed, moved, "replay vs eager on the new targets and weights")
assert not torch.equal(moved[0], eager[0]) and not torch.equal(moved[NV], eager[NV])
assert moved[NV].shape == leaves["means3D"].shape
print("GRAPH_OK")
