"""Run in its OWN process by tests/test_losses.py::test_render_loss_backward_captured_into_a_hip_graph_follows_targets_and_weights
(stream capture is process-wide state; a capture that goes wrong takes the process with it, not the test session).

ManiGaussian's step through public API -- render_sets_stacked (two sets of 16 384 Gaussians, F = 3) -> manigaussian_losses
with DEVICE-side weights -> backward -- captured with torch.cuda.graph after eager warm-up steps (async forward mode).  The
graph is replayed after the target images and the weights were overwritten in place; the replay must equal the eager step on
the new targets and weights: loss and terms bit for bit (the loss kernels are deterministic and the images are), parameter
gradients to float-atomic order (the rasterizer backward).  Prints GRAPH_OK on success."""
import _graph
import torch

import manigaussian_amd as mg

mg.set_forward_mode("async")  # graph capture needs forwards that never synchronise
from manigaussian_amd import synthetic as syn
from manigaussian_amd.gaussian_renderer import render_sets_stacked

dev = _graph.DEV
P, F, W = 16384, 3, 128
sc = syn.make_scene(P, F=F, M=4, seed=5)
cams = syn.circle_cameras(4, W, W, negative_focal=True)


g = torch.Generator().manual_seed(6)
dxyz, drot = (0.01 * torch.randn(P, 3, generator=g)).to(dev), (0.05 * torch.randn(P, 4, generator=g)).to(dev)
gt_rgb = torch.rand(2, W, W, 3, generator=g).to(dev)       # the stack of both frames' targets, channel-last
gt_embed = torch.randn(1, F, W, W, generator=g).to(dev)    # channel-first
new_rgb, new_embed = torch.rand(2, W, W, 3, generator=g).to(dev), torch.randn(1, F, W, W, generator=g).to(dev)
weights = torch.tensor([[1.0, 0.01], [0.0, 0.0]]).to(dev)  # before the warm-up: lambda_dyna = 0
new_weights = torch.tensor([[1.0, 0.01], [0.01, 0.0]]).to(dev)
leaves = {k: v.to(dev).clone().requires_grad_(True) for k, v in sc.items()}
datas = [_graph.data_of(cams[0], W, dev), _graph.data_of(cams[2], W, dev)]
bg = torch.zeros(3, device=dev)


def step():
    cur = (datas[0], 0, leaves["means3D"], leaves["rotations"], leaves["scales"], leaves["opacities"], None, leaves["shs"],
           leaves["language_feature"])
    nxt = (datas[1], 0, leaves["means3D"] + dxyz, leaves["rotations"] + drot, leaves["scales"].detach(),
           leaves["opacities"].detach(), None, leaves["shs"].detach(), leaves["language_feature"].detach())
    outs, batch = render_sets_stacked([cur, nxt], bg)
    loss, d = mg.manigaussian_losses(outs[0], outs[1], gt_rgb, gt_embed, None, lambda_embed=0.01, lambda_dyna=0.0,
                                     stacked=batch, weights=weights)
    grads = torch.autograd.grad(loss, list(leaves.values()))
    return (loss, d["loss_rgb"], d["loss_embed"], d["loss_dyna"], d["psnr"], batch["render"], batch["render_embed"]) + grads


NV = 7  # values that must replay bit for bit; the rest are parameter gradients
graph, out, eager = _graph.captured_step(step, dev, eager=3, replays=3)
mg.check_status(dev)
_graph.stage("replayed")
_graph.same_step(out, eager, NV, "replay vs eager")
_graph.stage("replays equal the eager step")
with torch.no_grad():  # new targets and the warm-up's end, in place: the graph reads them where they live
    gt_rgb.copy_(new_rgb)
    gt_embed.copy_(new_embed)
    weights.copy_(new_weights)
moved = _graph.replay_follows(graph, out, step, dev, NV, "replay vs eager on the new targets and weights")
assert not torch.equal(moved[0], eager[0]) and eager[3].item() > 0
assert moved[NV].shape == leaves["means3D"].shape
_graph.ok()
