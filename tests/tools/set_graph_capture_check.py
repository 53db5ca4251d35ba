"""Run in its OWN process by tests/test_set_batch.py::test_set_batch_captured_into_a_hip_graph_replays_bit_identically
(stream capture is process-wide state).  ManiGaussian's step shape as a set batch -- two sets of 16 384 Gaussians, one view
each, F = 3 -- forward + backward captured with torch.cuda.graph after two eager steps; replays must reproduce the eager
images bit for bit and the gradients to float-atomic order.  Prints GRAPH_OK on success."""
import _graph
import torch

import manigaussian_amd as mg

mg.set_forward_mode("async")
import util
from manigaussian_amd import GaussianRasterizationSettings, GaussianRasterizerBatch
from manigaussian_amd import synthetic as syn

dev = _graph.DEV
P, F, W = 16384, 3, 128
scs = [util.scene_case(P=P, F=F, seed=2 + 7 * s)[0] for s in range(2)]
leaves = {k: torch.stack([sc[k] for sc in scs]).to(dev).requires_grad_(True) for k in scs[0]}
cams = syn.circle_cameras(4, W, W, negative_focal=True)[:2]
rast = GaussianRasterizerBatch([GaussianRasterizationSettings(**syn.camera_settings_kwargs(c, 1, True, device=dev))
                                for c in cams], view_sets=[0, 1])
g = torch.Generator().manual_seed(4)
dC, dF = torch.randn(2, 3, W, W, generator=g).to(dev), torch.randn(2, F, W, W, generator=g).to(dev)
m2 = torch.zeros(2, P, 3, device=dev)


def step():
    c, f, r = rast(leaves["means3D"], m2, leaves["opacities"], shs=leaves["shs"],
                   language_feature_precomp=leaves["language_feature"], scales=leaves["scales"],
                   rotations=leaves["rotations"])
    return (c, f, r) + torch.autograd.grad([c, f], list(leaves.values()), [dC, dF])


graph, out, eager = _graph.captured_step(step, dev, eager=2, replays=3)
mg.check_status(dev)
for a, b in zip(out[3:], eager[3:]):
    assert a.shape == b.shape and a.shape[0] == 2
_graph.same_step(out, eager, 3, "replay vs eager")
_graph.ok()
