"""Run in its OWN process by tests/test_fwd_reachable_chunks.py::test_skip_path_replays_bit_identically_from_a_captured_graph
(stream capture is process-wide state; a capture that goes wrong takes the process with it, not the test session).

The scene whose blocks are handed 16 chunks and visit 5 -- the render forward skips its second chunk slot -- forward + backward
through the public autograd API, captured with torch.cuda.graph: the replay reproduces the eager images and radii bit for bit.
Prints GRAPH_OK on success."""
import _graph
import torch

import manigaussian_amd as mg

mg.set_forward_mode("async")  # graph capture needs forwards that never synchronise (opt-in; the default is "safe")
import reachable_chunks_cases as rc
from manigaussian_amd import GaussianRasterizationSettings, GaussianRasterizer
from manigaussian_amd import synthetic as syn

dev = _graph.DEV
F = 32
sc, cam, kw, dC, dF = rc.stack_scene(n=1100, opacity=rc.die_after(300), F=F)
m = rc.chunk_model(rc.oracle_forward(sc, kw)[3])
assert m.n[0] >= 1024 and max(m.block_vis.values()) < 8, (m.n, m.block_vis)
leaves = {k: v.to(dev).requires_grad_(True) for k, v in sc.items()}
rast = GaussianRasterizer(GaussianRasterizationSettings(**syn.camera_settings_kwargs(cam, 1, True, bg=(0.1, 0.2, 0.3), device=dev)))
dC, dF = dC.to(dev), dF.to(dev)
m2 = torch.zeros(sc["means3D"].shape[0], 3, device=dev)


def step():
    c, f, r = rast(leaves["means3D"], m2, leaves["opacities"], shs=leaves["shs"],
                   language_feature_precomp=leaves["language_feature"], scales=leaves["scales"], rotations=leaves["rotations"])
    return (c, f, r) + torch.autograd.grad([c, f], list(leaves.values()), [dC, dF])


graph, out, eager = _graph.captured_step(step, dev, eager=3, replays=2)
mg.check_status(dev)
_graph.same_step(out, eager, 3, "replay vs eager")
_graph.ok()
