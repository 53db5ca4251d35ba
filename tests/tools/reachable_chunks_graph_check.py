"""Run in its OWN process by tests/test_fwd_reachable_chunks.py::test_skip_path_replays_bit_identically_from_a_captured_graph
(stream capture is process-wide state; a capture that goes wrong takes the process with it, not the test session).

The scene whose blocks are handed 16 chunks and visit 5 -- the render forward skips its second chunk slot -- forward + backward
through the public autograd API, captured with torch.cuda.graph: the replay reproduces the eager images and radii bit for bit.
Prints GRAPH_OK on success."""
import faulthandler
import os
import sys

faulthandler.enable()
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import manigaussian_amd as mg  # noqa: E402

mg.set_forward_mode("async")  # graph capture needs forwards that never synchronise (opt-in; the default is "safe")
import reachable_chunks_cases as rc  # noqa: E402
from manigaussian_amd import GaussianRasterizationSettings, GaussianRasterizer  # noqa: E402
from manigaussian_amd import synthetic as syn  # noqa: E402

dev = torch.device("cuda:0")
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


for _ in range(3):
    # (detached copies: a kept output would keep its autograd graph alive into the capture)
    eager = [t.detach().clone() for t in step()]
    mg.check_status(dev)
side = torch.cuda.Stream()
side.wait_stream(torch.cuda.current_stream())
with torch.cuda.stream(side):
    step()  # warm-up on a side stream, as torch's capture recipe asks
torch.cuda.current_stream().wait_stream(side)
torch.cuda.synchronize()
graph = torch.cuda.CUDAGraph()
with torch.cuda.graph(graph):
    out = step()
for _ in range(2):
    graph.replay()
torch.cuda.synchronize()
mg.check_status(dev)
assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1]) and torch.equal(out[2], eager[2]), "images differ"
for a, b in zip(out[3:], eager[3:]):
    assert (a - b).abs().max().item() <= 2e-5 * b.abs().max().item() + 1e-12, "gradients differ"
print("GRAPH_OK")
