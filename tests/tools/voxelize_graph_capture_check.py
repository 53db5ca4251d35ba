"""Run in its OWN process by tests/test_voxelizer.py::test_voxelize_then_point_latent_captured_into_a_hip_graph (stream capture
is process-wide state; a capture that goes wrong takes the process with it, not the test session).

voxelize -> point_latent_pe (the grid, permuted as the agent permutes it, read back by the fused trilinear gather) captured
into ONE graph after eager warm-up, then replayed while new clouds, colours and bounds are written IN PLACE into the tensors
the graph reads.  The voxelizer is deterministic, so after every replay the grid equals, bit for bit, both an eager call on the
same inputs and the CPU restatement; the gathered latents equal the eager ones bit for bit as well (a gather adds nothing).
Both memory layouts.  Prints GRAPH_OK on success."""
import _graph
import torch

import voxelize_cases as vc
from manigaussian_amd import point_latent_pe
from manigaussian_amd.voxelizer import voxelize

dev = _graph.DEV
B, N, V, P = 1, 16384, 100, 4096


def inputs(seed):
    coords, feats, bounds, _ = vc.make_inputs(B=B, N=N, V=V, Fc=3, kind="depth", bounds="scene", seed=seed)
    bounds = bounds + 0.01 * (seed % 3) * torch.tensor([1.0, -1.0, 0.5, -1.0, 1.0, -0.5])
    return coords, feats, bounds


g = torch.Generator().manual_seed(7)
lo, hi = torch.tensor(vc.SCENE_BOUNDS[:3]), torch.tensor(vc.SCENE_BOUNDS[3:])
query = (lo + (hi - lo) * torch.rand(P, 3, generator=g)).to(dev)

for memory in ("channels_first", "channels_last"):
    first = inputs(100)
    coords, feats, bounds = (t.to(dev).clone() for t in first)

    def step():
        vox = voxelize(coords, feats, bounds, V, memory)
        return vox, point_latent_pe(vox.permute(0, 4, 1, 2, 3), query, vc.SCENE_BOUNDS)

    _graph.warm_up(step)
    _graph.stage(f"{memory}: warm-up done")
    graph, (out_vox, out_lat) = _graph.capture(step)
    _graph.stage(f"{memory}: captured")
    for seed in (100, 101, 102, 103):
        new = inputs(seed)
        for dst, src in zip((coords, feats, bounds), new):
            dst.copy_(src.to(dev))
        _graph.replay(graph)
        got_vox, got_lat = out_vox.clone(), out_lat.clone()
        eager_vox, eager_lat = step()
        torch.cuda.synchronize()
        exp = vc.restate(*new, V)
        n = int((vc.bits(got_vox.cpu()) != vc.bits(exp)).sum())
        print(f"{memory} seed {seed}: {n} floats of the replayed grid differ from the restatement, occupied {int(exp[..., -1].sum())}")
        assert n == 0
        _graph.equal_bits((got_vox, got_lat), (eager_vox, eager_lat), ("the replayed grid", "the replayed latents"), f"{memory} seed {seed}")
    _graph.stage(f"{memory}: replays equal the eager calls and the restatement, bit for bit")
_graph.ok()
