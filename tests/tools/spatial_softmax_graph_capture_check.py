"""Run in its OWN process by tests/test_spatial_softmax.py::test_forward_and_backward_captured_into_a_hip_graph (stream capture is
process-wide state; a capture that goes wrong takes the process with it, not the test session).

forward_with_max + backward of SpatialSoftmax3D captured into ONE graph after two eager warm-up runs, then replayed while new
volumes and upstream gradients are written IN PLACE into the tensors the graph reads.  The kernels are deterministic, so after
every replay keypoints, maxpool and the volume's gradient equal, bit for bit, an eager call on the same inputs, and lie within
the fixture bounds' yardstick of the float64 restatement.  An aligned cube (rows split in several slices) and an odd, non-cube
volume (scalar heads and tails).  The queue settings stay the machine's defaults.  Prints GRAPH_OK on success."""
import _graph
import torch

import spatial_softmax_cases as sc
from manigaussian_amd import SpatialSoftmax3D

dev = _graph.DEV
T = sc.TEMPERATURE


def inputs(shape, seed):
    B, C = shape[:2]
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * 0.1 + 0.01 * seed, torch.randn(B, 3 * C, generator=g), torch.randn(B, C, generator=g))


for shape in ((1, 8, 40, 40, 40), (2, 3, 21, 19, 23)):
    B, C, D, H, W = shape
    m = SpatialSoftmax3D(D, H, W, C).to(dev)
    x, g_k, g_m = (t.to(dev).clone() for t in inputs(shape, 50))
    x.requires_grad_(True)

    def step():
        kp, mx = m.forward_with_max(x)
        ((kp * g_k).sum() + (mx * g_m).sum()).backward()
        return kp, mx

    _graph.warm_up(step)
    _graph.stage(f"{shape}: warm-up done")
    x.grad = None
    graph, (out_kp, out_mx) = _graph.capture(step)
    out_dx = x.grad  # written in place by every replay (x.grad was None at capture: the backward's own output tensor)
    _graph.stage(f"{shape}: captured")
    for seed in (50, 51, 52, 53):
        new = inputs(shape, seed)
        with torch.no_grad():
            for dst, src in zip((x, g_k, g_m), new):
                dst.copy_(src.to(dev))
        _graph.replay(graph)
        got = (out_kp.detach().clone(), out_mx.detach().clone(), out_dx.clone())
        x.grad = None
        kp, mx = step()
        torch.cuda.synchronize()
        eager = (kp.detach(), mx.detach(), x.grad.clone())
        _graph.equal_bits(got, eager, ("the replayed keypoints", "the replayed maxpool", "the replayed dx"), f"{shape} seed {seed}")
        xx = new[0].double().requires_grad_(True)
        kp64, mx64 = sc.restatement(xx, D, H, W, T, torch.float64)
        ((kp64 * new[1].double()).sum() + (mx64 * new[2].double()).sum()).backward()
        e_kp = (got[0].cpu().double() - kp64.detach()).abs().max().item()
        e_dx = (got[2].cpu().double() - xx.grad).abs().max().item() / xx.grad.abs().max().item()
        print(f"{shape} seed {seed}: keypoints err {e_kp:.2e}, dx err {e_dx:.2e} of max|dx|")
        assert torch.equal(got[1].cpu().double(), mx64.detach()) and e_kp <= 1e-5 and e_dx <= 1e-4
    _graph.stage(f"{shape}: replays equal the eager calls bit for bit")
_graph.ok()
