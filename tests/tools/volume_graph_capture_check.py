"""Run in its OWN process by tests/test_volume.py::test_forward_and_backward_captured_into_a_hip_graph (stream capture is
process-wide state; a capture that goes wrong takes the process with it, not the test session).

Forward + backward of the Conv3DUpsampleBlock drop-in (strides 2, small) captured into ONE graph after two eager warm-up runs, then
replayed twice while a new input and a new upstream gradient are written IN PLACE into the tensors the graph reads.  The fused
op is deterministic, and MIOpen picks its convolution algorithms in the warm-up, so after every replay the output, the input's
gradient and every parameter's gradient equal, bit for bit, an eager call on the same inputs.  The queue settings stay the
machine's defaults.  Prints GRAPH_OK on success."""
import _graph
import torch

import volume_cases as vc
import manigaussian_amd

dev = _graph.DEV
NAME = "up_s2_k3"


def inputs(seed):
    f = vc.load_module_fixture(NAME)
    g = torch.Generator().manual_seed(seed)
    return torch.randn(f["x"].shape, generator=g), torch.randn(f["g"].shape, generator=g)


m = vc.fixture_module(manigaussian_amd, NAME).to(dev)
params = dict(m.named_parameters())
x, g = (t.to(dev) for t in inputs(60))
x.requires_grad_(True)


def step():
    out = m(x)
    out.backward(g)
    return out


def clear():
    x.grad = None
    m.zero_grad(set_to_none=True)


_graph.warm_up(step)
_graph.stage("warm-up done")
clear()
graph, out_graph = _graph.capture(step)
grads_graph = {"x": x.grad, **{k: v.grad for k, v in params.items()}}  # written in place by every replay
_graph.stage("captured")
for seed in (61, 62):
    new = inputs(seed)
    with torch.no_grad():
        x.copy_(new[0].to(dev))
        g.copy_(new[1].to(dev))
    _graph.replay(graph)
    got = {"out": out_graph.detach().clone(), **{k: v.clone() for k, v in grads_graph.items()}}
    clear()
    out = step()
    torch.cuda.synchronize()
    eager = {"out": out.detach(), "x": x.grad, **{k: v.grad for k, v in params.items()}}
    _graph.equal_bits(got.values(), [eager[k] for k in got], [f"the replayed {k}" for k in got], f"seed {seed}")
    want = vc.run_module(vc.fixture_module(vc.plain, NAME), new[0], new[1], torch.float64)
    e_out, e_dx = vc.rel_err(got["out"].cpu(), want[0]), vc.rel_err(got["x"].cpu(), want[1])
    print(f"seed {seed}: out err {e_out:.2e}, dx err {e_dx:.2e} of the float64 layers on the CPU")
    assert e_out <= 1e-4 and e_dx <= 1e-4
    # the graph's own gradient tensors are restored for the next replay
    x.grad = grads_graph["x"]
    for k, v in params.items():
        v.grad = grads_graph[k]
    _graph.stage(f"seed {seed}: the replay equals the eager call bit for bit")
_graph.ok()
