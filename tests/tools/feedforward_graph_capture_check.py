"""Run in its OWN process by tests/test_feedforward.py::test_forward_and_backward_captured_into_a_hip_graph (stream capture is
process-wide state; a capture that goes wrong takes the process with it, not the test session).

Forward + backward of PreNorm(64, FeedForward(64)) -- the fused layer norm, two GEMMs and the fused bias-GEGLU, both routed through
the kernels -- captured into ONE graph after two eager warm-up runs, then replayed twice while a new input and a new upstream
gradient are written IN PLACE into the tensors the graph reads.  The fused ops are deterministic and the GEMMs pick their
algorithms in the warm-up, so after every replay the output, the input's gradient and every parameter's gradient equal, bit for
bit, an eager call on the same inputs.  Inside the capture the library is entered exactly four times and no workspace is
allocated (the warm-up's are reused: asserted); a host read of device memory or an allocation inside the library would end the
capture with an error, which fails this script.  The queue settings stay the machine's defaults.  Prints GRAPH_OK on success."""
import _graph
import torch

import feedforward_cases as fc
import manigaussian_amd
from manigaussian_amd import _lib, _ops, feedforward
from numerics import spy

dev = _graph.DEV
feedforward.ROUTE.update(layer_norm=True, bias_geglu=True)


def inputs(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(3, 37, 64, generator=g), torch.randn(3, 37, 64, generator=g)


torch.manual_seed(70)
m = manigaussian_amd.PreNorm(64, manigaussian_amd.FeedForward(64))
with torch.no_grad():
    gen = torch.Generator().manual_seed(71)
    m.norm.weight.copy_(1 + 0.3 * torch.randn(64, generator=gen))
    m.norm.bias.copy_(0.3 * torch.randn(64, generator=gen))
m = m.to(dev)
params = dict(m.named_parameters())
x, g = (t.to(dev) for t in inputs(60))
x.requires_grad_(True)

FUSED = ("mgs_layernorm_forward", "mgs_layernorm_backward", "mgs_bias_geglu_forward", "mgs_bias_geglu_backward")
launches = spy(_lib.lib(), FUSED)


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
launches.clear()
workspaces = dict(_ops._WORKSPACES)
graph, out_graph = _graph.capture(step)
grads_graph = {"x": x.grad, **{k: v.grad for k, v in params.items()}}  # written in place by every replay
assert {k: len(v) for k, v in launches.items()} == dict.fromkeys(FUSED, 1), launches
assert dict(_ops._WORKSPACES) == workspaces, "the capture took no new workspace: the warm-up's are reused"
_graph.stage("captured: the four fused calls, no new workspace")
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
    # the same block in float64 on the CPU, where the drop-ins take torch's own composition
    want_m = manigaussian_amd.PreNorm(64, manigaussian_amd.FeedForward(64))
    want_m.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()}, strict=True)
    want = fc.run_module(want_m, new[0], new[1], torch.float64)
    e_out, e_dx = fc.rel_err(got["out"].cpu(), want[0]), fc.rel_err(got["x"].cpu(), want[1])
    print(f"seed {seed}: out err {e_out:.2e}, dx err {e_dx:.2e} of the float64 composition on the CPU")
    assert e_out <= 1e-4 and e_dx <= 1e-4
    # the graph's own gradient tensors are restored for the next replay
    x.grad = grads_graph["x"]
    for k, v in params.items():
        v.grad = grads_graph[k]
    _graph.stage(f"seed {seed}: the replay equals the eager call bit for bit")
_graph.ok()
