"""Run in its OWN process by tests/test_attention.py::test_forward_and_backward_captured_into_a_hip_graph (stream capture is
process-wide state; a capture that goes wrong takes the process with it, not the test session).

Forward + backward of a training-mode Attention with dropout 0.1 captured into ONE graph after two eager warm-up runs, then
replayed three times back to back with no host synchronisation in between.  The kernels read (seed, offset) from the module's
device buffer and the captured in-place add advances the offset, so every replay draws a fresh mask: consecutive outputs
differ, the offsets the replays saw are consecutive, and each replay's output and gradients equal, bit for bit, the eager
kernels run on the state that replay saw -- and, within rounding, plain torch ops with that replay's keep mask
(mgs_attention_dropout_mask).  The queue settings stay the machine's defaults.  Prints GRAPH_OK on success."""
import _graph
import torch

import attention_cases as ac
from manigaussian_amd import Attention
from manigaussian_amd.attention import dropout_keep_mask, fused_attention_kv

dev = _graph.DEV
B, H, Nq, Nk, P = 2, 2, 150, 200, 0.1

torch.manual_seed(3)
m = Attention(16, context_dim=24, heads=H, dropout=P).to(dev).train()
m.manual_seed(0x5DEECE66D, 0xFFFFFFFE)  # the offset crosses 2^32 during the replays
x = torch.randn(B, Nq, 16, device=dev, requires_grad=True)
context = torch.randn(B, Nk, 24, device=dev, requires_grad=True)
g = torch.randn(B, Nq, 16, device=dev)
leaves = [x, context] + list(m.parameters())


def step():
    out = m(x, context=context)
    out.backward(g)
    return out


_graph.warm_up(step)
_graph.stage("warm-up done")
for t in leaves:
    t.grad = None
graph, out = _graph.capture(step)
_graph.stage("captured")
seen = []
for r in range(3):
    state = m.rng_state.clone()
    graph.replay()
    seen.append((state, out.detach().clone(), [t.grad.clone() for t in leaves]))
torch.cuda.synchronize()
_graph.stage("three replays, one synchronise")

for r, (state, got, grads) in enumerate(seen):
    assert int(state[1]) == 0xFFFFFFFE + 2 + r, (r, state.tolist())  # two warm-up runs, then one per replay
    # the eager kernels on the state this replay saw
    q, kv = m.to_q(x), m.to_kv(context)
    eager = m.to_out(fused_attention_kv(q, kv, H, dropout_p=P, rng_state=state))
    for t in leaves:
        t.grad = None
    eager.backward(g)
    _graph.equal_bits([got] + grads, [eager] + [t.grad for t in leaves], ["the output"] + ["a gradient"] * len(leaves), f"replay {r}")
    # plain torch ops with this replay's keep mask
    keep = dropout_keep_mask(B, H, Nq, Nk, P, state)
    assert int((keep.cpu().numpy().astype(bool) != ac.keep_mask(int(state[0]), int(state[1]), B * H, Nq, Nk, P)).sum()) == 0
    k, v = (t.reshape(B, Nk, H, 64).transpose(1, 2) for t in kv.chunk(2, dim=-1))
    attn = (torch.einsum("bhid,bhjd->bhij", q.reshape(B, Nq, H, 64).transpose(1, 2), k) * 64 ** -0.5).softmax(dim=-1)
    attn = attn * keep.reshape(B, H, Nq, Nk).float() / (1 - P)
    dense = m.to_out(torch.einsum("bhij,bhjd->bhid", attn, v).transpose(1, 2).reshape(B, Nq, H * 64))
    err = (dense - got).abs().max().item()
    print(f"replay {r}: offset {int(state[1])}, kept {float(keep.float().mean()):.4f}, |dense - replay| {err:.2e}")
    assert err <= 1e-5 * dense.abs().max().item(), err
    if r:
        assert not ac.same_bits(got.cpu(), seen[r - 1][1].cpu()), "two consecutive replays drew the same mask"
        d = (got - seen[r - 1][1]).abs().max().item()
        assert d > 1e-3 * got.abs().max().item(), d
_graph.stage("every replay equals the eager call on its own state and differs from its predecessor")
_graph.ok()
