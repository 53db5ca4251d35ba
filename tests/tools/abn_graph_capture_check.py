"""Run in its OWN process by tests/test_encoder.py::test_forward_and_backward_captured_into_a_hip_graph (stream capture is
process-wide state; a capture that goes wrong takes the process with it, not the test session).

One forward + backward of batch_norm_act (training mode, with the skip tensor) captured into ONE graph after two eager warm-up
runs, then replayed twice.  The kernels are deterministic, so after the k-th replay y, dx, dweight, dbias, the two running buffers and
num_batches_tracked equal, bit for bit, the k-th of two eager calls that started from the same buffers: the running buffers and the
counter advance once per replay, by the launch itself.  An aligned cube (rows split into several sub-slices) and an odd, batched
volume (scalar heads and tails).  The queue settings stay the machine's defaults.  Prints GRAPH_OK on success."""
import _graph
import torch

import abn_cases as ac
from manigaussian_amd import batch_norm_act

dev = _graph.DEV
NAMES = ("y", "dx", "dweight", "dbias", "running_mean", "running_var", "num_batches_tracked")

for shape in ((1, 8, 40, 40, 40), (2, 3, 21, 19, 23)):
    C = shape[1]
    gen = torch.Generator().manual_seed(60)
    x, res, g = (torch.randn(*shape, generator=gen).to(dev) for _ in range(3))
    w = (1.0 + 0.5 * torch.randn(C, generator=gen)).to(dev).requires_grad_(True)
    b = (0.3 * torch.randn(C, generator=gen)).to(dev).requires_grad_(True)
    x.requires_grad_(True)
    rm, rv, nbt = torch.zeros(C, device=dev), torch.ones(C, device=dev), torch.zeros((), dtype=torch.int64, device=dev)

    def reset():
        with torch.no_grad():
            rm.zero_()
            rv.fill_(1.0)
            nbt.zero_()
        x.grad = w.grad = b.grad = None

    def step():
        y = batch_norm_act(x, w, b, rm, rv, nbt, training=True, momentum=ac.MOMENTUM, eps=ac.EPS, residual=res)
        y.backward(g)
        return y

    def snapshot(y):
        return [t.detach().clone() for t in (y, x.grad, w.grad, b.grad, rm, rv, nbt)]

    _graph.warm_up(step, before_each=reset)
    _graph.stage(f"{shape}: warm-up done")

    reset()
    eager = []
    for _ in range(2):
        x.grad = w.grad = b.grad = None
        eager.append(snapshot(step()))
    torch.cuda.synchronize()
    assert int(eager[0][6]) == 1 and int(eager[1][6]) == 2
    assert not torch.equal(eager[0][4], eager[1][4]), "the running mean did not move between two eager steps"

    reset()
    graph, out_y = _graph.capture(step)
    assert int(nbt) == 0 and not bool(rm.any()), "the capture itself ran the kernels"
    _graph.stage(f"{shape}: captured")
    # (x.grad, w.grad, b.grad were None at capture: the backward's own output tensors; no NaN fill: the running buffers and the
    #  counter are read before they are written.  num_batches_tracked after replay k is the k-th eager call's: k, asserted above)
    _graph.replays_equal(graph, lambda: snapshot(out_y), lambda k: eager[k - 1], NAMES, shape, poison=False)
    _graph.stage(f"{shape}: two replays equal two eager calls bit for bit; the buffers advanced once per replay")
_graph.ok()
