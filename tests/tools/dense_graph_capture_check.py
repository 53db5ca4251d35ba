"""Run in its OWN process by tests/test_dense_conv.py::test_forward_and_backward_captured_into_a_hip_graph (stream capture is
process-wide state; a capture that goes wrong takes the process with it, not the test session).

One forward + backward of dense_conv3d at the `odd_k3` case (a batch, odd rows, a partial N-tile, leaky ReLU) and one at
`up0_last_head` (a site's channels, k = 5), each captured into ONE graph on a single stream after two eager warm-up runs, then
replayed twice.  The kernels are deterministic and keep no state, so after every replay y, dx, dw and db equal the eager call's bit
for bit.  The queue settings stay the machine's defaults.  Prints GRAPH_OK on success."""
import faulthandler
import os
import sys

faulthandler.enable()
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import dense_conv_cases as dc  # noqa: E402
from manigaussian_amd import dense_conv3d  # noqa: E402

dev = torch.device("cuda:0")


def stage(msg):
    print("stage:", msg, flush=True)


for case in ("odd_k3", "up0_last_head"):
    t = dc.make_inputs(case)
    x, w, b = (t[k].to(dev).requires_grad_(True) for k in ("x", "w", "b"))
    g = t["g"].to(dev)
    slope = dc.slope_of(case)

    def step():
        x.grad = w.grad = b.grad = None
        y = dense_conv3d(x, w, b, slope)
        y.backward(g)
        return y

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    stage(f"{case}: warm-up done")

    eager = [v.detach().clone() for v in (step(), x.grad, w.grad, b.grad)]
    torch.cuda.synchronize()
    x.grad = w.grad = b.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_y = step()
    torch.cuda.synchronize()
    stage(f"{case}: captured")
    for k in range(2):
        for v in (out_y, x.grad, w.grad, b.grad):
            v.detach().fill_(float("nan"))   # (a replay that wrote nothing would be seen)
        graph.replay()
        torch.cuda.synchronize()
        for name, p, q in zip(("y", "dx", "dw", "db"), (out_y, x.grad, w.grad, b.grad), eager):
            assert dc.same_bits(p.detach().cpu(), q.cpu()), f"{case} replay {k + 1}: {name} differs from the eager call"
    stage(f"{case}: two replays equal the eager call bit for bit")
print("GRAPH_OK")
