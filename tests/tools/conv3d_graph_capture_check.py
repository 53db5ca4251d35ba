"""Run in its OWN process by tests/test_conv3d.py::test_forward_and_backward_captured_into_a_hip_graph (stream capture is
process-wide state; a capture that goes wrong takes the process with it, not the test session).

One forward + backward of conv3d at the `stem_in` case, and one of conv_transpose3d at `up_op1`, each captured into ONE graph on a
single stream after two eager warm-up runs, then replayed twice.  The kernels are deterministic and keep no state, so after every
replay y, dx and dw equal the eager call's bit for bit.  The queue settings stay the machine's defaults.  Prints GRAPH_OK on success."""
import faulthandler
import os
import sys

faulthandler.enable()
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import conv3d_cases as cc  # noqa: E402
from manigaussian_amd import conv3d, conv_transpose3d  # noqa: E402

dev = torch.device("cuda:0")


def stage(msg):
    print("stage:", msg, flush=True)


for case in ("stem_in", "up_op1"):
    t = cc.make_inputs(case)
    x, w = (t[k].to(dev).requires_grad_(True) for k in ("x", "w"))
    g = t["g"].to(dev)

    def step():
        x.grad = w.grad = None
        if cc.is_transposed(case):
            y = conv_transpose3d(x, w, cc.TRANSPOSED[case]["shape"][4])
        else:
            y = conv3d(x, w, cc.CASES[case]["shape"][4])
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

    eager = [v.detach().clone() for v in (step(), x.grad, w.grad)]
    torch.cuda.synchronize()
    x.grad = w.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_y = step()
    torch.cuda.synchronize()
    stage(f"{case}: captured")
    for k in range(2):
        for v in (out_y, x.grad, w.grad):
            v.detach().fill_(float("nan"))   # (a replay that wrote nothing would be seen)
        graph.replay()
        torch.cuda.synchronize()
        for name, p, q in zip(("y", "dx", "dw"), (out_y, x.grad, w.grad), eager):
            assert cc.same_bits(p.detach().cpu(), q.cpu()), f"{case} replay {k + 1}: {name} differs from the eager call"
    stage(f"{case}: two replays equal the eager call bit for bit")
print("GRAPH_OK")
