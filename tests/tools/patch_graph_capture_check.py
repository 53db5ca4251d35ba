"""Run in its OWN process by test_forward_and_backward_captured_into_a_hip_graph of tests/test_patch_conv.py (stream capture is
process-wide state; a capture that goes wrong takes the process with it, not the test session):
patch_graph_capture_check.py <case> [<case> ...], names of tests/patch_conv_cases.py's CASES.

One forward + backward of the public patch_conv3d at each case (the test passes `odd`: a batch, rows off 16-byte boundaries, a partial
N-tile and leaky ReLU, and `site_small`: the site's channels at k = 5 with uncovered voxels), each captured into ONE graph on a single
stream after two eager warm-up runs, then replayed twice.  The kernels are deterministic and keep no state, so after every replay y,
dx, dw and db equal the eager call's bit for bit.  The queue settings stay the machine's defaults.  Prints GRAPH_OK on success."""
import faulthandler
import os
import sys

faulthandler.enable()
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import patch_conv_cases as pc  # noqa: E402

cases = sys.argv[1:]
assert cases and all(c in pc.CASES for c in cases), cases
dev = torch.device("cuda:0")


def stage(msg):
    print("stage:", msg, flush=True)


for case in cases:
    t = pc.make_inputs(case)
    names = [k for k in ("x", "w", "b") if t.get(k) is not None]
    leaves = {k: t[k].to(dev).requires_grad_(True) for k in names}
    g = t["g"].to(dev)

    def no_grads():
        for v in leaves.values():
            v.grad = None

    def step():
        no_grads()
        y = pc.call(case, leaves["x"], leaves["w"], leaves.get("b"))
        y.backward(g)
        return y

    def results(y):
        return [y] + [v.grad for v in leaves.values()]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    stage(f"{case}: warm-up done")

    eager = [v.detach().clone() for v in results(step())]
    torch.cuda.synchronize()
    no_grads()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_y = step()
    torch.cuda.synchronize()
    stage(f"{case}: captured")
    for k in range(2):
        for v in results(out_y):
            v.detach().fill_(float("nan"))   # (a replay that wrote nothing would be seen)
        graph.replay()
        torch.cuda.synchronize()
        for name, p, q in zip(["y"] + ["d" + n for n in names], results(out_y), eager):
            assert pc.same_bits(p.detach().cpu(), q.cpu()), f"{case} replay {k + 1}: {name} differs from the eager call"
    stage(f"{case}: two replays equal the eager call bit for bit")
print("GRAPH_OK")
