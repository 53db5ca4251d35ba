"""Run in its OWN process by test_forward_and_backward_captured_into_a_hip_graph of tests/test_wide_pointwise.py (stream capture is
process-wide state; a capture that goes wrong takes the process with it, not the test session):
wide_pointwise_graph_capture_check.py [<case> ...], names of tests/wide_pointwise_cases.py (none: `stem_out_128_batch`, single-word
accesses, two blocks of output channels and a batch, and `in_16`, the 16-channel forms and three blocks).

One forward + backward of wide_pointwise_conv3d at each case, captured into ONE graph on a single stream after two eager warm-up
runs on a side stream, then replayed twice with NaN-filled outputs.  The kernels are deterministic and keep no state, so after every
replay y, dx, dw and db equal the eager call's bit for bit.  The queue settings stay the machine's defaults.  Prints GRAPH_OK on
success."""
import sys

import _graph
import torch

import wide_pointwise_cases as wc

for case in sys.argv[1:] or ("stem_out_128_batch", "in_16"):
    t = wc.make_inputs(case)
    names = [k for k in ("x", "w", "b") if t.get(k) is not None]
    leaves = {k: t[k].to(_graph.DEV).requires_grad_(True) for k in names}
    g = t["g"].to(_graph.DEV)

    def no_grads():
        for v in leaves.values():
            v.grad = None

    def step():
        no_grads()
        y = wc.call(case, leaves["x"], leaves["w"], leaves.get("b"))
        y.backward(g)
        return y

    def results(y):
        return [y] + [v.grad for v in leaves.values()]

    _graph.warm_up(step)
    _graph.stage(f"{case}: warm-up done")
    eager = _graph.copies(results(step()))
    torch.cuda.synchronize()
    no_grads()
    graph, out_y = _graph.capture(step)
    _graph.stage(f"{case}: captured")
    _graph.replays_equal(graph, lambda: results(out_y), eager, ["y"] + ["d" + n for n in names], case)
    _graph.stage(f"{case}: two replays equal the eager call bit for bit")
_graph.ok()
