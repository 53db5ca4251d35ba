"""Run in its OWN process by test_forward_and_backward_captured_into_a_hip_graph of tests/test_conv3d.py, test_pointwise.py,
test_narrow_conv.py, test_dense_conv.py and test_patch_conv.py (stream capture is process-wide state; a capture that goes wrong takes
the process with it, not the test session):  conv_graph_capture_check.py <family> [<case> ...], a name of tests/conv_family.py's
FAMILIES and names of that family's cases (none: the family's graph_cases).

One forward + backward of the family's public op at each of its two graph cases (conv_family's graph_cases: conv3d `stem_in` and the
transposed `up_op1`; pointwise `stem_out_batch`, single-word accesses and the fused backward, and `in_pre`, 16-byte accesses and the
16-channel forms; narrow `odd`, word-by-word rows, three output channels and a batch, and `head`, the site's channels; dense
`odd_k3`, a batch, odd rows, a partial N-tile and leaky ReLU, and `up0_last_head`, a site's channels at k = 5; patch `odd`, a batch,
rows off 16-byte boundaries, a partial N-tile and leaky ReLU, and `site_small`, the site's channels at k = 5 with uncovered voxels),
each captured into ONE graph on a single stream after two eager warm-up runs, then replayed twice.  The kernels are deterministic and
keep no state, so after every replay y, dx, dw and db equal the eager call's bit for bit.  The queue settings stay the machine's
defaults.  Prints GRAPH_OK on success."""
import sys

import _graph
import torch

import conv_family as cf

family = cf.FAMILIES[sys.argv[1]]
cases = sys.argv[2:] or family.graph_cases

for case in cases:
    t = family.cases.make_inputs(case)
    names = [k for k in ("x", "w", "b") if t.get(k) is not None]
    leaves = {k: t[k].to(_graph.DEV).requires_grad_(True) for k in names}
    g = t["g"].to(_graph.DEV)

    def no_grads():
        for v in leaves.values():
            v.grad = None

    def step():
        no_grads()
        y = family.call(case, leaves["x"], leaves["w"], leaves.get("b"))
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
