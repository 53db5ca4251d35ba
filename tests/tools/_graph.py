"""The scaffold of the graph-capture tools in this directory -- TEST INFRASTRUCTURE.  A tool is started as
`python tests/tools/NAME.py [args]`, in a process of its own (stream capture is process-wide state; a capture that goes wrong takes
the process with it, not the test session), so this directory is first on its sys.path and `import _graph` needs no prelude.
Importing it enables faulthandler and puts the repository root and tests/ on sys.path.

A tool is a step() function plus a comparison: warm_up(step) and capture(step) are torch's capture recipe; captured_step() is the
rasterizer tools' whole sequence (eager steps with check_status, side-stream warm-up, capture, replays) and same_step() their
comparison; replays_equal() and equal_bits() are the stateless ops' bit-for-bit comparison with an eager call.  Nothing here passes
a pool, an error mode or a queue setting: the queue settings stay the machine's defaults."""
import faulthandler
import os
import sys

if not faulthandler.is_enabled():   # (a test session that imports this for same_step has pytest's own)
    faulthandler.enable()
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for path in (ROOT, os.path.join(ROOT, "tests")):
    if path not in sys.path:
        sys.path.insert(0, path)
import torch  # noqa: E402

from numerics import same_bits  # noqa: E402

DEV = torch.device("cuda:0")


def stage(msg):
    """The runner's failure message shows the child's output: the last stage line says how far the tool came."""
    print("stage:", msg, flush=True)


def ok():
    print("GRAPH_OK")


def warm_up(step, runs=2, before_each=None):
    """`runs` calls of step() on a side stream, as torch's capture recipe asks, each after before_each() if given."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(runs):
            if before_each is not None:
                before_each()
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()


def capture(step):
    """(graph, what step() returned inside the capture: the tensors every replay writes)."""
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outputs = step()
    torch.cuda.synchronize()
    return graph, outputs


def replay(graph, times=1):
    """`times` replays back to back, then one synchronise."""
    for _ in range(times):
        graph.replay()
    torch.cuda.synchronize()


def copies(tensors):
    return [t.detach().clone() for t in tensors]


# ---- stateless ops: replays against an eager call, bit for bit -----------------------------------------------------------------
def equal_bits(got, want, names, what):
    for name, p, q in zip(names, got, want):
        assert same_bits(p.detach().cpu(), q.detach().cpu()), f"{what}: {name} differs from the eager call"


def replays_equal(graph, outputs_fn, eager, names, what, replays=2, poison=True):
    """After each of `replays` replays, outputs_fn() -- the tensors the graph writes -- equal `eager` bit for bit: a list of tensors, or
    a function of the replay's number (1, 2, ...) where the op keeps state.  poison: the outputs are filled with NaN before each replay
    (a replay that wrote nothing would be seen); only for outputs that every replay writes in full."""
    for k in range(1, replays + 1):
        if poison:
            for v in outputs_fn():
                v.detach().fill_(float("nan"))
        replay(graph)
        equal_bits(outputs_fn(), eager(k) if callable(eager) else eager, names, f"{what} replay {k}")


# ---- rasterizer steps (the tool has called set_forward_mode("async")) ----------------------------------------------------------
def eager_steps(step, n, dev):
    """n eager steps, each followed by check_status; the last one's results."""
    import manigaussian_amd as mg
    for _ in range(n):
        # detached copies: a kept output would keep its autograd graph -- and the leaves' AccumulateGrad nodes, bound to the
        # default stream -- alive into the capture, where torch would then try to synchronise the two streams (its own
        # warning says so) and the runtime aborts the capture
        last = copies(step())
        mg.check_status(dev)
    return last


def captured_step(step, dev, eager=3, replays=3):
    """`eager` eager steps, one warm-up step on a side stream, the capture, `replays` replays: (graph, the graph's outputs, the last
    eager step's results)."""
    want = eager_steps(step, eager, dev)
    stage("eager steps done")
    warm_up(step, runs=1)
    stage("side-stream warm-up done")
    graph, out = capture(step)
    stage("captured")
    replay(graph, replays)
    return graph, out, want


def same_step(got, want, n_exact, what):
    """The first n_exact values bit for bit (images, radii, losses: deterministic kernels); the rest, parameter gradients, to the
    order of the rasterizer backward's float atomics."""
    assert len(got) == len(want), f"{what}: {len(got)} results, {len(want)} expected"
    for i, (a, b) in enumerate(zip(got[:n_exact], want[:n_exact])):
        assert torch.equal(a, b), f"{what}: value {i} differs"
    for a, b in zip(got[n_exact:], want[n_exact:]):
        assert (a - b).abs().max().item() <= 2e-5 * b.abs().max().item() + 1e-12, f"{what}: gradients differ"


def replay_follows(graph, out, step, dev, n_exact, what):
    """After the caller rewrote the step's inputs in place -- the graph reads them where they live -- one replay equals a fresh eager
    step; returns that step's results."""
    import manigaussian_amd as mg
    torch.cuda.synchronize()
    replay(graph)
    replayed, moved = copies(out), copies(step())
    torch.cuda.synchronize()
    mg.check_status(dev)
    same_step(replayed, moved, n_exact, what)
    return moved


def data_of(cam, W, dev):
    """Host copies of the camera scalars (what manigaussian_amd.camera.TargetCache hands out): no device read per render."""
    from manigaussian_amd import synthetic as syn
    kw = syn.camera_settings_kwargs(cam, 1, True, device=dev)
    return {"novel_view": {"tanfov_host": [(kw["tanfovx"], kw["tanfovy"])], "size_host": [(W, W)],
                           "world_view_transform": kw["viewmatrix"][None], "full_proj_transform": kw["projmatrix"][None],
                           "camera_center": kw["campos"][None]}}
