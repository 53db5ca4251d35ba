"""Run in its OWN process by tests/test_optim.py::test_manigaussian_step_with_the_optimizer_captured_into_a_hip_graph_follows_a_device_lr
(stream capture is process-wide state; a capture that goes wrong takes the process with it, not the test session).

ManiGaussian's whole step through public API -- render_sets_stacked (two sets of 16 384 Gaussians, F = 3) -> manigaussian_losses
-> backward into the optimizer's flat gradient buffer -> FusedLamb.step(zero_grad=True) with a DEVICE learning rate -- captured
into ONE graph after eager warm-up steps, then replayed while the learning rate is written in place between replays.  Checks:
  1. the optimizer inside the graph: a second FusedLamb on a copy of the parameters, stepped EAGERLY on the gradients each replay
     produced (the graph copies them aside before the step zeroes them) with the same learning rates as Python floats, holds
     bit-identical parameters and moments after every replay -- the kernels are deterministic, so "equal" means equal;
  2. the whole trajectory against the same steps run eagerly from the same start: the rasterizer backward adds with float
     atomics, so two runs agree to summation order only (the existing capture test allows gradients 2e-5 of their maximum).
     The loss is Lipschitz in the parameters and every step moves them by lr x trust ratio x u, so the losses must agree to
     1e-4 relative; per tensor the total displacement must agree to 1 % in L2 (LAMB's update m / sqrt(v) is a function of the
     RATIO of successive gradients, so the few elements whose gradient is a cancelled sum may differ by a whole update; an
     L2 share of 1e-2 allows one element in 10 000 to do so);
  3. the learning rate is followed: a replay at lr = 0 leaves the parameters bit for bit where they were.
Prints GRAPH_OK on success."""
import _graph
import torch

import manigaussian_amd as mg

mg.set_forward_mode("async")  # graph capture needs forwards that never synchronise
from manigaussian_amd import synthetic as syn
from manigaussian_amd.gaussian_renderer import render_sets_stacked

dev = _graph.DEV
P, F, W = 16384, 3, 128
sc = syn.make_scene(P, F=F, M=4, seed=5)
cams = syn.circle_cameras(4, W, W, negative_focal=True)


g = torch.Generator().manual_seed(6)
dxyz, drot = (0.01 * torch.randn(P, 3, generator=g)).to(dev), (0.05 * torch.randn(P, 4, generator=g)).to(dev)
gt_rgb = torch.rand(2, W, W, 3, generator=g).to(dev)
gt_embed = torch.randn(1, F, W, W, generator=g).to(dev)
weights = torch.tensor([[1.0, 0.01], [0.01, 0.0]]).to(dev)
datas = [_graph.data_of(cams[0], W, dev), _graph.data_of(cams[2], W, dev)]
bg = torch.zeros(3, device=dev)
HYPER = dict(betas=(0.9, 0.999), eps=1e-6, weight_decay=1e-6)
LRS = [5e-4, 5e-4, 2.5e-4, 1e-3, 1e-4]  # the schedule: one value per step
WARM = 2


class Trainer:
    """Leaves, optimizer and the step; lr = None: a device tensor the caller writes in place."""

    def __init__(self, start, lr=None):
        self.leaves = {k: v.clone().requires_grad_(True) for k, v in start.items()}
        self.lr = torch.tensor([LRS[0]], device=dev) if lr is None else lr
        self.opt = mg.FusedLamb(list(self.leaves.values()), lr=self.lr, zero_grad=True, **HYPER)
        self.flat = self.opt._layout["flat"]
        self.grads = torch.zeros_like(self.flat)

    def step(self):
        lv = self.leaves
        cur = (datas[0], 0, lv["means3D"], lv["rotations"], lv["scales"], lv["opacities"], None, lv["shs"], lv["language_feature"])
        nxt = (datas[1], 0, lv["means3D"] + dxyz, lv["rotations"] + drot, lv["scales"].detach(), lv["opacities"].detach(), None,
               lv["shs"].detach(), lv["language_feature"].detach())
        outs, batch = render_sets_stacked([cur, nxt], bg)
        loss, _ = mg.manigaussian_losses(outs[0], outs[1], gt_rgb, gt_embed, None, lambda_embed=0.01, lambda_dyna=0.01,
                                         stacked=batch, weights=weights)
        loss.backward()           # accumulates into the views of the flat buffer (all zeros: the last step zeroed it)
        self.grads.copy_(self.flat)
        self.opt.step()
        return loss.detach()

    def params(self):
        return [p.detach().clone() for p in self.leaves.values()]


start = {k: v.to(dev) for k, v in sc.items()}

# ---- the eager trajectory ----------------------------------------------------------------------------------------------------
eager = Trainer(start)
eager_losses, eager_params = [], []
for lr in LRS:
    eager.lr.fill_(lr)
    eager_losses.append(eager.step().clone())
    mg.check_status(dev)
    eager_params.append(eager.params())
torch.cuda.synchronize()
assert not eager.flat.any().item(), "zero_grad=True left gradients behind"
_graph.stage("eager trajectory done")

# ---- the captured one: WARM eager steps, then one graph replayed for the rest ------------------------------------------------
tr = Trainer(start)
shadow_leaves = [v.clone().requires_grad_(True) for v in start.values()]
shadow = mg.FusedLamb(shadow_leaves, lr=LRS[0], **HYPER)
losses = []


def shadow_step(lr):
    shadow.param_groups[0]["lr"] = lr
    for p, q in zip(shadow_leaves, tr.leaves.values()):
        view = tr.opt._layout["views"][tr.opt._layout["index"][id(q)]]
        p.grad.copy_(tr.grads[view.storage_offset():view.storage_offset() + view.numel()].view_as(p))
    shadow.step()
    torch.cuda.synchronize()
    for p, q in zip(shadow_leaves, tr.leaves.values()):
        assert torch.equal(p.detach(), q.detach()), f"lr {lr}: the captured optimizer and the eager one differ"
        assert torch.equal(shadow.state[p]["exp_avg"], tr.opt.state[q]["exp_avg"])
        assert torch.equal(shadow.state[p]["exp_avg_sq"], tr.opt.state[q]["exp_avg_sq"])
        assert torch.equal(shadow.state[p]["trust_ratio"], tr.opt.state[q]["trust_ratio"])


for lr in LRS[:WARM]:
    tr.lr.fill_(lr)
    losses.append(tr.step().clone())
    mg.check_status(dev)
    shadow_step(lr)
_graph.stage("warm-up steps done")
saved = tr.params(), [t.clone() for t in (tr.opt._layout["state"],)]
# (lr = 0, written on the side stream, moves no parameter, but the moments advance: put both back below)
_graph.warm_up(tr.step, runs=1, before_each=lambda: tr.lr.fill_(0.0))
with torch.no_grad():
    for p, q in zip(tr.leaves.values(), saved[0]):
        assert torch.equal(p.detach(), q), "a step at lr = 0 moved a parameter"
    tr.opt._layout["state"].copy_(saved[1][0])
_graph.stage("side-stream warm-up done")
graph, out_loss = _graph.capture(tr.step)
_graph.stage("captured")
with torch.no_grad():  # (capture executes nothing: state and parameters are as saved)
    for p, q in zip(tr.leaves.values(), saved[0]):
        assert torch.equal(p.detach(), q)
for lr in LRS[WARM:]:
    tr.lr.fill_(lr)  # the schedule, written in place between replays
    _graph.replay(graph)
    mg.check_status(dev)
    losses.append(out_loss.clone())
    shadow_step(lr)
_graph.stage("replays equal the eager optimizer on the replays' gradients, bit for bit")
assert not tr.flat.any().item(), "zero_grad=True left gradients behind in the graph"

# ---- 2. against the eager trajectory -----------------------------------------------------------------------------------------
for k, (a, b) in enumerate(zip(losses, eager_losses)):
    rel = abs(a.item() - b.item()) / abs(b.item())
    print(f"step {k}: loss {a.item():.9g} eager {b.item():.9g} rel {rel:.3g}")
    assert rel <= 1e-4, (k, rel)
first = [v for v in start.values()]
for name, p, q, p0 in zip(start, tr.params(), eager_params[-1], first):
    moved = (q - p0).double().norm().item()
    diff = (p - q).double().norm().item()
    print(f"{name}: |graph - eager| {diff:.3g} of |eager - start| {moved:.3g} ({diff / moved if moved else 0:.3g})")
    assert moved > 0 and diff <= 1e-2 * moved, name
_graph.stage("the replayed trajectory equals the eager one")

# ---- 3. lr = 0 ------------------------------------------------------------------------------------------------------------------
before = tr.params()
tr.lr.fill_(0.0)
_graph.replay(graph)
for p, q in zip(tr.params(), before):
    assert torch.equal(p, q), "a replay at lr = 0 moved a parameter"
_graph.ok()
