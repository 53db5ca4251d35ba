"""manigaussian_amd.optim.FusedLamb (csrc/mgs_optim.hip) against the reference's own `Lamb` (helpers/optim/lamb.py), executed
unmodified on the CPU in float64 (tests/lamb_cases.py; committed fixtures where no copy of the reference exists).

Bounds.  Every step ends in one fp32 addition into p, which rounds by at most half an ulp of p, and a relative error epsilon
in the update can move that rounding by one more half; so after K steps, per tensor,
    max |p - p64| <= K 2^-23 max |p64| + epsilon path,        path = sum_k max |delta p_k|.
m, v: max |x - x64| <= epsilon max |x64| per tensor; weight_norm, adam_norm, trust_ratio of every step: relative epsilon.
epsilon = 1e-5 comes from the reference's OWN float32 run against its float64 run, not from what the kernels give
(tests/golden/make_golden_lamb.py measures it on the committed cases): worst over the ten cases 3.7e-7 on the statistics
(mani_small_k20, 20 steps), 3.5e-7 on m, 4.0e-7 on v, parameters at no more than 0.29 of the bound above -- all below a quarter
of epsilon.  The fused pass sums the two norms in another order and may contract multiply-adds, hence the head-room.
Discrete outcomes are exact: which branch the trust ratio took, a skipped parameter bit for bit unchanged and without state,
zero_grad=True leaving the flat gradient buffer all zeros.
"""
import os

import numpy as np
import pytest
import torch

from child import run_graph_tool
import lamb_cases as lc

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(lc.CASES))
def test_the_restatement_reproduces_every_fixture(case):
    """lamb_cases.restate (float64, vectorised over flat buffers) against the committed float64 numbers of the reference, to
    1e-12 relative: what lets the GPU box, which has no reference, use the restatement at sizes the fixtures cannot hold."""
    inp = lc.make_inputs(case)
    run = lc.restate(inp)
    lc.assert_input_classes(case, inp, run)
    got, exp = lc.fixture_of_run(run), lc.load_fixture(case)
    assert got["steps"].tolist() == exp["steps"].tolist()
    assert torch.equal(torch.isnan(got["stats"]), torch.isnan(exp["stats"]))
    for key in ("stats", "path", "p", "m", "v", "pmax", "mmax", "vmax"):
        a, b = torch.nan_to_num(got[key]), torch.nan_to_num(exp[key])
        err = ((a - b).abs() / b.abs().clamp_min(1e-300)).max().item() if key in ("stats", "path") else \
            (a - b).abs().max().item() / max(b.abs().max().item(), 1e-300)
        assert err <= 1e-12, (case, key, err)
    degenerate = (exp["stats"][..., 0] == 0) | (exp["stats"][..., 1] == 0)
    assert (got["stats"][..., 2][degenerate] == 1).all()


@pytest.mark.skipif(not lc.have_reference(), reason="no copy of the reference on this machine")
def test_fixtures_match_the_reference():
    """The generator's computation, re-run: the committed files are what the reference's Lamb gives today."""
    for case in lc.CASES:
        inp = lc.make_inputs(case)
        run = lc.reference_run(inp)
        lc.assert_input_classes(case, inp, run)
        got, exp = lc.fixture_of_run(run), lc.load_fixture(case)
        for key in exp:
            assert torch.equal(torch.nan_to_num(got[key].double()), torch.nan_to_num(exp[key].double())), (case, key)


def test_the_production_set_has_62_tensors_and_5725407_parameters():
    shapes = [p.shape for m in lc.mani_modules(512) for p in m.parameters()]
    assert len(shapes) == 62 and sum(int(np.prod(s)) for s in shapes) == 5_725_407


def test_bad_hyper_parameters_and_unsupported_tensors_are_refused():
    from manigaussian_amd import FusedLamb
    p = [torch.zeros(4, 4, requires_grad=True)]
    for kw, msg in ((dict(lr=-1.0), "Invalid learning rate"), (dict(eps=-1e-6), "Invalid epsilon value"),
                    (dict(betas=(1.0, 0.999)), "Invalid beta parameter at index 0"),
                    (dict(betas=(0.9, -0.1)), "Invalid beta parameter at index 1")):
        with pytest.raises(ValueError, match=msg):
            FusedLamb(p, **kw)
    with pytest.raises(RuntimeError, match="no CPU path"):
        FusedLamb(p)


def test_the_library_refuses_bad_arguments_before_any_launch():
    from manigaussian_amd import _lib
    L = _lib.lib()
    assert L.mgs_lamb_chunk_elems() == 4096
    assert L.mgs_lamb_workspace_bytes(0) == 0 and L.mgs_lamb_workspace_bytes(3) >= 24
    fake = 0x10000
    assert L.mgs_lamb_step(0, 1, 1, fake, fake, fake, fake, fake, fake, 1.0, 0, fake, 256, None) == _lib.MGS_ERR_INVALID_ARG
    assert L.mgs_lamb_step(2, 1, 1, fake, fake, fake, fake, fake, fake, 1.0, 0, fake, 256, None) == _lib.MGS_ERR_INVALID_ARG
    assert L.mgs_lamb_step(1, 1, 1, fake, fake, None, fake, fake, fake, 1.0, 0, fake, 256, None) == _lib.MGS_ERR_INVALID_ARG
    assert L.mgs_lamb_step(1, 1, 1, fake, fake, fake, fake + 4, fake, fake, 1.0, 0, fake, 256, None) == _lib.MGS_ERR_INVALID_ARG
    assert "16-byte aligned" in _lib.last_error()
    assert L.mgs_lamb_step(1, 1, 100, fake, fake, fake, fake, fake, fake, 1.0, 0, fake, 256, None) == _lib.MGS_ERR_WORKSPACE


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
def _device_params(inp, dev):
    """The case's parameters on the device; those listed under `offset_view` lie 4 bytes past a 16-byte boundary."""
    out = []
    for i, t in enumerate(inp["params"]):
        if i in inp["case"].get("offset_view", []):
            base = torch.empty(t.numel() + 1, dtype=torch.float32, device=dev)
            v = base[1:].view(t.shape)
            v.copy_(t)
            assert v.data_ptr() % 16 == 4
            out.append(v.requires_grad_(True))
        else:
            out.append(t.to(dev).requires_grad_(True))
    return out


def _optimizer(inp, ps, **kw):
    from manigaussian_amd import FusedLamb
    groups = [dict(params=[ps[i] for i in g["idx"]], lr=g["lr"], betas=g["betas"], eps=g["eps"], weight_decay=g["weight_decay"])
              for g in inp["groups"]]
    return FusedLamb(groups, adam=inp["adam"], **kw)


def _set_grads(ps, gs, dev, scale=1.0):
    for p, g in zip(ps, gs):
        if g is None:
            p.grad = None
        elif p.grad is None:
            p.grad = (g * scale).to(dev)
        else:
            p.grad.copy_((g * scale).to(dev))


def _result(opt, ps, stats, path):
    z = [opt.state.get(p) or {} for p in ps]
    return dict(stats=stats, path=path, p=[p.detach().cpu() for p in ps],
                m=[s["exp_avg"].cpu() if s else torch.zeros(p.shape) for s, p in zip(z, ps)],
                v=[s["exp_avg_sq"].cpu() if s else torch.zeros(p.shape) for s, p in zip(z, ps)],
                steps=[int(s.get("step", 0)) for s in z])


def _run(inp, dev, K=None, params=None, grads_of_step=None, **kw):
    """K eager steps of FusedLamb on the case; -> (result dict in the form of lamb_cases.reference_run, optimizer, parameters)."""
    K = inp["K"] if K is None else K
    grads_of_step = grads_of_step or (lambda k: lc.gradients(inp, k))
    ps = _device_params(inp, dev) if params is None else params
    opt = _optimizer(inp, ps, **kw)
    n = len(ps)
    stats = torch.full((K, n, 3), float("nan"), dtype=torch.float64)
    path = torch.zeros(n, dtype=torch.float64)
    for k in range(K):
        before = [p.detach().clone() for p in ps]
        _set_grads(ps, grads_of_step(k), dev)
        opt.step()
        for i, p in enumerate(ps):
            path[i] += (p.detach() - before[i]).abs().max().double().cpu()
            st = opt.state.get(p)
            if st:
                assert all(isinstance(st[key], torch.Tensor) and st[key].dim() == 0 for key in ("weight_norm", "adam_norm", "trust_ratio"))
                stats[k, i] = torch.stack([st["weight_norm"], st["adam_norm"], st["trust_ratio"]]).double().cpu()
    return _result(opt, ps, stats, path), opt, ps


@gpu
@pytest.mark.parametrize("case", list(lc.CASES))
def test_against_the_float64_reference(case):
    dev = torch.device("cuda:0")
    inp = lc.make_inputs(case)
    initial = [p.clone() for p in inp["params"]]
    got, opt, ps = _run(inp, dev)
    lc.compare(case, got, lc.expected(case, inp), inp["K"])
    for i in inp["case"].get("grad_none", []):  # untouched bit for bit, and no state
        assert torch.equal(ps[i].detach().cpu(), initial[i]) and ps[i] not in opt.state and ps[i].grad is None
    if inp["case"].get("offset_view"):
        assert all(ps[i].data_ptr() % 16 == 4 for i in inp["case"]["offset_view"])


@gpu
def test_production_size_against_the_float64_restatement():
    """The 62 tensors at hidden width 512, three steps, against lamb_cases.restate in float64 on the CPU."""
    dev = torch.device("cuda:0")
    inp = lc.make_inputs(dict(kind="mani", hidden=512, groups=[dict(lc.MANI)], K=3, seed=11))
    assert len(inp["params"]) == 62 and sum(p.numel() for p in inp["params"]) == 5_725_407
    got, _, _ = _run(inp, dev)
    want = lc.restate(inp)
    lc.compare("mani_512", got, dict(lc.fixture_of_run(want), source="restatement"), inp["K"])
    # ... and every element, not only the fixtures' sample
    for i, (a, b) in enumerate(zip(got["p"], want["p"])):
        bound = inp["K"] * 2.0 ** -23 * b.abs().max().item() + lc.EPS_REL * want["path"][i].item()
        assert (a.double() - b).abs().max().item() <= bound, (i, inp["names"][i])
    for key in ("m", "v"):
        for i, (a, b) in enumerate(zip(got[key], want[key])):
            assert (a.double() - b).abs().max().item() <= lc.EPS_REL * b.abs().max().item(), (key, i, inp["names"][i])


def _same(a, b):
    assert torch.equal(torch.nan_to_num(a["stats"]), torch.nan_to_num(b["stats"]))
    for key in ("p", "m", "v"):
        for x, y in zip(a[key], b[key]):
            assert torch.equal(x, y), key


@gpu
def test_two_runs_a_gradient_bucket_and_grad_scale_are_bit_identical():
    from manigaussian_amd.parallel import GradBucket
    dev = torch.device("cuda:0")
    for case in ("mani_small", "odd_sizes"):
        inp = lc.make_inputs(case)
        first, _, _ = _run(inp, dev)
        second, _, _ = _run(inp, dev)
        _same(first, second)
        # a caller-supplied bucket: its views are not padded, so most gradients are NOT 16-byte aligned there
        ps = _device_params(inp, dev)
        bucket = GradBucket({f"p{i}": p for i, p in enumerate(ps)})
        bucket.attach()
        with_bucket, opt, _ = _run(inp, dev, params=ps, bucket=bucket)
        assert all(p.grad.data_ptr() == bucket.views[f"p{i}"].data_ptr() for i, p in enumerate(ps))
        assert any(p.grad.data_ptr() % 16 for p in ps)
        _same(first, with_bucket)
        # grad_scale = 1/4 on the gradients == stepping on gradients pre-multiplied by 0.25 (a power of two: bit for bit)
        scaled, _, _ = _run(inp, dev, grad_scale=0.25)
        pre, _, _ = _run(inp, dev, grads_of_step=lambda k: [None if g is None else g * 0.25 for g in lc.gradients(inp, k)])
        _same(scaled, pre)
        assert not torch.equal(scaled["m"][0], first["m"][0])


@gpu
def test_zero_grad_in_the_step_and_zero_grad_keep_the_views():
    dev = torch.device("cuda:0")
    inp = lc.make_inputs("grad_none")
    plain, _, _ = _run(inp, dev)
    fused, opt, ps = _run(inp, dev, zero_grad=True)
    _same(plain, fused)
    flat = opt._layout["flat"]
    assert flat.numel() >= sum(p.numel() for p in ps) and not flat.any().item()  # all zeros after the step
    views = [p.grad for p in ps]
    _set_grads(ps, [torch.ones(p.shape) for p in ps], dev)
    assert flat.any().item()
    opt.zero_grad()  # set_to_none is ignored: one fill, the views stay
    assert not flat.any().item() and all(p.grad is not None for p in ps)
    assert all(v is None or p.grad.data_ptr() == v.data_ptr() for p, v in zip(ps, views))


@gpu
def test_state_dicts_continue_the_trajectory_and_load_the_reference_layout():
    dev = torch.device("cuda:0")
    inp = lc.make_inputs("two_groups")
    whole, _, _ = _run(inp, dev, K=5)
    half, opt, ps = _run(inp, dev, K=2)
    sd = opt.state_dict()
    assert sd["param_groups"][1]["betas"] == (0.8, 0.99) and set(sd["state"][0]) >= {"step", "exp_avg", "exp_avg_sq", "weight_norm",
                                                                                  "adam_norm", "trust_ratio"}
    sd = {"state": {k: {a: (b.clone() if isinstance(b, torch.Tensor) else b) for a, b in v.items()} for k, v in sd["state"].items()},
          "param_groups": sd["param_groups"]}
    ps2 = [p.detach().clone().requires_grad_(True) for p in ps]
    opt2 = _optimizer(inp, ps2)
    opt2.load_state_dict(sd)
    assert opt2.state[ps2[0]]["step"] == 2
    for k in range(2, 5):
        _set_grads(ps2, lc.gradients(inp, k), dev)
        opt2.step()
    for a, b in zip(ps2, whole["p"]):
        assert torch.equal(a.detach().cpu(), b)
    for p, m, v in zip(ps2, whole["m"], whole["v"]):
        assert torch.equal(opt2.state[p]["exp_avg"].cpu(), m) and torch.equal(opt2.state[p]["exp_avg_sq"].cpu(), v)
        assert opt2.state[p]["step"] == 5
    # the reference's layout, built by hand: per-parameter tensors, Python-number statistics (its degenerate ratio is the int 1)
    ref_sd = {"state": {i: {"step": 2, "exp_avg": half["m"][i].clone(), "exp_avg_sq": half["v"][i].clone(),
                            "weight_norm": torch.tensor(1.5), "adam_norm": torch.tensor(2.5), "trust_ratio": 1}
                        for i in range(len(ps))},
              "param_groups": [dict(lr=g["lr"], betas=g["betas"], eps=g["eps"], weight_decay=g["weight_decay"], params=list(g["idx"]))
                               for g in inp["groups"]]}
    ps3 = [p.detach().clone().requires_grad_(True) for p in ps]
    opt3 = _optimizer(inp, ps3)
    opt3.load_state_dict(ref_sd)
    st = opt3.state[ps3[2]]
    assert st["trust_ratio"].item() == 1 and st["weight_norm"].item() == 1.5
    for k in range(2, 5):
        _set_grads(ps3, lc.gradients(inp, k), dev)
        opt3.step()
    for a, b in zip(ps3, whole["p"]):
        assert torch.equal(a.detach().cpu(), b)


@gpu
def test_a_replaced_parameter_storage_and_a_foreign_gradient_are_picked_up():
    dev = torch.device("cuda:0")
    inp = lc.make_inputs("wd0")
    want, _, _ = _run(inp, dev)
    ps = _device_params(inp, dev)
    opt = _optimizer(inp, ps)
    keep = []
    for k in range(inp["K"]):
        if k == 1:   # the parameter moves to another allocation: the old pointer must not be used again
            keep.append(ps[0].data)
            ps[0].data = ps[0].data.clone()
            keep[0].fill_(float("nan"))
        gs = lc.gradients(inp, k)
        if k == 2:   # somebody assigns fresh gradient tensors: copied into the views, .grad re-pointed
            views = [p.grad for p in ps]
            for p, g in zip(ps, gs):
                p.grad = g.to(dev)
            opt.step()
            assert all(p.grad.data_ptr() == v.data_ptr() for p, v in zip(ps, views))
        else:
            _set_grads(ps, gs, dev)
            opt.step()
    for a, b in zip(ps, want["p"]):
        assert torch.equal(a.detach().cpu(), b)
    assert torch.isnan(keep[0]).all()
    # changed Python hyper-parameters reach the device table; a device lr is read where it lives
    inp2 = lc.make_inputs("wd0")
    inp2["groups"][0]["lr"] = 2e-3
    want2, _, _ = _run(inp2, dev, K=2)
    for form in ("float", "tensor"):
        ps = _device_params(inp, dev)
        opt = _optimizer(inp, ps)          # lr 1e-3
        lr = torch.tensor([1.0], device=dev)
        opt.param_groups[0]["lr"] = 2e-3 if form == "float" else lr
        if form == "tensor":
            lr.fill_(2e-3)                 # in place, after the optimizer was handed the tensor
        for k in range(2):
            _set_grads(ps, lc.gradients(inp, k), dev)
            opt.step()
        for a, b in zip(ps, want2["p"]):
            assert torch.equal(a.detach().cpu(), b), form


@gpu
def test_the_step_never_synchronises_with_the_host():
    """FusedLamb.step under torch's sync debug mode "error" (process-wide: restored in the finally), including a step that
    rebuilds the device tables (changed lr) and one that adopts a foreign gradient."""
    dev = torch.device("cuda:0")
    inp = lc.make_inputs("mani_small")
    ps = _device_params(inp, dev)
    opt = _optimizer(inp, ps, zero_grad=True)
    gs = [[g.to(dev) for g in lc.gradients(inp, k)] for k in range(3)]
    for p, g in zip(ps, gs[0]):
        p.grad.copy_(g)
    opt.step()  # (library loaded, pools warm)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for p, g in zip(ps, gs[1]):
            p.grad.copy_(g)
        opt.step()
        opt.param_groups[0]["lr"] = 1e-4
        for p, g in zip(ps, gs[2]):
            p.grad = g
        opt.step()
        opt.zero_grad()
    finally:
        torch.cuda.set_sync_debug_mode(before)
    torch.cuda.synchronize()
    assert opt.state[ps[0]]["step"] == 3 and torch.isfinite(ps[0]).all()


@gpu
def test_manigaussian_step_with_the_optimizer_captured_into_a_hip_graph_follows_a_device_lr():
    """In a child process (stream capture is process-wide state) under its own time limit."""
    run_graph_tool("optim_graph_capture_check.py", limit=170)
