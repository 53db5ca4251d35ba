"""manigaussian_amd.losses: the fused rendering losses (csrc/mgs_loss.hip) against the reference's own loss.py /
PSNR_torch / _embed_loss_fn, executed unmodified in float64 (tests/loss_cases.py; committed fixtures where no copy of the
reference exists).

Tolerances come from fp32 rounding, not from what the kernels give: the reference's OWN float32 evaluation is within 8e-8
(loss values, relative) and 2.8e-7 (gradients, in the units of loss_cases.compare) of float64 at 128^2 / 256^2 / 100 x 75,
F = 3 and 32, all three embed functions; the fused pass sums in another order and may contract a dot product, so it gets
1e-5.  PSNR: 20 log10 of a 1e-5 relative change is 4e-5 dB -> 1e-4 dB absolute.
"""
import os

import pytest
import torch

from child import run_graph_tool
import loss_cases as lc
from manigaussian_amd import losses
from manigaussian_amd import synthetic as syn

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _offset_copy(t, off, dev):
    """t on the device, its first element `off` floats past an allocation's (16-byte aligned) base."""
    if not off:
        return t.to(dev)
    base = torch.empty(t.numel() + off, dtype=t.dtype, device=dev)
    v = base[off:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * off
    return v


def _device_inputs(case, dev):
    c = lc.CASES[case]
    inp, special = lc.make_inputs(case)
    off = c.get("offset", 0)
    color = _offset_copy(inp["color"], off, dev).detach().requires_grad_(True)
    feature = _offset_copy(inp["feature"], off, dev).detach().requires_grad_(True)
    gt_rgb = _offset_copy(lc.lay_out(inp["gt_rgb"], c["layout"][0]), off, dev)
    gt_embed = _offset_copy(lc.lay_out(inp["gt_embed"], c["layout"][1]), off, dev)
    if off:
        assert color.data_ptr() % 16 == 4 and feature.data_ptr() % 16 == 4
    return inp, special, color, feature, gt_rgb, gt_embed


def _run(case, dev, scale=None):
    c = lc.CASES[case]
    inp, special, color, feature, gt_rgb, gt_embed = _device_inputs(case, dev)
    loss, terms = losses.rendering_loss(color, gt_rgb, feature, gt_embed, weights=c["weights"], embed_loss_fn=c["fn"])
    (loss if scale is None else scale * loss).backward()
    got = dict(loss=loss.detach().cpu(), terms=torch.stack([terms["loss_rgb"], terms["loss_embed"], terms["psnr"]], 1).cpu(),
               g_color=color.grad.cpu(), g_feature=feature.grad.cpu())
    return inp, special, got


@gpu
@pytest.mark.parametrize("case", list(lc.CASES))
def test_against_the_float64_reference(case):
    """Every case of loss_cases.CASES: ManiGaussian's step (V = 2, 128^2, F = 3, cosine, weights [(1, 0.01), (0.01, 0)]), the
    same before the warm-up (lambda_dyna = 0: value reported, gradient exactly zero), the static step, F = 32, V = 8 at 256^2,
    100 x 75 with F = 5 (W % 4 != 0), bases 4 bytes past a 16-byte boundary, every embed function, channel-last /
    channel-first / permuted-view targets."""
    dev = torch.device("cuda:0")
    c = lc.CASES[case]
    inp, special, got = _run(case, dev)
    lc.assert_input_classes(case, inp, special)
    exp = lc.expected(case, inp, special, dev)
    lc.compare(case, inp, got, exp)
    for v, (w_rgb, w_emb) in enumerate(c["weights"] or []):
        if w_rgb == 0:
            assert got["terms"][v, 0] > 0 and not got["g_color"][v].any()
        if w_emb == 0:
            assert not got["g_feature"][v].any()
    if c["fn"] == "cosine":  # the zero-pixel quirk: the reference's gradient there is 1e8 / N x the weight, not zero
        V, F, N = c["V"], c["F"], c["H"] * c["W"]
        w = c["weights"] or [(1.0, 1.0)] * V
        zero = inp["feature"].view(V, F, N)[0].norm(dim=0) == 0
        live_target = inp["gt_embed"].view(V, N, F)[0].norm(dim=1) > 0
        g0 = got["g_feature"].view(V, F, N)[0][:, zero & live_target].norm(dim=0)
        assert torch.allclose(g0, torch.full_like(g0, w[0][1] * 1e8 / N), rtol=1e-4)


@gpu
def test_psnr_is_exactly_100_for_identical_images_and_embed_terms_vanish_without_features():
    dev = torch.device("cuda:0")
    inp, _ = lc.make_inputs("mani_step")
    color = inp["color"].to(dev).requires_grad_(True)
    gt = inp["color"].permute(0, 2, 3, 1).contiguous().to(dev)
    loss, t = losses.rendering_loss(color, gt)
    loss.backward()
    assert t["psnr"].tolist() == [100.0, 100.0] and t["loss_rgb"].tolist() == [0.0, 0.0] and loss.item() == 0.0
    assert t["loss_embed"].tolist() == [0.0, 0.0] and not color.grad.any()
    # one view without a leading dimension, feature given without a target: no embed term, no feature gradient
    c1 = inp["color"][0].to(dev).requires_grad_(True)
    f1 = inp["feature"][0].to(dev).requires_grad_(True)
    loss, t = losses.rendering_loss(c1, inp["gt_rgb"][0].to(dev), f1, None)
    loss.backward()
    assert c1.grad.shape == c1.shape and f1.grad is None and t["loss_embed"].item() == 0.0
    want = ((inp["color"][0].double().permute(1, 2, 0) - inp["gt_rgb"][0].double()) ** 2).mean().item()
    assert abs(loss.item() - want) <= 1e-5 * want


@gpu
@pytest.mark.parametrize("layout", ["view", "first", "last"])
def test_targets_are_consumed_where_they_lie(layout, monkeypatch):
    """No copy of a target, whatever its layout: the pointer and the strides the library receives are the caller's tensor's."""
    dev = torch.device("cuda:0")
    inp, _ = lc.make_inputs("cosine_view")
    gt_rgb, gt_embed = lc.lay_out(inp["gt_rgb"], layout).to(dev), lc.lay_out(inp["gt_embed"], layout).to(dev)
    if layout == "view":
        assert not gt_rgb.is_contiguous() and gt_rgb.shape == inp["gt_rgb"].shape
    seen = []
    real = losses._lib.lib().mgs_render_loss_forward

    def spy(*a):
        seen.append(a)
        return real(*a)

    L = losses._lib.lib()
    monkeypatch.setattr(L, "mgs_render_loss_forward", spy)
    loss, _ = losses.rendering_loss(inp["color"].to(dev), gt_rgb, inp["feature"].to(dev), gt_embed, weights=lc.MANI)
    (a,) = seen
    assert a[5] == gt_rgb.data_ptr() and a[8] == gt_embed.data_ptr()
    sv, s1, s2, s3 = gt_rgb.stride()
    want = (sv, s1, s2, s3) if layout == "first" else (sv, s3, s1, s2)
    assert tuple(a[6]) == want
    monkeypatch.undo()
    ref, _ = losses.rendering_loss(inp["color"].to(dev), inp["gt_rgb"].to(dev), inp["feature"].to(dev), inp["gt_embed"].to(dev),
                                   weights=lc.MANI)
    assert abs(loss.item() - ref.item()) <= 1e-6 * abs(ref.item())


@gpu
def test_upstream_scale_unrequired_inputs_and_a_second_backward():
    dev = torch.device("cuda:0")
    inp, special, unit = _run("mani_step", dev)
    _, _, scaled = _run("mani_step", dev, scale=0.01)
    for k in ("g_color", "g_feature"):
        want = unit[k].double() * 0.01
        assert (scaled[k].double() - want).abs().max().item() <= 1e-6 * want.abs().max().item()
    # only the inputs that require grad get one
    c = lc.CASES["mani_step"]
    _, _, color, feature, gt_rgb, gt_embed = _device_inputs("mani_step", dev)
    f_const = feature.detach()
    loss, _ = losses.rendering_loss(color, gt_rgb, f_const, gt_embed, weights=c["weights"])
    g = torch.autograd.grad(loss, [color])[0]
    assert torch.equal(g.cpu(), unit["g_color"]) and f_const.grad is None
    loss, _ = losses.rendering_loss(color.detach(), gt_rgb, feature, gt_embed, weights=c["weights"])
    assert torch.equal(torch.autograd.grad(loss, [feature])[0].cpu(), unit["g_feature"])
    loss, _ = losses.rendering_loss(color.detach(), gt_rgb, f_const, gt_embed, weights=c["weights"])
    assert loss.grad_fn is None and not loss.requires_grad
    # retain_graph and a second backward: the same gradients
    loss, _ = losses.rendering_loss(color, gt_rgb, feature, gt_embed, weights=c["weights"])
    g1 = torch.autograd.grad(loss, [color, feature], retain_graph=True)
    g2 = torch.autograd.grad(loss, [color, feature])
    assert all(torch.equal(a, b) for a, b in zip(g1, g2))
    with pytest.raises(RuntimeError, match="must not require grad"):
        losses.rendering_loss(color, gt_rgb.clone().requires_grad_(True), feature, gt_embed)


@gpu
@pytest.mark.parametrize("case", ["mani_step", "l2_norm_odd_f5", "v8_256_f32"])
def test_two_calls_are_bit_identical(case):
    dev = torch.device("cuda:0")
    _, _, a = _run(case, dev)
    _, _, b = _run(case, dev)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def _torch_block(color, feature, gt_rgb, gt_embed, weights, psnr):
    """The loss block as the reference writes it (neural_rendering.py:299-329), float32, with or without PSNR_torch."""
    nr = lc.reference_modules()[1] if psnr else None
    loss = 0.
    for v, (w_rgb, w_emb) in enumerate(weights):
        x = color[v:v + 1].permute(0, 2, 3, 1)
        loss = loss + w_rgb * ((x - gt_rgb[v:v + 1]) ** 2).mean()
        if psnr:
            nr.PSNR_torch(x, gt_rgb[v:v + 1])
        e = feature[v:v + 1].permute(0, 2, 3, 1)
        loss = loss + w_emb * (1 - torch.nn.functional.cosine_similarity(e, gt_embed[v:v + 1], dim=-1).mean())
    return loss


@gpu
def test_forward_and_backward_never_synchronise_with_the_host():
    """rendering_loss and its backward on plain leaf tensors under torch's sync debug mode "error" (process-wide: restored in
    the finally); the reference's PSNR_torch raises there -- its `if mse == 0` reads the device."""
    dev = torch.device("cuda:0")
    c = lc.CASES["mani_step"]
    _, _, color, feature, gt_rgb, gt_embed = _device_inputs("mani_step", dev)
    gt_embed_last = gt_embed.permute(0, 2, 3, 1).contiguous()
    w_dev = torch.tensor(c["weights"], dtype=torch.float32).to(dev)
    losses.rendering_loss(color, gt_rgb, feature, gt_embed, weights=c["weights"])[0].backward()  # (library loaded, pools warm)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for fn in ("cosine", "l2", "l2_norm"):
            for w in (c["weights"], w_dev, None):
                color.grad = feature.grad = None
                loss, terms = losses.rendering_loss(color, gt_rgb, feature, gt_embed, weights=w, embed_loss_fn=fn)
                (0.01 * loss).backward()
        _torch_block(color, feature, gt_rgb, gt_embed_last, c["weights"], psnr=False).backward()  # (torch's own block: fine)
        if lc.ref_import.have_reference():
            with pytest.raises(RuntimeError, match="synchroniz"):
                _torch_block(color, feature, gt_rgb, gt_embed_last, c["weights"], psnr=True)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    torch.cuda.synchronize()
    assert terms["psnr"].shape == (2,) and color.grad is not None


def _mani_scene(dev, P=16384, F=3, W=128):
    sc = syn.make_scene(P, F=F, M=4, seed=5)
    cams = syn.circle_cameras(4, W, W, negative_focal=True)

    def data_of(cam):
        kw = syn.camera_settings_kwargs(cam, 1, True, device=dev)
        fov = 2.0 * torch.atan(torch.tensor([kw["tanfovx"], kw["tanfovy"]], dtype=torch.float64))
        return {"novel_view": {"FovX": fov[0:1], "FovY": fov[1:2], "height": torch.tensor([W]), "width": torch.tensor([W]),
                               "world_view_transform": kw["viewmatrix"][None], "full_proj_transform": kw["projmatrix"][None],
                               "camera_center": kw["campos"][None]}}

    g = torch.Generator().manual_seed(6)
    dxyz, drot = (0.01 * torch.randn(P, 3, generator=g)).to(dev), (0.05 * torch.randn(P, 4, generator=g)).to(dev)
    gt_rgb, next_gt_rgb = torch.rand(1, W, W, 3, generator=g).to(dev), torch.rand(1, W, W, 3, generator=g).to(dev)
    gt_embed = torch.randn(1, F, W, W, generator=g).to(dev)  # channel-first, as extract_foundation_model_feature returns it

    def items(leaves):
        cur = (data_of(cams[0]), 0, leaves["means3D"], leaves["rotations"], leaves["scales"], leaves["opacities"], None,
               leaves["shs"], leaves["language_feature"])
        nxt = (data_of(cams[2]), 0, leaves["means3D"] + dxyz, leaves["rotations"] + drot, leaves["scales"].detach(),
               leaves["opacities"].detach(), None, leaves["shs"].detach(), leaves["language_feature"].detach())
        return [cur, nxt]

    return sc, items, gt_rgb, next_gt_rgb, gt_embed


@gpu
@pytest.mark.parametrize("form", ["stacked", "per_view"])
def test_manigaussian_step_end_to_end(form):
    """render -> manigaussian_losses -> backward against render -> the torch restatement of the same losses -> backward, at
    ManiGaussian's shape (two sets of 16 384 Gaussians, F = 3, negative focal): the same images bit for bit, every leaf
    gradient within the project's standing 1e-3 max|g| (measured on the MI355X: 1e-7 to 4.4e-7; printed)."""
    from manigaussian_amd.gaussian_renderer import render_sets, render_sets_stacked
    dev = torch.device("cuda:0")
    sc, items, gt_rgb, next_gt_rgb, gt_embed = _mani_scene(dev)
    lam_e, lam_d = 0.01, 0.01

    def run(fused):
        leaves = {k: v.to(dev).clone().requires_grad_(True) for k, v in sc.items()}
        if fused and form == "stacked":
            outs, batch = render_sets_stacked(items(leaves), (0.0, 0.0, 0.0))
            loss, d = losses.manigaussian_losses(outs[0], outs[1], gt_rgb, gt_embed, next_gt_rgb, lambda_embed=lam_e,
                                                 lambda_dyna=lam_d, stacked=batch)
        else:
            outs = render_sets(items(leaves), (0.0, 0.0, 0.0))
            if fused:
                loss, d = losses.manigaussian_losses(outs[0], outs[1], gt_rgb, gt_embed, next_gt_rgb, lambda_embed=lam_e,
                                                     lambda_dyna=lam_d)
            else:
                rn = outs[0]["render"].unsqueeze(0).permute(0, 2, 3, 1)
                re = outs[0]["render_embed"].unsqueeze(0).permute(0, 2, 3, 1)
                l_rgb = ((rn - gt_rgb) ** 2).mean()
                l_emb = 1 - torch.nn.functional.cosine_similarity(re, gt_embed.permute(0, 2, 3, 1), dim=-1).mean()
                l_dyn = ((outs[1]["render"].unsqueeze(0).permute(0, 2, 3, 1) - next_gt_rgb) ** 2).mean()
                loss = 0. + l_rgb + lam_e * l_emb + lam_d * l_dyn
                d = dict(loss_rgb=l_rgb, loss_embed=l_emb, loss_dyna=l_dyn, l1=l_rgb,
                         psnr=20 * torch.log10(1 / torch.sqrt(l_rgb)), loss_reg=torch.zeros((), device=dev))
        loss.backward()
        return outs, leaves, loss.detach(), d

    o_ref, l_ref, loss_ref, d_ref = run(False)
    o_got, l_got, loss_got, d_got = run(True)
    for a, b in zip(o_ref, o_got):
        assert torch.equal(a["render"], b["render"]) and torch.equal(a["render_embed"], b["render_embed"])
    assert set(d_got) == {"loss", "loss_rgb", "loss_embed", "loss_dyna", "loss_reg", "l1", "psnr"}
    assert abs(loss_got.item() - loss_ref.item()) <= 1e-5 * abs(loss_ref.item())
    for k in ("loss_rgb", "loss_embed", "loss_dyna", "l1", "loss_reg"):
        assert d_got[k].is_cuda and d_got[k].dim() == 0 and not d_got[k].requires_grad
        assert abs(d_got[k].item() - d_ref[k].item()) <= 1e-5 * abs(d_ref[k].item()), k
    assert abs(d_got["psnr"].item() - d_ref["psnr"].item()) <= 1e-4
    for k in l_ref:
        ref, got = l_ref[k].grad, l_got[k].grad
        err = (got - ref).abs().max().item() / ref.abs().max().item()
        print(f"  end to end ({form}) {k}: max |g - g_ref| / max |g_ref| = {err:.3g}")
        assert err <= 1e-3, k


@gpu
def test_render_loss_backward_captured_into_a_hip_graph_follows_targets_and_weights():
    """tests/tools/loss_graph_capture_check.py in a process of its own (stream capture is process-wide state): render -> loss
    -> backward captured with torch.cuda.graph, replayed after the target images and the device-side weights were
    overwritten in place; the replay equals the eager step on the new targets and weights."""
    run_graph_tool("loss_graph_capture_check.py", limit=170)


# ---- without a GPU --------------------------------------------------------------------------------------------------------

def test_cpu_tensors_and_bad_arguments_are_refused_with_a_message():
    c, t = torch.zeros(2, 3, 8, 8), torch.zeros(2, 8, 8, 3)
    f, e = torch.zeros(2, 5, 8, 8), torch.zeros(2, 5, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        losses.rendering_loss(c, t)
    with pytest.raises(RuntimeError, match="no CPU path"):
        losses.rendering_loss(c, t, f, e)
    with pytest.raises(RuntimeError, match=r"must have 3 channels"):
        losses.rendering_loss(torch.zeros(2, 4, 8, 8), t)
    with pytest.raises(RuntimeError, match=r"\[C,H,W\] or \[V,C,H,W\]"):
        losses.rendering_loss(torch.zeros(8, 8), t)
    with pytest.raises(RuntimeError, match="float32"):
        losses.rendering_loss(c.double(), t)
    with pytest.raises(RuntimeError, match="float32"):
        losses.rendering_loss(c, t.half())
    with pytest.raises(RuntimeError, match=r"holds 3 views.*V = 2"):
        losses.rendering_loss(c, torch.zeros(3, 8, 8, 3))
    with pytest.raises(RuntimeError, match=r"gt_rgb must be \[2,8,8,3\] or \[2,3,8,8\]"):
        losses.rendering_loss(c, torch.zeros(2, 8, 9, 3))
    with pytest.raises(RuntimeError, match=r"F = 65 feature channels"):
        losses.rendering_loss(c, t, torch.zeros(2, 65, 8, 8), torch.zeros(2, 65, 8, 8))
    with pytest.raises(RuntimeError, match=r"does not match color"):
        losses.rendering_loss(c, t, torch.zeros(3, 5, 8, 8), e)
    with pytest.raises(RuntimeError, match=r"gt_embed holds 1 views"):
        losses.rendering_loss(c, t, f, torch.zeros(1, 5, 8, 8))
    with pytest.raises(RuntimeError, match="not implemented"):
        losses.rendering_loss(c, t, f, e, embed_loss_fn="l1")
    with pytest.raises(RuntimeError, match="must not require grad"):
        losses.rendering_loss(c, t.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match=r"2 pairs"):
        losses._weights([(1.0, 1.0)], 2, torch.device("cpu"))
    import manigaussian_amd as mg
    assert mg.rendering_loss is losses.rendering_loss and mg.manigaussian_losses is losses.manigaussian_losses


def test_library_refuses_bad_shapes_with_a_message():
    """The C ABI's own argument checks (no device needed: they come before any launch)."""
    from manigaussian_amd import _lib
    L = _lib.lib()
    assert L.mgs_render_loss_workspace_bytes(2, 128, 128) >= 2 * 16 * 2 * 4
    rc = L.mgs_render_loss_forward(2, 65, 8, 8, *([None] * 6), 0, None, None, *([None] * 5), 0, None)
    assert rc == _lib.MGS_ERR_INVALID_ARG and "F = 65" in _lib.last_error()
    rc = L.mgs_render_loss_forward(17, 3, 8, 8, *([None] * 6), 0, None, None, *([None] * 5), 0, None)
    assert rc == _lib.MGS_ERR_INVALID_ARG and "V = 17" in _lib.last_error()
    rc = L.mgs_render_loss_forward(2, 3, 8, 8, *([None] * 6), 0, None, None, *([None] * 5), 0, None)
    assert rc == _lib.MGS_ERR_INVALID_ARG and "NULL" in _lib.last_error()
    rc = L.mgs_render_loss_backward(2, 3, 8, 8, None, None, None, None, None, None)
    assert rc == _lib.MGS_ERR_INVALID_ARG and "g_up" in _lib.last_error()


def test_fixtures_match_the_reference():
    """Re-runs tests/golden/make_golden_loss.py's computation where a copy of the reference exists: the committed fixtures
    hold what the reference's code gives today (values to float64 rounding, gradients to the float32 they are stored in)."""
    if not lc.ref_import.have_reference():
        pytest.skip("no copy of the reference (tests then compare against the committed fixtures)")
    total = sum(os.path.getsize(os.path.join(lc.GOLDEN_DIR, f)) for f in os.listdir(lc.GOLDEN_DIR))
    assert total < 1_000_000
    for case in lc.CASES:
        inp, special = lc.make_inputs(case)
        lc.assert_input_classes(case, inp, special)
        now, fx = lc.to_fixture(case, lc.reference(case, inp), special), lc.load_fixture(case)
        assert set(now) == set(fx)
        for k in ("terms", "loss"):
            a, b = torch.from_numpy(now[k]).double(), fx[k].double()
            assert (a - b).abs().max().item() <= 1e-12 * b.abs().max().item(), (case, k)
        assert torch.equal(torch.from_numpy(now["pixels"]), fx["pixels"])
        for k in ("g_color", "g_feature"):
            a, b = torch.from_numpy(now[k]).double(), fx[k].double()
            assert (a - b).abs().max().item() <= 2e-7 * b.abs().max().item(), (case, k)
