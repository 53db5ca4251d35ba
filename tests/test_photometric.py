"""manigaussian_amd.photometric: the fused L1 + L2 + D-SSIM loss (csrc/mgs_photometric.hip) against the reference's own
loss.py (l1_loss, l2_loss, ssim, psnr), executed unmodified in float64 (tests/photometric_cases.py; committed fixtures where
no copy of the reference exists).  Tolerances: photometric_cases' docstring -- derived from the reference's own float32
deviation recorded per case, never from what the kernels give.
"""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from child import run_graph_tool
import photometric_cases as pc
from manigaussian_amd import _lib, photometric

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


def _device_inputs(case, dev, layout=None):
    c = pc.CASES[case]
    inp = pc.make_inputs(case)
    off = c.get("offset", 0)
    layout = layout or c["layout"]
    color = _offset_copy(inp["color"], off, dev).detach().requires_grad_(True)
    if layout == "view":
        target = _offset_copy(inp["target"], off, dev).permute(0, 2, 3, 1)
        assert not target.is_contiguous()
    else:
        target = _offset_copy(pc.lay_out(inp["target"], layout), off, dev)
    if off:
        assert color.data_ptr() % 16 == 4 and target.data_ptr() % 16 == 4
    return inp, color, target


def _run(case, dev, weights="case", layout=None):
    c = pc.CASES[case]
    inp, color, target = _device_inputs(case, dev, layout)
    w = c["weights"] if isinstance(weights, str) else weights
    loss, terms = photometric.photometric_loss(color, target, weights=w)
    loss.backward()
    got = dict(loss=loss.detach().cpu(), g=color.grad.cpu(),
               terms=torch.stack([terms["l1"], terms["l2"], terms["ssim"], terms["psnr"]], 1).cpu())
    return inp, got


@gpu
@pytest.mark.parametrize("case", list(pc.CASES))
def test_against_the_float64_reference(case):
    """Every case of photometric_cases.CASES: an image smaller than the window, one exactly its size, W % 4 != 0, tiles with
    halos on both sides, ManiGaussian's step, 32 feature channels, bases 4 bytes past a 16-byte boundary, identical images;
    uniform, smooth (cancelling), black-against-bright and 30 %-equal inputs; every target layout."""
    dev = torch.device("cuda:0")
    c = pc.CASES[case]
    inp, got = _run(case, dev)
    pc.assert_input_classes(case, inp)
    pc.compare(case, got, pc.expected(case))
    assert got["g"].shape == inp["color"].shape
    if c["cls"] == "equal30":  # view 0 has the weights (1, 0, 0): exactly zero where the images are equal
        same = inp["color"][0] == inp["target"][0]
        assert same.any() and not got["g"][0][same].any() and got["g"][0][~same].abs().min() > 0


@gpu
@pytest.mark.parametrize("layout", ["last", "first", "view"])
def test_targets_are_consumed_where_they_lie(layout, monkeypatch):
    """No copy of a target, whatever its layout: the pointer and the strides the library receives are the caller's tensor's;
    and every layout gives the same bits."""
    dev = torch.device("cuda:0")
    case = "odd_37x23"
    inp, color, target = _device_inputs(case, dev, layout)
    seen = []
    L = _lib.lib()
    real = L.mgs_photometric_forward

    def spy(*a):
        seen.append(a)
        return real(*a)

    monkeypatch.setattr(L, "mgs_photometric_forward", spy)
    loss, terms = photometric.photometric_loss(color, target, weights=pc.CASES[case]["weights"])
    monkeypatch.undo()
    (a,) = seen
    assert a[5] == target.data_ptr()
    s0, s1, s2, s3 = target.stride()
    assert tuple(a[6]) == ((s0, s1, s2, s3) if layout == "first" else (s0, s3, s1, s2))
    loss.backward()
    _, ref = _run(case, dev, layout="first")
    assert torch.equal(loss.detach().cpu(), ref["loss"]) and torch.equal(color.grad.cpu(), ref["g"])
    got = dict(loss=loss.detach().cpu(), g=color.grad.cpu(),
               terms=torch.stack([terms["l1"], terms["l2"], terms["ssim"], terms["psnr"]], 1).cpu())
    pc.compare(case, got, pc.expected(case))


@gpu
def test_a_zero_weight_reports_its_term_and_adds_a_bit_zero_gradient():
    dev = torch.device("cuda:0")
    case = "tiles_70x45"
    _, full = _run(case, dev, weights=[(0.8, 0.5, 0.2)])
    _, none = _run(case, dev, weights=[(0.0, 0.0, 0.0)])
    assert torch.equal(full["terms"], none["terms"]) and none["terms"][0, :2].min() > 0 and none["terms"][0, 2] != 0
    assert none["loss"].item() == 0.0 and not none["g"].any()
    _, l1 = _run(case, dev, weights=[(0.8, 0.0, 0.0)])
    _, l2 = _run(case, dev, weights=[(0.0, 0.5, 0.0)])
    _, ss = _run(case, dev, weights=[(0.0, 0.0, 0.2)])
    # each share alone is the same bits as inside the sum's operands: the full gradient is their float32 sum
    assert torch.equal(full["g"], (l1["g"] + l2["g"]) + ss["g"])
    inp = pc.make_inputs(case)
    d = inp["color"] - inp["target"]
    n = d[0].numel()
    assert torch.allclose(l1["g"], 0.8 * torch.sign(d) / n, rtol=1e-6, atol=0)
    assert torch.allclose(l2["g"], 0.5 * 2 * d / n, rtol=1e-6, atol=1e-12)


@gpu
def test_device_weights_updated_in_place_are_followed_and_host_weights_agree():
    dev = torch.device("cuda:0")
    case = "odd_37x23"
    c = pc.CASES[case]
    _, want = _run(case, dev)
    w = torch.tensor([[1.0, 1.0, 1.0], [0.0, 0.0, 0.0]], dtype=torch.float32, device=dev)
    _, other = _run(case, dev, weights=w)
    assert not torch.equal(other["g"], want["g"])
    with torch.no_grad():
        w.copy_(torch.tensor(c["weights"]))
    _, got = _run(case, dev, weights=w)
    for k in want:
        assert torch.equal(got[k], want[k]), k


@gpu
@pytest.mark.parametrize("case", ["odd_37x23", "mani_128", "feat_64_c32"])
def test_two_runs_are_bit_identical(case):
    dev = torch.device("cuda:0")
    _, a = _run(case, dev)
    _, b = _run(case, dev)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@gpu
def test_ssim_per_view_with_a_non_uniform_upstream_vector_and_the_drop_ins():
    dev = torch.device("cuda:0")
    case = "odd_37x23"
    c = pc.CASES[case]
    exp = pc.expected(case)
    inp, color, _ = _device_inputs(case, dev)
    target = inp["target"].to(dev)  # channel-first, as loss.ssim wants it
    s = photometric.ssim(color, target, size_average=False)
    assert s.shape == (c["V"],) and s.grad_fn is not None
    u = torch.tensor(c["ssim_vec"], dtype=torch.float32, device=dev)
    (s * u).sum().backward()
    tol_s, _ = pc.ssim_bounds(exp)
    for v in range(c["V"]):
        d = abs(s[v].item() - exp["terms"][v, 2].item())
        print(f"  ssim[{v}] {s[v].item():.9g} want {exp['terms'][v, 2].item():.9g} abs {d:.3g} bound {tol_s:.3g}")
        assert d <= tol_s
    failures = []
    pc.compare_gradient(case, "g_vec", color.grad.cpu(), exp["g_vec"], exp, failures, {})
    assert not failures, failures
    # size_average=True: the mean over everything, as loss.ssim gives it; the gradient is the per-view one / V
    color.grad = None
    m = photometric.ssim(color, target)
    m.backward()
    want = exp["terms"][:, 2].mean().item()
    assert m.dim() == 0 and abs(m.item() - want) <= tol_s
    # l1_loss: mean |x - y| over everything
    l1 = photometric.l1_loss(color.detach(), target)
    want = exp["terms"][:, 0].mean().item()
    assert abs(l1.item() - want) <= 1e-5 * want
    # one view without a leading dimension
    c1 = inp["color"][0].to(dev).requires_grad_(True)
    loss, t = photometric.photometric_loss(c1, inp["target"][0].to(dev), weights=[c["weights"][0]])
    loss.backward()
    assert c1.grad.shape == c1.shape and t["ssim"].shape == (1,)
    assert abs(t["ssim"].item() - exp["terms"][0, 2].item()) <= tol_s


@gpu
def test_upstream_scale_second_backward_and_inputs_that_need_no_gradient():
    dev = torch.device("cuda:0")
    case = "tiny_8x5"
    _, color, target = _device_inputs(case, dev)
    loss, _ = photometric.photometric_loss(color, target)
    g1, = torch.autograd.grad(loss, [color], retain_graph=True)
    g2, = torch.autograd.grad(loss, [color], retain_graph=True)
    assert torch.equal(g1, g2)
    gs, = torch.autograd.grad(0.25 * loss, [color])
    assert torch.equal(gs, 0.25 * g1)
    loss, terms = photometric.photometric_loss(color.detach(), target)
    assert loss.grad_fn is None and not loss.requires_grad and terms["psnr"].shape == (1,)
    with pytest.raises(RuntimeError, match="must not require grad"):
        photometric.photometric_loss(color, target.clone().requires_grad_(True))


@gpu
def test_forward_and_backward_never_synchronise_with_the_host():
    dev = torch.device("cuda:0")
    _, color, target = _device_inputs("odd_37x23", dev)
    w_dev = torch.ones(2, 3, dtype=torch.float32, device=dev)
    photometric.photometric_loss(color, target)[0].backward()  # (library loaded, pools warm)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for w in (None, [(0.8, 0.0, 0.2)] * 2, w_dev):
            color.grad = None
            loss, terms = photometric.photometric_loss(color, target, weights=w)
            (0.5 * loss).backward()
    finally:
        torch.cuda.set_sync_debug_mode(before)
    torch.cuda.synchronize()
    assert color.grad is not None and terms["ssim"].shape == (2,)


@gpu
def test_render_photometric_loss_backward_captured_into_a_hip_graph_follows_targets_and_weights():
    """tests/tools/photometric_graph_capture_check.py in a process of its own (stream capture is process-wide state): render ->
    photometric_loss -> backward captured with torch.cuda.graph, replayed after the target images and the device-side weights
    were overwritten in place; the replay equals the eager step on the new targets and weights."""
    run_graph_tool("photometric_graph_capture_check.py", limit=170)


# ---- without a GPU --------------------------------------------------------------------------------------------------------

def test_cpu_tensors_and_bad_arguments_are_refused_with_a_message():
    c, t = torch.zeros(2, 3, 8, 8), torch.zeros(2, 8, 8, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        photometric.photometric_loss(c, t)
    with pytest.raises(RuntimeError, match="no CPU path"):
        photometric.ssim(c, torch.zeros(2, 3, 8, 8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        photometric.l1_loss(c, t)
    with pytest.raises(RuntimeError, match=r"window_size = 7 is not implemented"):
        photometric.photometric_loss(c, t, window_size=7)
    with pytest.raises(RuntimeError, match=r"window_size = 7 is not implemented"):
        photometric.ssim(c, torch.zeros(2, 3, 8, 8), window_size=7)
    with pytest.raises(RuntimeError, match=r"C = 65 channels"):
        photometric.photometric_loss(torch.zeros(1, 65, 8, 8), torch.zeros(1, 65, 8, 8))
    with pytest.raises(RuntimeError, match=r"V = 17 views"):
        photometric.photometric_loss(torch.zeros(17, 3, 8, 8), torch.zeros(17, 3, 8, 8))
    with pytest.raises(RuntimeError, match="must not require grad"):
        photometric.photometric_loss(c, t.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match=r"holds 3 views.*V = 2"):
        photometric.photometric_loss(c, torch.zeros(3, 8, 8, 3))
    with pytest.raises(RuntimeError, match=r"no view dimension"):
        photometric.photometric_loss(c, torch.zeros(8, 8, 3))
    with pytest.raises(RuntimeError, match=r"\[C,H,W\] or \[V,C,H,W\]"):
        photometric.photometric_loss(torch.zeros(8, 8), t)
    with pytest.raises(RuntimeError, match=r"target must be \[2,8,8,3\] or \[2,3,8,8\]"):
        photometric.photometric_loss(c, torch.zeros(2, 8, 9, 3))
    with pytest.raises(RuntimeError, match=r"target must be \[2,3,8,8\], got"):
        photometric.ssim(c, t)  # loss.ssim wants channel-first images
    with pytest.raises(RuntimeError, match="float32"):
        photometric.photometric_loss(c.double(), t)
    with pytest.raises(RuntimeError, match="float32"):
        photometric.photometric_loss(c, t.half())
    with pytest.raises(RuntimeError, match=r"2 triples"):
        photometric.photometric_loss(c, t, weights=[(1.0, 0.0, 0.2)])
    with pytest.raises(RuntimeError, match=r"2 triples"):
        photometric._weights([(1.0, 1.0)] * 2, 2, torch.device("cpu"), "photometric_loss")
    with pytest.raises(RuntimeError, match=r"\[V,3\] = \[2,3\]"):
        photometric._weights(torch.zeros(2, 2), 2, torch.device("cpu"), "photometric_loss")
    import manigaussian_amd as mg
    assert mg.photometric_loss is photometric.photometric_loss and mg.ssim is photometric.ssim
    assert mg.l1_loss is photometric.l1_loss


def test_library_refuses_bad_shapes_with_a_message_and_sizes_its_workspace():
    """The C ABI's own argument checks (no device needed: they come before any launch), the workspace query, the ABI version."""
    L = _lib.lib()
    assert _lib.ABI_VERSION == 17 and L.mgs_abi_version() == 17
    with open(os.path.join(ROOT, "include", "mgsplat.h")) as f:
        assert re.search(r"#define MGS_ABI_VERSION 17\b", f.read())
    fwd = lambda V, C, W, H, *p: L.mgs_photometric_forward(V, C, W, H, *(p or [None] * 9), 0, None)  # noqa: E731
    assert fwd(2, 65, 8, 8) == _lib.MGS_ERR_INVALID_ARG and "C = 65" in _lib.last_error()
    assert fwd(17, 3, 8, 8) == _lib.MGS_ERR_INVALID_ARG and "V = 17" in _lib.last_error()
    assert fwd(2, 3, 0, 8) == _lib.MGS_ERR_INVALID_ARG and "empty or too large" in _lib.last_error()
    assert fwd(16, 64, 4096, 4096) == _lib.MGS_ERR_INVALID_ARG and "empty or too large" in _lib.last_error()
    assert fwd(2, 3, 8, 8) == _lib.MGS_ERR_INVALID_ARG and "NULL" in _lib.last_error()
    bwd = L.mgs_photometric_backward
    assert bwd(2, 3, 8, 8, None, 0, None, None, None) == _lib.MGS_ERR_INVALID_ARG and "g_up" in _lib.last_error()
    assert bwd(2, 3, 8, 8, 16, 2, 16, 16, None) == _lib.MGS_ERR_INVALID_ARG and "g_up_stride" in _lib.last_error()
    # addresses that are never dereferenced: the checks below come before any launch
    i64x4 = ctypes.c_int64 * 4
    rc = L.mgs_photometric_forward(2, 3, 8, 8, 256, 256, i64x4(192, 64, -8, 1), None, None, None, 256, 256, 256, 1 << 20, None)
    assert rc == _lib.MGS_ERR_INVALID_ARG and "negative stride" in _lib.last_error()
    rc = L.mgs_photometric_forward(2, 3, 8, 8, 256, 256, i64x4(192, 64, 8, 1), None, None, None, 256, 256, 256, 16, None)
    assert rc == _lib.MGS_ERR_WORKSPACE
    rc = L.mgs_photometric_forward(2, 3, 8, 8, 256, 256, i64x4(1 << 31, 64, 8, 1), None, None, None, 256, 256, 256, 1 << 20, None)
    assert rc == _lib.MGS_ERR_INVALID_ARG and "2^31" in _lib.last_error()
    ws = L.mgs_photometric_workspace_bytes
    assert ws(0, 3, 8, 8) == 0
    prev = 0
    for V, C, W, H in [(1, 1, 1, 1), (1, 1, 8, 5), (1, 3, 8, 5), (1, 3, 37, 23), (2, 3, 37, 23), (2, 3, 128, 128), (2, 4, 128, 128),
                       (2, 4, 129, 128), (2, 4, 129, 129), (8, 3, 256, 256), (16, 64, 256, 256)]:
        n = ws(V, C, W, H)
        tiles = ((W + 31) // 32) * ((H + 31) // 32)
        assert n % 16 == 0 and n > prev and n >= 4 * 3 * V * C * (W * H + tiles), (V, C, W, H, n)
        prev = n


def _header_window():
    with open(os.path.join(ROOT, "include", "mgsplat.h")) as f:
        text = f.read()
    body = re.search(r"#define MGS_SSIM_WINDOW \{(.*?)\}", text, re.S).group(1).replace("\\", " ")
    return np.array([np.float32(x.strip().rstrip("f")) for x in body.split(",")], dtype=np.float32)


def test_the_window_weights_are_the_references_bit_for_bit():
    """photometric.WINDOW and the header's MGS_SSIM_WINDOW (the kernels' constant) against loss.gaussian(11, 1.5): the recorded
    float32 values, and the live function where a copy of the reference exists."""
    want = np.load(os.path.join(pc.GOLDEN_DIR, "window.npz"))["window"]
    assert want.dtype == np.float32 and want.shape == (11,)
    assert float(want[0]) == 0.001028380123898387 and float(want[5]) == 0.26601171493530273
    assert np.array_equal(np.array(photometric.WINDOW, dtype=np.float64), want.astype(np.float64))
    assert np.array_equal(_header_window().view(np.uint32), want.view(np.uint32))
    if pc.ref_import.have_reference():
        live = pc.reference_module().gaussian(11, 1.5).numpy()
        assert np.array_equal(live.view(np.uint32), want.view(np.uint32))


def test_fixtures_match_the_reference():
    """Re-runs tests/golden/make_golden_photometric.py's computation where a copy of the reference exists: the committed
    fixtures hold what the reference's code gives today (values to float64 rounding, gradients to the float32 they are
    stored in), and the recorded float32 deviations are of the size the reference shows today (they set the tolerance)."""
    if not pc.ref_import.have_reference():
        pytest.skip("no copy of the reference (tests then compare against the committed fixtures)")
    total = sum(os.path.getsize(os.path.join(pc.GOLDEN_DIR, f)) for f in os.listdir(pc.GOLDEN_DIR))
    assert total < 1_000_000
    for case in pc.CASES:
        inp = pc.make_inputs(case)
        pc.assert_input_classes(case, inp)
        now, fx = pc.to_fixture(case, inp, pc.reference(case, inp)), pc.load_fixture(case)
        assert set(now) == set(fx)
        for k in ("terms", "loss"):
            a, b = torch.from_numpy(np.asarray(now[k])).double(), fx[k].double()
            assert (a - b).abs().max().item() <= 1e-12 * max(b.abs().max().item(), 1e-300) or torch.equal(a, b), (case, k)
        assert torch.equal(torch.from_numpy(now["elements"]), fx["elements"])
        for k in ("g", "g_vec"):
            if k in fx:
                a, b = torch.from_numpy(now[k]).double(), fx[k].double()
                # (+ 1e-15: identical images leave 1e-19 of float64 noise that differs from host to host; every bound the
                #  tests derive is above 1e-10)
                assert (a - b).abs().max().item() <= 2e-7 * b.abs().max().item() + 1e-15, (case, k)
        if pc.CASES[case]["cls"] == "identical":  # pure float32 noise of the reference: its size, not its value, is reproducible
            assert 0 < float(now["ref32_grad_abs"]) <= 1e-9 and 0 < float(fx["ref32_grad_abs"]) <= 1e-9
            continue
        for k in ("ref32_value_dev", "ref32_grad_dev", "ref32_grad_abs"):  # (float32 sums depend on the host's threads)
            a, b = float(now[k]), float(fx[k])
            assert a <= 4 * b + 1e-12 and b <= 4 * a + 1e-12, (case, k, a, b)


def test_the_parity_profile_lists_every_case():
    """profiles/photometric_parity.json: the deviations measured on the MI355X beside the reference's own float32 ones."""
    with open(os.path.join(ROOT, "profiles", "photometric_parity.json")) as f:
        rows = json.load(f)["cases"]
    assert set(rows) == set(pc.CASES)
    for case, r in rows.items():
        fx = pc.load_fixture(case)
        assert r["ref32_grad_dev"] == pytest.approx(float(fx["ref32_grad_dev"]))
        assert r["ssim_dev"] <= max(1e-5, 4 * float(fx["ref32_value_dev"])) or pc.CASES[case]["cls"] == "identical"
