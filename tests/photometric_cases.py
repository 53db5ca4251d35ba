"""Inputs, the float64 reference and the comparison of tests/test_photometric.py -- TEST INFRASTRUCTURE, shared with
tests/golden/make_golden_photometric.py (which records what `reference()` returns) so that the live reference and the
committed fixtures are checked by the same code.

The reference is the ManiGaussian code itself, executed unmodified through tests/ref_import.py: loss.py's l1_loss, l2_loss,
ssim and psnr in float64, view by view, with autograd gradients, accumulated as the loss is specified:
loss = 0.; loss += w_l1 * l1; loss += w_l2 * l2; loss += w_ssim * (1 - ssim).

Tolerances.  SSIM's G*x^2 - mu^2 cancels in float32, by an amount that depends on the images, so the fixture generator
records per case how far the reference's OWN float32 evaluation is from its float64 one (`ref32_value_dev`: max |ssim32 -
ssim64| over the views; `ref32_grad_dev`: max over the views of max |g32 - g64| / max |g64|).  The code under test must be
within max(1e-5, 4 x that) of float64 in the same units: 1e-5 is the loss tests' allowance for another summation order, the
factor 4 covers the separable two-pass rounding against the reference's one-pass 121-tap sum.  l1, l2: 1e-5 relative; psnr:
1e-4 dB.  The loss is a weighted sum of the terms, so its bound is the same sum of the terms' bounds.
"""
import math
import os

import numpy as np
import torch

import ref_import

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_DIR = os.path.join(HERE, "golden", "photometric")
WHOLE_LIMIT = 20000      # fixtures keep a view's whole gradient up to this many elements, a sample of SAMPLE beyond
SAMPLE = 4000
ULP1 = 2.0 ** -23        # float32 ulp at 1

MANI = [(1.0, 0.0, 0.2), (0.01, 0.0, 0.0)]
# name: V, C, H, W, input class, target layout ("last" [V,H,W,C], "first" [V,C,H,W], "view": channel-last shape over
# channel-first memory, a permuted non-contiguous view), weights, seed, offset (floats the bases lie past a 16-byte boundary),
# ssim_vec: the upstream vector of the `ssim(..., size_average=False)` test
CASES = {
    "tiny_8x5":      dict(V=1, C=3, H=5, W=8, cls="uniform", layout="first", weights=None, seed=1),
    "win_11x11":     dict(V=1, C=1, H=11, W=11, cls="uniform", layout="last", weights=[(0.8, 0.5, 0.2)], seed=2),
    "odd_37x23":     dict(V=2, C=3, H=23, W=37, cls="smooth", layout="last", weights=[(0.8, 0.0, 0.2), (0.3, 1.0, 0.5)], seed=3,
                          ssim_vec=(0.7, -1.3)),
    "tiles_70x45":   dict(V=1, C=3, H=45, W=70, cls="black", layout="view", weights=[(0.8, 0.0, 0.2)], seed=4),
    "odd_100x75":    dict(V=2, C=3, H=75, W=100, cls="equal30", layout="first", weights=[(1.0, 0.0, 0.0), (0.5, 0.25, 1.0)], seed=5),
    "mani_128":      dict(V=2, C=3, H=128, W=128, cls="smooth", layout="last", weights=MANI, seed=6),
    "feat_64_c32":   dict(V=1, C=32, H=64, W=64, cls="uniform", layout="first", weights=[(0.8, 0.0, 0.2)], seed=7),
    "offset_slice":  dict(V=2, C=3, H=24, W=40, cls="smooth", layout="first", weights=None, seed=8, offset=1),
    "black_128":     dict(V=1, C=3, H=128, W=128, cls="black", layout="last", weights=[(0.8, 0.0, 0.2)], seed=9),
    "identical_128": dict(V=1, C=3, H=128, W=128, cls="identical", layout="first", weights=None, seed=10),
}


def make_inputs(case):
    """CPU float32 tensors, the same on every machine: color [V,C,H,W] and the target in logical channel-first form."""
    c = CASES[case] if isinstance(case, str) else case
    V, C, H, W = c["V"], c["C"], c["H"], c["W"]
    g = torch.Generator().manual_seed(c["seed"])
    cls = c["cls"]
    if cls == "uniform":
        x, y = torch.rand(V, C, H, W, generator=g), torch.rand(V, C, H, W, generator=g)
    elif cls == "smooth":  # a low-frequency image plus a little noise on either side: G*x^2 - mu^2 cancels
        yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
        ph = torch.rand(V, C, 1, 1, generator=g) * 6.28
        base = 0.5 + 0.3 * torch.sin(xx / 17.0 + ph) * torch.cos(yy / 13.0 - ph)
        x = base + 0.02 * torch.randn(V, C, H, W, generator=g)
        y = base + 0.02 * torch.randn(V, C, H, W, generator=g)
    elif cls == "black":   # a render on a black background against a bright target: sigma is exactly 0 over regions
        x, y = torch.zeros(V, C, H, W), torch.ones(V, C, H, W)
        x[:, :, H // 3:H // 3 + 9, W // 4:W // 4 + 13] = torch.rand(V, C, 9, 13, generator=g)
        y[:, :, H // 2:H // 2 + 7, W // 2:W // 2 + 10] = torch.rand(V, C, 7, 10, generator=g)
    elif cls == "equal30":  # 30 % of the pixels exactly equal to the target: the L1 gradient is exactly 0 there
        x, y = torch.rand(V, C, H, W, generator=g), torch.rand(V, C, H, W, generator=g)
        same = torch.rand(V, C, H, W, generator=g) < 0.3
        y = torch.where(same, x, y)
    elif cls == "identical":
        x = torch.rand(V, C, H, W, generator=g)
        y = x.clone()
    else:
        raise ValueError(cls)
    return dict(color=x.contiguous(), target=y.contiguous())


def assert_input_classes(case, inp):
    """The classes the generator claims, asserted on the tensors it made."""
    c = CASES[case] if isinstance(case, str) else case
    x, y = inp["color"], inp["target"]
    cls = c["cls"]
    if cls == "uniform":
        assert 0.0 <= x.min() and x.max() < 1.0 and (x != y).all() and x.std() > 0.2
    elif cls == "smooth":
        assert (x - y).abs().max() < 0.2 and x.max() - x.min() > 0.3 and (x != y).float().mean() > 0.99
    elif cls == "black":
        assert (x == 0).float().mean() > 0.5 and (y == 1).float().mean() > 0.5 and (x > 0).any() and (y < 1).any()
        both = ((x == 0) & (y == 1)).float()  # an 11 x 11 window somewhere sees constants only: sigma exactly 0
        assert torch.nn.functional.avg_pool2d(both, 11, stride=1).max() == 1.0 or min(c["H"], c["W"]) < 11
    elif cls == "equal30":
        share = (x == y).float().mean().item()
        assert 0.25 <= share <= 0.35, share
    elif cls == "identical":
        assert torch.equal(x, y)


def lay_out(t_first, layout):
    """The logical channel-first target [V,C,H,W] in the memory layout under test (same values), as the caller passes it."""
    if layout == "first":
        return t_first.contiguous()
    if layout == "last":
        return t_first.permute(0, 2, 3, 1).contiguous()
    if layout == "view":  # channel-last shape over channel-first memory: a permuted view
        return t_first.contiguous().permute(0, 2, 3, 1)
    raise ValueError(layout)


def have_reference():
    return not os.environ.get("MGS_PHOTOMETRIC_FIXTURES_ONLY") and ref_import.have_reference()


def reference_module():
    m = ref_import._module("loss")
    assert m is not None
    return m


def weights_of(c):
    return c["weights"] or [(1.0, 1.0, 1.0)] * c["V"]


def reference(case, inp, dtype=torch.float64):
    """terms [V,4] = (l1, l2, ssim, psnr), loss, d loss / d color [V,C,H,W]; with `ssim_vec` also g_vec = d (sum_v u[v]
    ssim[v]) / d color.  loss.py's own functions, unmodified, in `dtype`, on the CPU."""
    c = CASES[case] if isinstance(case, str) else case
    m = reference_module()
    V, w = c["V"], weights_of(c)
    col = inp["color"].to(dtype).requires_grad_(True)
    tgt = inp["target"].to(dtype)
    loss, terms, vec = 0., [], 0.
    u = c.get("ssim_vec")
    for v in range(V):
        x, y = col[v:v + 1], tgt[v:v + 1]
        l1, l2, ss = m.l1_loss(x, y), m.l2_loss(x, y), m.ssim(x, y)
        psnr = m.psnr(x, y).reshape(()) if l2.item() != 0 else torch.tensor(100.0, dtype=dtype)
        loss += w[v][0] * l1
        loss += w[v][1] * l2
        loss += w[v][2] * (1 - ss)
        if u:
            vec = vec + u[v] * ss
        terms.append(torch.stack([l1.detach(), l2.detach(), ss.detach(), psnr.detach().to(dtype)]))
    g, = torch.autograd.grad(loss, [col], retain_graph=bool(u))
    out = dict(terms=torch.stack(terms), loss=loss.detach(), g=g)
    if u:
        out["g_vec"], = torch.autograd.grad(vec, [col])
    return out


def ref32_deviation(case, inp, r64):
    """How far the reference's own float32 evaluation is from its float64 one: (max |ssim32 - ssim64|, max over views of
    max |g32 - g64| / max |g64|, max |g32 - g64|)."""
    c = CASES[case]
    r32 = reference(case, inp, torch.float32)
    value = (r32["terms"][:, 2].double() - r64["terms"][:, 2]).abs().max().item()
    rel, absolute = 0.0, 0.0
    for k in ("g", "g_vec"):
        if k not in r64:
            continue
        for v in range(c["V"]):
            d = (r32[k][v].double() - r64[k][v]).abs().max().item()
            scale = r64[k][v].abs().max().item()
            absolute = max(absolute, d)
            if scale > 0 and c["cls"] != "identical":
                rel = max(rel, d / scale)
    return value, rel, absolute


def sample_elements(case):
    """Flat indices into one view's [C,H,W] gradient that a fixture keeps: all of them, or a fixed odd stride through them."""
    c = CASES[case]
    n = c["C"] * c["H"] * c["W"]
    if n <= WHOLE_LIMIT:
        return torch.arange(n)
    return torch.arange(3, n, (n // SAMPLE) | 1)


def fixture_path(case):
    return os.path.join(GOLDEN_DIR, case + ".npz")


def to_fixture(case, inp, ref):
    c = CASES[case]
    V = c["V"]
    px = sample_elements(case)
    value, rel, absolute = ref32_deviation(case, inp, ref)
    fx = dict(terms=ref["terms"].numpy(), loss=ref["loss"].numpy(), elements=px.numpy().astype(np.int32),
              g=ref["g"].reshape(V, -1)[:, px].numpy().astype(np.float32),
              ref32_value_dev=np.float64(value), ref32_grad_dev=np.float64(rel), ref32_grad_abs=np.float64(absolute))
    if "g_vec" in ref:
        fx["g_vec"] = ref["g_vec"].reshape(V, -1)[:, px].numpy().astype(np.float32)
    return fx


def load_fixture(case):
    z = np.load(fixture_path(case))
    return {k: torch.from_numpy(np.asarray(z[k])) for k in z.files}


_EXPECTED = {}


def expected(case):
    """What to compare against (computed once per case and shared, never modified): the live float64 reference over every
    element where a copy of the reference exists, else the committed fixture (recorded from the same computation) at its
    elements.  The recorded float32 deviations of the reference always come from the fixture."""
    if case in _EXPECTED:
        return _EXPECTED[case]
    c = CASES[case]
    V, n = c["V"], c["C"] * c["H"] * c["W"]
    f = load_fixture(case)
    e = dict(ref32_value_dev=float(f["ref32_value_dev"]), ref32_grad_dev=float(f["ref32_grad_dev"]),
             ref32_grad_abs=float(f["ref32_grad_abs"]))
    if have_reference():
        r = reference(case, make_inputs(case))
        e.update(terms=r["terms"], loss=r["loss"], elements=torch.arange(n), g=r["g"].reshape(V, n), source="reference")
        if "g_vec" in r:
            e["g_vec"] = r["g_vec"].reshape(V, n)
    else:
        e.update(terms=f["terms"], loss=f["loss"], elements=f["elements"].long(), g=f["g"].double(), source="fixture")
        if "g_vec" in f:
            e["g_vec"] = f["g_vec"].double()
    _EXPECTED[case] = e
    return e


def ssim_bounds(exp):
    """(bound on |ssim - ssim64|, bound on max |g - g64| in units of max |g64|)"""
    return max(1e-5, 4 * exp["ref32_value_dev"]), max(1e-5, 4 * exp["ref32_grad_dev"])


def compare_gradient(case, name, g, want, exp, failures, measured, report=print):
    """g [V,C,H,W] from the code under test against want [V, elements]: per view (each has its own weights), every element."""
    c = CASES[case]
    V = c["V"]
    _, tol_g = ssim_bounds(exp)
    got = g.double().reshape(V, -1)[:, exp["elements"]]
    worst = 0.0
    for v in range(V):
        err, scale = (got[v] - want[v]).abs().max().item(), want[v].abs().max().item()
        if c["cls"] == "identical":  # an absolute case: 4 x the noise the reference's own float32 run leaves
            bound = 4 * exp["ref32_grad_abs"]
            report(f"  {case} {name}[{v}]: max |g| {got[v].abs().max().item():.3g} (float64 {scale:.3g}), bound {bound:.3g}")
        else:
            bound = tol_g * scale
            report(f"  {case} {name}[{v}]: max err {err:.3g} of max {scale:.3g} ({err / scale if scale else 0:.3g}), "
                   f"bound {tol_g:.3g} (reference float32: {exp['ref32_grad_dev']:.3g})")
            worst = max(worst, err / scale if scale else err)
        if not err <= bound:
            failures.append((f"{name}[{v}]", err, scale, bound))
    measured[name + "_dev"] = worst


def compare(case, got, exp, report=print):
    """got: loss (0-dim), terms [V,4] (l1, l2, ssim, psnr), g [V,C,H,W] from the code under test (CPU tensors).  Prints every
    figure, then asserts the bounds in this module's docstring.  Returns the measured deviations."""
    c = CASES[case]
    V, w = c["V"], weights_of(c)
    tol_s, _ = ssim_bounds(exp)
    failures, measured = [], {}
    loss_bound, worst_s = 0.0, 0.0
    for v in range(V):
        t, e = got["terms"][v].double(), exp["terms"][v].double()
        if c["cls"] == "identical":
            report(f"  {case} terms[{v}]: l1 {t[0].item():.3g} l2 {t[1].item():.3g} ssim - 1 {t[2].item() - 1:.3g} psnr {t[3].item():.6g}")
            if not (t[0] == 0 and t[1] == 0 and t[3] == 100 and abs(t[2].item() - 1) <= 4 * ULP1):
                failures.append((f"terms[{v}]", t.tolist()))
            loss_bound += abs(w[v][2]) * 4 * ULP1
            continue
        for i, name in ((0, "l1"), (1, "l2")):
            err = abs(t[i].item() - e[i].item()) / abs(e[i].item())
            report(f"  {case} {name}[{v}]: got {t[i].item():.9g} want {e[i].item():.9g} rel {err:.3g}")
            if not err <= 1e-5:
                failures.append((f"{name}[{v}]", err))
            loss_bound += abs(w[v][i]) * 1e-5 * abs(e[i].item())
        d = abs(t[2].item() - e[2].item())
        worst_s = max(worst_s, d)
        report(f"  {case} ssim[{v}]: got {t[2].item():.9g} want {e[2].item():.9g} abs {d:.3g}, bound {tol_s:.3g} "
               f"(reference float32: {exp['ref32_value_dev']:.3g})")
        if not d <= tol_s:
            failures.append((f"ssim[{v}]", d, tol_s))
        loss_bound += abs(w[v][2]) * tol_s
        d = abs(t[3].item() - e[3].item())
        report(f"  {case} psnr[{v}]: got {t[3].item():.7f} want {e[3].item():.7f} abs {d:.3g}")
        if not d <= 1e-4:
            failures.append((f"psnr[{v}]", d))
    measured["ssim_dev"] = worst_s
    d = abs(float(got["loss"]) - float(exp["loss"]))
    report(f"  {case} loss: got {float(got['loss']):.9g} want {float(exp['loss']):.9g} abs {d:.3g}, bound {loss_bound:.3g}")
    if not d <= loss_bound:
        failures.append(("loss", d, loss_bound))
    compare_gradient(case, "g", got["g"], exp["g"], exp, failures, measured, report)
    assert not failures, (case, exp["source"], failures)
    assert math.isfinite(float(got["loss"]))
    return measured
