"""Inputs, the float64 reference and the comparison of tests/test_losses.py -- TEST INFRASTRUCTURE, shared with
tests/golden/make_golden_loss.py (which records what `reference()` returns) so that the live reference and the committed
fixtures are checked by the same code.

The reference is the ManiGaussian code itself, executed unmodified through tests/ref_import.py: loss.py (l2_loss, cosine_loss),
NeuralRenderer._embed_loss_fn and PSNR_torch of neural_rendering.py, in float64, view by view, accumulated as
neural_rendering.py:305-329 does (loss = 0.; loss += w_rgb * l2; loss += w_embed * embed).
"""
import os
import types

import numpy as np
import torch

import ref_import

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_DIR = os.path.join(HERE, "golden", "loss")
COS_EPS = 1e-8
WHOLE_GRADIENT = ("static_v1",)  # fixtures keep whole gradients for these, pixel samples for the rest (size: see make_golden_loss.py)

MANI = [(1.0, 0.01), (0.01, 0.0)]
# name: V, H, W, F, embed_fn, layout of (gt_rgb, gt_embed) -- "last" [V,H,W,C], "first" [V,C,H,W], "view": a permuted
# (non-contiguous) view of the other layout --, weights, seed, offset (floats the image bases lie past a 16-byte boundary)
CASES = {
    "mani_step":        dict(V=2, H=128, W=128, F=3, fn="cosine", layout=("last", "first"), weights=MANI, seed=1),
    "mani_warmup":      dict(V=2, H=128, W=128, F=3, fn="cosine", layout=("last", "first"), weights=[(1.0, 0.01), (0.0, 0.0)], seed=1),
    "static_v1":        dict(V=1, H=128, W=128, F=3, fn="cosine", layout=("last", "first"), weights=[(1.0, 0.01)], seed=2),
    "v1_f32":           dict(V=1, H=128, W=128, F=32, fn="cosine", layout=("last", "first"), weights=[(1.0, 0.01)], seed=3),
    "v8_256_f32":       dict(V=8, H=256, W=256, F=32, fn="cosine", layout=("last", "last"), weights=None, seed=4),
    "odd_100x75_f5":    dict(V=2, H=100, W=75, F=5, fn="cosine", layout=("last", "first"), weights=MANI, seed=1),
    "offset_slice":     dict(V=2, H=128, W=128, F=3, fn="cosine", layout=("last", "first"), weights=MANI, seed=2, offset=1),
    "cosine_last":      dict(V=2, H=128, W=128, F=3, fn="cosine", layout=("last", "last"), weights=MANI, seed=3),
    "cosine_first":     dict(V=2, H=128, W=128, F=3, fn="cosine", layout=("first", "first"), weights=MANI, seed=3),
    "cosine_view":      dict(V=2, H=128, W=128, F=3, fn="cosine", layout=("view", "view"), weights=MANI, seed=3),
    "l2_last":          dict(V=2, H=128, W=128, F=3, fn="l2", layout=("last", "last"), weights=MANI, seed=4),
    "l2_first":         dict(V=2, H=128, W=128, F=3, fn="l2", layout=("first", "first"), weights=[(1.0, 0.01), (0.01, 0.5)], seed=4),
    "l2_norm_last":     dict(V=2, H=128, W=128, F=3, fn="l2_norm", layout=("last", "last"), weights=[(1.0, 0.01), (0.01, 0.5)], seed=1),
    "l2_norm_first":    dict(V=2, H=128, W=128, F=3, fn="l2_norm", layout=("first", "first"), weights=MANI, seed=2),
    "odd_f8_last":      dict(V=1, H=100, W=75, F=8, fn="cosine", layout=("last", "last"), weights=[(1.0, 0.01)], seed=4),
    "l2_f8_last":       dict(V=2, H=64, W=64, F=8, fn="l2", layout=("first", "last"), weights=MANI, seed=2),
    "l2_norm_odd_f5":   dict(V=1, H=100, W=75, F=5, fn="l2_norm", layout=("last", "first"), weights=[(1.0, 0.01)], seed=3),
}


def make_inputs(case):
    """CPU float32 tensors, the same on every machine: color [V,3,H,W] in [0,1), feature [V,F,H,W] = randn * 0.3 with the
    pixels of `rand < 0.3` exactly zero (a feature image gets no background: every pixel no Gaussian reaches is the zero
    vector) and three special pixels per view, targets in logical channel-last form gt_rgb [V,H,W,3], gt_embed [V,H,W,F].
    Returns the tensors and, per view, the flat indices of the special pixels."""
    c = CASES[case] if isinstance(case, str) else case
    V, H, W, F = c["V"], c["H"], c["W"], c["F"]
    N = H * W
    g = torch.Generator().manual_seed(c["seed"])
    color = torch.rand(V, 3, H, W, generator=g)
    gt_rgb = torch.rand(V, H, W, 3, generator=g)
    feature = torch.randn(V, F, H, W, generator=g) * 0.3
    gt_embed = torch.randn(V, H, W, F, generator=g)
    mask = torch.rand(V, H, W, generator=g) < 0.3
    feature = feature * (~mask).unsqueeze(1).float()
    special = []
    fl, ge = feature.view(V, F, N), gt_embed.view(V, N, F)
    for v in range(V):
        tiny, small, zt = (N // 7 + 3 * v) % N, (N // 3 + 5 * v) % N, (N // 2 + 11 * v) % N
        d = torch.randn(F, generator=g)
        d = d / d.norm()
        fl[v, :, tiny] = d * 1e-9          # |e_p| = 1e-9: below the eps clamp, both gradient terms live
        fl[v, :, small] = d * 2e-8         # just above the clamp
        ge[v, zt, :] = 0.0                 # a target pixel of zero norm
        if fl[v, :, zt].abs().sum() == 0:  # ... against a live feature pixel
            fl[v, :, zt] = d * 0.3
        special.append((tiny, small, zt))
    return dict(color=color, gt_rgb=gt_rgb, feature=feature, gt_embed=gt_embed), special


def assert_input_classes(case, inp, special):
    """The classes the generator claims (issue case 4), asserted on the tensors it made."""
    c = CASES[case] if isinstance(case, str) else case
    V, F, N = c["V"], c["F"], c["H"] * c["W"]
    n = inp["feature"].double().view(V, F, N).norm(dim=1)
    for v in range(V):
        zero = n[v] == 0
        share = zero.double().mean().item()
        assert 0.2 <= share <= 0.4, (v, share)
        assert zero.any() and (~zero).any()
        tiny, small, zt = special[v]
        assert abs(n[v, tiny].item() - 1e-9) < 1e-11 and 1e-8 < n[v, small].item() < 3e-8
        assert inp["gt_embed"].view(V, N, F)[v, zt].abs().sum().item() == 0 and n[v, zt].item() > 0
        other = ~zero
        other[tiny] = other[small] = False
        assert n[v][other].min().item() >= 1e-3, n[v][other].min().item()


def lay_out(t_last, layout):
    """The logical channel-last target [V,H,W,C] in the memory layout under test (same values)."""
    if layout == "last":
        return t_last.contiguous()
    if layout == "first":
        return t_last.permute(0, 3, 1, 2).contiguous()
    if layout == "view":  # channel-last shape over channel-first memory: a permuted view
        return t_last.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)
    raise ValueError(layout)


def have_reference():
    return not os.environ.get("MGS_LOSS_FIXTURES_ONLY") and ref_import.have_reference()


_REF = []


def reference_modules():
    if not _REF:
        loss_mod = ref_import._module("loss")
        nr = ref_import.load_neural_rendering()
        assert loss_mod is not None and nr is not None
        _REF.append((loss_mod, nr))
    return _REF[0]


def reference(case, inp, device="cpu"):
    """float64: terms [V,3] = (mse, embed, psnr), loss, d loss / d color [V,3,H,W], d loss / d feature [V,F,H,W]."""
    c = CASES[case] if isinstance(case, str) else case
    loss_mod, nr = reference_modules()
    V = c["V"]
    w = c["weights"] or [(1.0, 1.0)] * V
    col = inp["color"].to(device).double().requires_grad_(True)
    fea = inp["feature"].to(device).double().requires_grad_(True)
    gt_rgb, gt_emb = inp["gt_rgb"].to(device).double(), inp["gt_embed"].to(device).double()
    me = types.SimpleNamespace(loss_embed_fn=c["fn"])
    loss, terms = 0., []
    for v in range(V):
        x = col[v:v + 1].permute(0, 2, 3, 1)   # neural_rendering.py:285: channel-last, batch of 1
        e = fea[v:v + 1].permute(0, 2, 3, 1)
        l_rgb = loss_mod.l2_loss(x, gt_rgb[v:v + 1])
        psnr = nr.PSNR_torch(x, gt_rgb[v:v + 1])
        l_emb = nr.NeuralRenderer._embed_loss_fn(me, e, gt_emb[v:v + 1])
        loss += w[v][0] * l_rgb
        loss += w[v][1] * l_emb
        terms.append(torch.stack([l_rgb.detach(), l_emb.detach(), psnr.detach().double()]))
    loss.backward()
    return dict(terms=torch.stack(terms).cpu(), loss=loss.detach().cpu(), g_color=col.grad.cpu(), g_feature=fea.grad.cpu())


def sample_pixels(case, special):
    """Fixed pixel sample of a case's fixture: a stride through the image plus every special pixel."""
    c = CASES[case]
    N = c["H"] * c["W"]
    n = max(24, 6000 // (c["V"] * (3 + c["F"])))
    idx = set(range(5, N, max(1, N // n)))
    for s in special:
        idx.update(s)
    return torch.tensor(sorted(idx), dtype=torch.long)


def fixture_path(case):
    return os.path.join(GOLDEN_DIR, case + ".npz")


def to_fixture(case, ref, special):
    c = CASES[case]
    V, F, N = c["V"], c["F"], c["H"] * c["W"]
    px = torch.arange(N) if case in WHOLE_GRADIENT else sample_pixels(case, special)
    return dict(terms=ref["terms"].numpy(), loss=ref["loss"].numpy(), pixels=px.numpy().astype(np.int32),
                g_color=ref["g_color"].view(V, 3, N)[:, :, px].numpy().astype(np.float32),
                g_feature=ref["g_feature"].view(V, F, N)[:, :, px].numpy().astype(np.float32))


def load_fixture(case):
    z = np.load(fixture_path(case))
    return {k: torch.from_numpy(z[k]) for k in z.files}


def expected(case, inp, special, device="cpu"):
    """What to compare against: the live float64 reference over every pixel where a copy of the reference exists, else
    the committed fixture (recorded from the same computation) at its pixel sample."""
    c = CASES[case]
    V, F, N = c["V"], c["F"], c["H"] * c["W"]
    if have_reference():
        r = reference(case, inp, device)
        return dict(terms=r["terms"], loss=r["loss"], pixels=torch.arange(N), g_color=r["g_color"].view(V, 3, N),
                    g_feature=r["g_feature"].view(V, F, N), source="reference")
    f = load_fixture(case)
    return dict(terms=f["terms"], loss=f["loss"], pixels=f["pixels"].long(), g_color=f["g_color"].double(),
                g_feature=f["g_feature"].double(), source="fixture")


def compare(case, inp, got, exp, report=print):
    """got: loss (0-dim), terms [V,3] (mse, embed, psnr), g_color [V,3,H,W], g_feature [V,F,H,W] from the code under test
    (CPU tensors).  Prints every figure, then asserts the bounds of the issue:
      mse, embed, loss: relative 1e-5 to float64; psnr: absolute 1e-4 dB
      L2-type gradients: max |g - g64| <= 1e-5 max |g64| per tensor (per view: each view has its own weight)
      cosine gradients, per pixel: max_c |g - g64| <= 1e-5 w_embed / (N max(|e_p|, 1e-8))"""
    c = CASES[case]
    V, F, N = c["V"], c["F"], c["H"] * c["W"]
    w = c["weights"] or [(1.0, 1.0)] * V
    px = exp["pixels"]
    failures = []

    def rel(name, a, b):
        a, b = float(a), float(b)
        err = abs(a - b) / abs(b) if b != 0 else abs(a)
        report(f"  {case} {name}: got {a:.9g} want {b:.9g} rel {err:.3g}")
        if not err <= 1e-5:
            failures.append((name, a, b, err))

    rel("loss", got["loss"], exp["loss"])
    for v in range(V):
        rel(f"mse[{v}]", got["terms"][v, 0], exp["terms"][v, 0])
        rel(f"embed[{v}]", got["terms"][v, 1], exp["terms"][v, 1])
        d = abs(float(got["terms"][v, 2]) - float(exp["terms"][v, 2]))
        report(f"  {case} psnr[{v}]: got {float(got['terms'][v, 2]):.7f} want {float(exp['terms'][v, 2]):.7f} abs {d:.3g}")
        if not d <= 1e-4:
            failures.append((f"psnr[{v}]", d))
        gc, wc = got["g_color"].double().view(V, 3, N)[v][:, px], exp["g_color"][v]
        err, scale = (gc - wc).abs().max().item(), wc.abs().max().item()
        report(f"  {case} g_color[{v}]: max err {err:.3g} of max {scale:.3g} ({err / scale if scale else 0:.3g})")
        if not err <= 1e-5 * scale:
            failures.append((f"g_color[{v}]", err, scale))
        gf, wf = got["g_feature"].double().view(V, F, N)[v][:, px], exp["g_feature"][v]
        if c["fn"] == "cosine":
            n_e = inp["feature"].double().view(V, F, N)[v][:, px].norm(dim=0)
            bound = 1e-5 * w[v][1] / (N * n_e.clamp_min(COS_EPS))
            err = (gf - wf).abs().max(0)[0]
            worst = (err / bound.clamp_min(1e-300)).max().item() if w[v][1] else err.max().item()
            report(f"  {case} g_feature[{v}] (cosine, per pixel): worst err / bound {worst:.3g}; zero-norm pixels "
                   f"{int((n_e == 0).sum())} with |g| {wf[:, n_e == 0].abs().max().item() if (n_e == 0).any() else 0:.3g}")
            if not bool((err <= bound).all()):
                failures.append((f"g_feature[{v}]", worst))
        else:
            err, scale = (gf - wf).abs().max().item(), wf.abs().max().item()
            report(f"  {case} g_feature[{v}]: max err {err:.3g} of max {scale:.3g} ({err / scale if scale else 0:.3g})")
            if not err <= 1e-5 * scale:
                failures.append((f"g_feature[{v}]", err, scale))
    assert not failures, (case, exp["source"], failures)
