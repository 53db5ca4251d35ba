"""The rasterizer's gradients against a float64 truth, Gaussian by Gaussian (tests/gradient_truth.py holds the truth, the
measure and the cases).

Every other gate on these gradients is max |g - g_oracle| <= 1e-3 max |g_oracle| against a float32 oracle: one scalar per
tensor.  A Gaussian whose gradient is 1 % of the largest may be wrong by 10 % under it, and nobody knew the float32 rounding
budget of the gradients.  Here the truth is float64, the yardstick is what the two float32 oracles themselves deviate from
it, and the statistic is relative per Gaussian.

Without a GPU: Oracle A with record and pin off is bit-identical to what it was before it learned them; the pinned truth is
structurally identical to both float32 oracles in every case; pinning matters; the truth follows an implementation's
decision on a pair inside the 1/255 band; the measure sees two defects the tensor-wide gate passes.  On the GPU (marked gpu): the HIP path in every case, every kernel variant, view batches and a set batch.

Measured on an MI355X (profiles/gradient_truth.json): the HIP path at 0.17 .. 1.63 x the yardstick on every
tensor of every case, the bound being 16 x."""
import os
import types

import numpy as np
import pytest
import torch

import gradient_truth as gt
import util
from manigaussian_amd import synthetic as syn
from oracle import oracle_a

gpu = pytest.mark.gpu
IDENTITY = os.path.join(os.path.dirname(__file__), "golden", "oracle_a", "identity.npz")


# ---- without a GPU --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(gt.IDENTITY_CASES))
def test_oracle_a_is_bit_identical_with_record_and_pin_off(name):
    """oracle_a.forward_backward, record and pin off, against what it returned at the commit before it had them
    (tests/golden/oracle_a/identity.npz, written then by tests/golden/make_golden_oracle_a.py): every image, every gradient
    and the sorted list bit for bit, on the stored inputs.  Recording changes nothing either.  (Float32 bits follow the
    host's BLAS and math library, as tests/golden's other oracle vectors do: the file is from the development host.)"""
    z = np.load(IDENTITY)
    case = gt.IDENTITY_CASES[name]
    sc, cam, kw, dC, dF = util.scene_case(**case)
    sc = util.stored_inputs({k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + "/")}, sc)
    for record in (None, {}):
        c, f, r, g, aux = oracle_a.forward_backward(sc, types.SimpleNamespace(**kw), dC, dF, record=record)
        got = dict(out_color=c, out_feat=f, radii=r, point_list=aux["point_list"], n_contrib=aux["n_contrib"],
                   final_T=aux["final_T"], **{f"grad_{k}": v for k, v in g.items()})
        stored = {k[len(name) + 1:] for k in z.files if k.startswith(name + "/") and "/in_" not in k}
        assert stored == set(got)
        for k, v in got.items():
            ref = z[f"{name}/{k}"]
            assert v.numpy().dtype == ref.dtype and np.array_equal(v.numpy(), ref), (k, record is not None)


ALL_TRUTHS = [("case", n) for n in gt.CASES] + [("batch", n) for n in gt.VIEW_BATCHES]


@pytest.mark.parametrize("kind,name", ALL_TRUTHS, ids=[n for _, n in ALL_TRUTHS])
def test_truth_is_structurally_identical_and_oracle_b_lies_under_the_ceilings(kind, name):
    """Oracle B, the float32 Oracle A and the pinned float64 Oracle A take the same discrete decisions (asserted while the
    truth is built: sorted list, last contributor per pixel, radii, number of instances; the pinned run also finds the
    recorded radii and tile rectangles by itself), the fragile share is within its cap, and Oracle B's own statistics lie
    under a ceiling that catches a broken truth (CEILINGS, not contracts: about five times the measured values)."""
    T = (gt.case_truth if kind == "case" else gt.batch_truth)(name)[1]
    assert T.fragile_g.float().mean().item() <= gt.MAX_FRAGILE_GAUSSIANS
    if name.startswith("one_block"):
        assert int(T.fragile_px.sum()) <= 2       # at most 2 pixels (of 64: a share would read 3 %)
    else:
        assert T.fragile_px.float().mean().item() <= util.FRAGILE_MAX_FRACTION
    for k, (mx, p99) in gt.oracle_b_statistics(T).items():
        assert mx <= gt.CEILING_MAX and p99 <= gt.CEILING_P99, (k, mx, p99)
        assert T.yard[k][0] >= mx and T.yard[k][1] >= p99
    for n, yard in T.image_yard.items():
        assert yard <= 1e-5, (n, yard)


def test_unpinned_float64_sorts_the_translucent_list_differently():
    """Why the depth keys are pinned: a plain float64 run of the translucent case rounds float64 depths to the float32
    sort key and swaps near-ties of the long lists -- its sorted list is not Oracle B's, the pinned run's is."""
    (sc, cam, kw, dC, dF), T = gt.case_truth("translucent_long_lists_f3")
    plist = T.states[0].array("point_list")
    with torch.no_grad():
        aux = oracle_a.rasterize(sc["means3D"], sc["opacities"], types.SimpleNamespace(**kw), shs=sc["shs"],
                                 language_feature=sc["language_feature"], scales=sc["scales"], rotations=sc["rotations"],
                                 dtype=torch.float64)[3]
    assert aux["num_rendered"] == plist.size
    assert int((aux["point_list"].numpy() != plist).sum()) > 0


def test_the_truth_follows_an_implementation_s_decision_on_an_alpha_band_pair():
    """An 'implementation' that is the float32 Oracle A with ONE pair inside the 1/255 band decided the other way -- as
    correct as the recorded one.  Against the recorded truth it shows far outside the bound on Gaussians that are not marked
    fragile (everything blended at that pixel moves); follow() finds the pixel from the colour image alone, and against the
    followed truth the same gradients sit at the float32 oracle's own level."""
    name = "sh3_unnormalised_quat"
    (sc, cam, kw, dC, dF), T = gt.case_truth(name)
    o = T.views[0]
    assert o.pairs, "the case has no pair inside the alpha band any more: pick one that has"
    tile, row, j, y, x = o.pairs[0]
    pin = dict(o.rec, valid=dict(o.rec["valid"]), keep=dict(o.rec["keep"]))
    pin["valid"][tile], pin["keep"][tile] = o.rec["valid"][tile].clone(), o.rec["keep"][tile].clone()
    pin["valid"][tile][row, j] = ~pin["valid"][tile][row, j]
    pin["keep"][tile][row, j] = pin["valid"][tile][row, j]
    c, f, r, g, aux = oracle_a.forward_backward(sc, types.SimpleNamespace(**kw), dC, dF, pin=pin)
    got = gt._a_grads(g, T.b_grads, 1.0)
    Tf = gt.follow(T, c, f)
    assert Tf.followed == 1 and gt.follow(T, o.imgs["color"][2], o.imgs["feature"][2]) is T
    worst_before = max(gt.measure(got[k], T.grads[k], T.fragile_g)[0] / T.yard[k][0] for k in T.grads)
    assert worst_before > gt.FACTOR, worst_before
    for k in T.grads:
        mx, p99 = gt.measure(got[k], Tf.grads[k], T.fragile_g)
        a = gt.measure(T.a32_grads[k], T.grads[k], T.fragile_g)
        assert mx <= 2 * a[0] + 1e-12 and p99 <= 2 * a[1] + 1e-12, (k, mx, p99, a)


def _defects(b):
    """The two injected defects on one gradient tensor of Oracle B: every Gaussian whose gradient is below 1e-3 of the
    tensor's largest gets NO gradient; every 16th Gaussian's gradient is off by 1e-3 of itself."""
    s = b.abs().reshape(b.shape[0], -1).max(1)[0]
    zeroed = b.clone()
    zeroed[s < 1e-3 * s.max()] = 0
    scaled = b.clone()
    scaled[::16] *= 1.0 + 1e-3
    return {"small_gradients_zeroed": zeroed, "every_16th_off_by_1e-3": scaled}


def test_the_measure_sees_what_the_tensor_wide_gate_does_not():
    """Both defects pass max |g - g_B| <= 1e-3 max |g_B| on every tensor, and fail the per-Gaussian bound on every tensor
    (FACTOR x the unperturbed Oracle B's statistics) in the maximum or in the 99th percentile."""
    sc, cam, kw, dC, dF = gt.scene(gt.DEFECT_CASE)
    T = gt.truth(sc, kw, dC, dF)
    assert len(T.grads) >= 7
    for k, g64 in T.grads.items():
        b = T.b_grads[k]
        ymx, yp99 = gt.measure(b, g64, T.fragile_g)
        for name, bad in _defects(b).items():
            assert bool((bad != b).any()), (k, name)
            assert (bad - b).abs().max().item() <= 1e-3 * b.abs().max().item(), (k, name)           # today's gate: passes
            mx, p99 = gt.measure(bad, g64, T.fragile_g)
            print(f"  {k} {name}: max {mx:.3g} (bound {gt.FACTOR * ymx:.3g}), p99 {p99:.3g} (bound {gt.FACTOR * yp99:.3g})")
            assert mx > gt.FACTOR * ymx or p99 > gt.FACTOR * yp99, (k, name, mx, ymx, p99, yp99)    # the measure: fails


# ---- on the GPU -----------------------------------------------------------------------------------------------------------

def _need_gpu():
    from manigaussian_amd import _lib
    assert torch.cuda.is_available(), "-m gpu tests need a HIP device"
    L = _lib.lib()
    assert os.path.samefile(L._name, os.path.join(os.path.dirname(_lib.__file__), "libmgsplat.so"))
    return _lib


def _hip_scene(tag, s, T, few=None):
    """A scene tuple (sc, cam, kw, dC, dF) through util.run_hip under the options in force, gated against its truth T (few:
    the cap on the NUMBER of fragile pixels where a share of the image says nothing).  Returns what run_hip returned."""
    sc, cam, kw, dC, dF = s
    out = util.run_hip(sc, cam, dC, dF, kw["sh_degree"], bool(kw["include_feature"]), tuple(kw["bg"].tolist()),
                       scale_modifier=kw["scale_modifier"])
    _gate_scene(tag, s, T, out, few)
    return out


def _gate_scene(tag, s, T, out, few=None):
    """_hip_scene's gates on what a run of the scene returned, out = (color, feature, radii, gradients by leaf name) as
    util.run_hip returns them (tests/test_rasterizer_dirty_workspace.py gates its own runs with it)."""
    kw = s[2]
    inc = bool(kw["include_feature"])
    ch, fh, rh, gh = out
    assert torch.equal(rh, T.radii), "radii differ"
    T = gt.follow(T, ch, fh if inc else None)
    gt.gate_image(tag, "color", ch, T.images["color"], T.fragile_px, T.image_yard["color"], max_fragile_pixels=few)
    if inc:
        assert fh.shape == T.images["feature"].shape
        gt.gate_image(tag, "feature", fh, T.images["feature"], T.fragile_px, T.image_yard["feature"], max_fragile_pixels=few)
    else:
        assert fh.shape == (1,)
    got = {util.GRAD_KEYS[k]: v for k, v in gh.items() if util.GRAD_KEYS[k] in T.grads}
    assert set(got) == set(T.grads), (sorted(got), sorted(T.grads))
    gt.gate_gradients(tag, T, got)


def _hip_case(tag, name):
    """CASES[name] through the HIP path, gated against the shared truth."""
    s, T = gt.case_truth(name)
    kw, case = s[2], gt.CASES[name]
    assert (kw["sh_degree"], bool(kw["include_feature"]), kw["scale_modifier"]) == (
        case.get("sh_degree", 1), case.get("include_feature", True), case.get("scale_modifier", 1.0))
    _hip_scene(tag, s, T, few=2 if name.startswith("one_block") else None)  # the 8x8 image marks 2 of its 64 pixels


@gpu
@pytest.mark.parametrize("name", list(gt.CASES))
def test_hip_gradients_per_gaussian_against_the_float64_truth(name):
    _need_gpu()
    _hip_case(name, name)


def _variants():
    from test_gpu_parity import _DEFAULTS, VARIANTS
    return dict(VARIANTS, tight_bins_0=dict(tight_bins=0), tight_bins_1=dict(tight_bins=1)), _DEFAULTS


@gpu
@pytest.mark.parametrize("variant", list(_variants()[0]))
def test_kernel_variants_per_gaussian_against_the_float64_truth(variant):
    """Every per-call switch (MgsOptions) of test_gpu_parity.VARIANTS and both settings of tight_bins, on the MFMA-blend
    case and the precomputed-covariance case."""
    _lib = _need_gpu()
    variants, defaults = _variants()
    try:
        for k, v in variants[variant].items():
            _lib.set_option(k, v)
        for name in gt.VARIANT_CASES:
            _hip_case(f"{variant}/{name}", name)
    finally:
        for k, v in defaults.items():
            _lib.set_option(k, v)


@gpu
@pytest.mark.parametrize("name", list(gt.VIEW_BATCHES))
def test_view_batch_per_gaussian_against_the_float64_truth(name):
    """GaussianRasterizerBatch: the parameter gradients summed over the views and every view's means2D gradient, each under
    the measure; every view's images."""
    _need_gpu()
    from test_gpu_parity import _run_batch
    (sc, cams, dC, dF), T = gt.batch_truth(name)
    cb, fb, rb, gb, m2b = _run_batch(sc, cams, dC, dF, gt.BG)
    assert torch.equal(rb, T.radii), "radii differ"
    T = gt.follow(T, cb, fb)
    for v in range(len(cams)):
        gt.gate_image(f"{name}/view{v}", "color", cb[v], T.images["color"][v], T.fragile_px[v], T.image_yard["color"])
        gt.gate_image(f"{name}/view{v}", "feature", fb[v], T.images["feature"][v], T.fragile_px[v], T.image_yard["feature"])
    got = {util.GRAD_KEYS[k]: v for k, v in gb.items()}
    got.update({f"means2D[{v}]": m2b[v] for v in range(len(cams))})
    assert set(got) == set(T.yard), (sorted(got), sorted(T.yard))
    gt.gate_gradients(name, T, got)


def _through_normalise(f, g, dtype):
    """d/df of sum(g * f / (|f| + 1e-12)): render()'s feature normalisation, which sits between the leaf and the rasterizer."""
    x = f.detach().to(dtype).clone().requires_grad_(True)
    y = x / (x.norm(dim=-1, keepdim=True) + 1e-12)
    return torch.autograd.grad((y * g.to(dtype)).sum(), x)[0]


@gpu
def test_set_batch_per_gaussian_against_the_float64_truth():
    """render_sets_stacked: two DIFFERENT Gaussian sets of 2000, one view each, in one rasterizer call.  Each set has a truth
    of its own; the language-feature gradient reaches the leaf through render()'s normalisation, which the truth (float64)
    and the two yardstick oracles (float32) are taken through as well."""
    _need_gpu()
    from manigaussian_amd.gaussian_renderer import render_sets_stacked
    dev = torch.device("cuda:0")
    P, F, W = 2000, 3, 64
    cams = syn.circle_cameras(4, W, W, negative_focal=True)
    g = torch.Generator().manual_seed(8)
    dC, dF = torch.randn(2, 3, W, W, generator=g), torch.randn(2, F, W, W, generator=g)
    scs = [syn.make_scene(P, F=F, M=4, seed=11 + v) for v in range(2)]
    views = [cams[0], cams[2]]

    def data_of(cam):
        kw = syn.camera_settings_kwargs(cam, 1, True, device=dev)
        return {"novel_view": {"tanfov_host": [(kw["tanfovx"], kw["tanfovy"])], "size_host": [(W, W)],
                               "world_view_transform": kw["viewmatrix"][None], "full_proj_transform": kw["projmatrix"][None],
                               "camera_center": kw["campos"][None]}}

    leaves = [{k: v.to(dev).clone().requires_grad_(True) for k, v in sc.items()} for sc in scs]
    items = [(data_of(cam), 0, lv["means3D"], lv["rotations"], lv["scales"], lv["opacities"], None, lv["shs"],
              lv["language_feature"]) for cam, lv in zip(views, leaves)]
    outs, batch = render_sets_stacked(items, gt.BG)
    torch.autograd.backward([batch["render"], batch["render_embed"]], [dC.to(dev), dF.to(dev)])
    torch.cuda.synchronize()
    m2 = batch["viewspace_points"].grad.cpu()
    for v, (sc, cam, lv) in enumerate(zip(scs, views, leaves)):
        raw = sc["language_feature"]
        fed = dict(sc, language_feature=raw / (raw.norm(dim=-1, keepdim=True) + 1e-12))  # what the rasterizer is given
        kw = syn.camera_settings_kwargs(cam, 1, True, bg=gt.BG)
        T0 = gt.truth(fed, kw, dC[v], dF[v])
        T = gt.follow(T0, batch["render"][v].detach().cpu(), batch["render_embed"][v].detach().cpu())
        for grads in {id(d): d for d in (T0.grads, T0.b_grads, T0.a32_grads, T0.b_truth_grads, T.grads)}.values():
            lf = grads["language_feature"]
            grads["language_feature"] = _through_normalise(raw, lf, lf.dtype)
        T.yard = gt.yardsticks(T0)
        tag = f"set_batch/set{v}"
        assert torch.equal(batch["radii"][v].cpu(), T.radii), "radii differ"
        gt.gate_image(tag, "color", batch["render"][v].detach().cpu(), T.images["color"], T.fragile_px, T.image_yard["color"])
        gt.gate_image(tag, "feature", batch["render_embed"][v].detach().cpu(), T.images["feature"], T.fragile_px,
                      T.image_yard["feature"])
        got = {util.GRAD_KEYS[k]: t.grad.cpu() for k, t in lv.items()}
        got["means2D"] = m2[v]
        assert set(got) == set(T.grads), (sorted(got), sorted(T.grads))
        gt.gate_gradients(tag, T, got)
