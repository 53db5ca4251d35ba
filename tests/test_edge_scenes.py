"""The rasterizer in the regimes no generated test scene reaches (tests/edge_scenes.py holds the cases and what makes each of
them one): saturated alpha (quirk Q1, the only place where the reference's backward recovers T by dividing by 1 - alpha =
0.01), the near cull at view_z <= 0.2 seen from a camera inside the scene, opacities on both sides of 1/255, zero
quaternions and zero scales, footprints wider than the image, clamped SH colours of degree 3, and a view batch one of whose
views has no instance at all.

Without a GPU, per case: the case is in its regime (edge_scenes.conditions), the float64 truth is structurally identical to
Oracle B (asserted while it is built), the fragile shares are within their caps, Oracle B's own statistics lie under the
ceilings -- the first check that Oracle A's Q1 / Q2 modelling agrees with the C restatement where the quirks fire -- and the
image yardstick is <= 1e-5.  On the GPU (marked gpu): the HIP path under the gates of test_gradient_truth (radii equal, then
images within min(FACTOR x yardstick, 1e-4) and gradients within FACTOR x yardstick per Gaussian), three cases under every
kernel variant, the view batch, markVisible, and the reference's own kernels live.  No bound is new.

Measured on an MI355X (profiles/edge_scenes_parity.jsonl): the HIP path at 0.95 .. 3.13 x the yardstick on
every tensor of every case and variant, the bound being 16 x.  The saturated cases first failed: means, scales, rotations,
opacities and means2D at 16 .. 140 x the yardstick, because the render backward formed "what lies behind a Gaussian" as a
difference of prefix sums; it now sums from the back (mgs_device.h, half_excl_suffix_add)."""
import pytest
import torch

import edge_scenes as es
import gradient_truth as gt
import util
from test_gradient_truth import _hip_scene, _need_gpu, _variants

gpu = pytest.mark.gpu


# ---- without a GPU --------------------------------------------------------------------------------------------------------

def _caps_and_ceilings(T):
    assert T.fragile_g.float().mean().item() <= gt.MAX_FRAGILE_GAUSSIANS
    assert T.fragile_px.float().mean().item() <= util.FRAGILE_MAX_FRACTION
    for k, (mx, p99) in gt.oracle_b_statistics(T).items():
        print(f"  Oracle B {k}: max {mx:.3g}, p99 {p99:.3g}")
        assert mx <= gt.CEILING_MAX and p99 <= gt.CEILING_P99, (k, mx, p99)
        assert T.yard[k][0] >= mx and T.yard[k][1] >= p99
    for n, yard in T.image_yard.items():
        assert yard <= 1e-5, (n, yard)


@pytest.mark.parametrize("name", es.CASES)
def test_case_is_in_its_regime_and_oracle_b_lies_under_the_ceilings(name):
    (sc, cam, kw, dC, dF), T = es.case_truth(name)       # (structural identity with Oracle B: asserted in there)
    assert sc["means3D"].shape[0] <= 3000 and kw["image_width"] <= 72 and kw["image_height"] <= 64
    print(f"  {name}: {es.conditions(name, sc, kw, T)}")
    _caps_and_ceilings(T)


def test_degenerate_covariance_stays_clear_of_the_fragile_cap():
    """The case sits nearest to MAX_FRAGILE_GAUSSIANS: with the reference alone at most half of it."""
    assert es.case_truth("degenerate_covariance")[1].fragile_g.float().mean().item() <= 0.01


def test_view_batch_has_a_view_without_instances_and_oracle_b_lies_under_the_ceilings():
    (sc, cams, kws, dC, dF), T = es.batch_truth()
    print(f"  {es.VIEW_BATCH}: {es.batch_conditions(sc, kws, T)}")
    _caps_and_ceilings(T)
    assert all(bool((g == 0).all()) for g in (T.grads["means2D"][2], T.b_grads["means2D"][2]))
    bg = torch.tensor(gt.BG, dtype=torch.float64).reshape(3, 1, 1)
    assert torch.equal(T.images["color"][2], bg.float().double().expand(3, 64, 64)) and not T.images["feature"][2].any()


# ---- on the GPU -----------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("name", es.CASES)
def test_hip_edge_case_per_gaussian_against_the_float64_truth(name):
    _need_gpu()
    s, T = es.case_truth(name)
    _hip_scene(f"edge/{name}", s, T)


@gpu
@pytest.mark.parametrize("variant", list(_variants()[0]))
def test_kernel_variants_on_the_edge_cases(variant):
    """Every per-call switch of test_gpu_parity.VARIANTS and both settings of tight_bins on the saturated MFMA-blend case,
    the near-plane case and the opacity band (where tight_bins drops the most instances)."""
    _lib = _need_gpu()
    variants, defaults = _variants()
    try:
        for k, v in variants[variant].items():
            _lib.set_option(k, v)
        for name in es.VARIANT_CASES:
            s, T = es.case_truth(name)
            _hip_scene(f"edge/{variant}/{name}", s, T)
    finally:
        for k, v in defaults.items():
            _lib.set_option(k, v)


@gpu
def test_view_batch_with_an_empty_view_against_the_float64_truth():
    """GaussianRasterizerBatch over a populated view, a view from inside the scene and a view that sees nothing: every view's
    images, every view's means2D gradient and the summed parameter gradients under the gates; the empty view is the
    background exactly and its means2D gradient is all zero."""
    _need_gpu()
    from test_gpu_parity import _run_batch
    (sc, cams, kws, dC, dF), T = es.batch_truth()
    cb, fb, rb, gb, m2b = _run_batch(sc, cams, dC, dF, gt.BG)
    assert torch.equal(rb, T.radii), "radii differ"
    T = gt.follow(T, cb, fb)
    for v in range(len(cams)):
        tag = f"edge/{es.VIEW_BATCH}/view{v}"
        gt.gate_image(tag, "color", cb[v], T.images["color"][v], T.fragile_px[v], T.image_yard["color"])
        gt.gate_image(tag, "feature", fb[v], T.images["feature"][v], T.fragile_px[v], T.image_yard["feature"])
    got = {util.GRAD_KEYS[k]: v for k, v in gb.items()}
    got.update({f"means2D[{v}]": m2b[v] for v in range(len(cams))})
    assert set(got) == set(T.yard), (sorted(got), sorted(T.yard))
    gt.gate_gradients(f"edge/{es.VIEW_BATCH}", T, got)
    assert torch.equal(cb[2], torch.tensor(gt.BG).reshape(3, 1, 1).expand(3, 64, 64)), "the empty view is not the background"
    assert not fb[2].any() and not m2b[2].any() and not rb[2].any()


@gpu
@pytest.mark.parametrize("neg", [True, False], ids=["negfocal", "posfocal"])
def test_mark_visible_on_the_near_plane_cloud(neg):
    """markVisible from the camera inside the scene equals oracle_b.mark_visible bit for bit: most of the cloud is behind
    the near plane, and the hand-placed rows at 0.2 -+ 1e-4 fall on either side of it."""
    _need_gpu()
    from manigaussian_amd import GaussianRasterizationSettings, GaussianRasterizer
    from manigaussian_amd import synthetic as syn
    from oracle import oracle_b
    sc, cam, kw, _, _ = es.scene("near_plane_negfocal" if neg else "near_plane_posfocal")
    dev = torch.device("cuda:0")
    r = GaussianRasterizer(GaussianRasterizationSettings(**syn.camera_settings_kwargs(cam, 1, True, device=dev)))
    got = r.markVisible(sc["means3D"].to(dev)).cpu()
    ref = oracle_b.mark_visible(sc["means3D"], kw["viewmatrix"], kw["projmatrix"])
    assert got.dtype == torch.bool and torch.equal(got, ref)
    assert got[:8].tolist() == [d > es.NEAR for d in es.AXIS_DEPTHS + es.AXIS_DEPTHS]
    assert 100 <= int(got.sum()) <= 1000      # (the depth test alone: 560 of the 2000)


@gpu
@pytest.mark.parametrize("name", es.CASES)
def test_edge_case_against_the_live_reference_kernels(name):
    """The HIP path against the reference's own kernels run live on this GPU (oracle/_ref, prebuilt; the reference tree is
    never read here), through test_gpu_parity._check_against_reference, and the instance count the binding returns against
    the reference's under tight_bins 0 and 1.  Skipped where the library was not built."""
    _need_gpu()
    from oracle import ref_cuda
    from test_gpu_parity import _check_against_reference, _num_rendered
    (sc, cam, kw, dC, dF), T = es.case_truth(name)
    F = sc["language_feature"].shape[1]
    if not ref_cuda.available(F):
        pytest.skip("oracle/_ref/libmgs_ref*.so not built (needs the reference tree at build time)")
    case = dict(sh_degree=kw["sh_degree"], include_feature=True, bg=gt.BG, scale_modifier=kw["scale_modifier"])
    cr, fr, rr, gr, R = util.run_reference(sc, kw, dC, dF)
    got = util.run_hip(sc, cam, dC, dF, case["sh_degree"], True, gt.BG, scale_modifier=case["scale_modifier"])
    _check_against_reference(got, (cr, fr, rr, gr), True, f"edge/{name}", state=T.states[0])
    counts = {tight: _num_rendered(sc, cam, case, tight) for tight in (0, 1)}
    util.report(f"edge/{name}", num_rendered_reference=int(R), num_rendered_tight0=counts[0], num_rendered_tight1=counts[1])
    assert counts[0] == counts[1] == int(R) == int(T.states[0].num_rendered), (counts, int(R), T.states[0].num_rendered)
