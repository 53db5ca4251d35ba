"""A float64 truth for the rasterizer's images and gradients, and a per-Gaussian measure against it.

The truth is Oracle A (oracle/oracle_a.py: pure torch, backward from autograd) run in float64 with its DISCRETE decisions
pinned to those of a float32 run of itself: the float32 depth that enters the sort key (a z computed in float64 and then
rounded differs in the last bit from a z computed in float32, and near-ties of a long list swap) and, per tile, which pairs
pass alpha >= 1/255 and which are blended before the pixel stops.  That float32 run is first checked to be structurally
identical to Oracle B (the C restatement of the reference): the same sorted list, the same last contributor per pixel, the
same radii.  (It sorts by Oracle B's float32 depths: its own come out of a torch matrix product whose last bit follows the
host's BLAS.)  Everything smooth is float64.  Radii and tile rectangles are not pinned: the pinned run asserts that it finds
them itself.  One kind of decision is the implementation's to take -- a pair whose alpha lies within 2e-5 of 1/255 -- and
there the truth follows it: follow().

THE MEASURE, per gradient tensor, Gaussians along dimension 0, threshold-fragile Gaussians left out:
    e_i = max over a Gaussian's entries of |g - g64|
    s_i = max over its entries of |g64|
    r_i = e_i / (s_i + DELTA * max_j s_j),   DELTA = 1e-4
gated on max_i r_i and on the 99th percentile of r_i.  A Gaussian whose gradient reaches down to 1e-4 of the tensor's largest
is held to a RELATIVE bound; below that the bound turns absolute, at a level ten times finer than 1e-3 of the maximum.
THE YARDSTICK is the same pair of statistics for Oracle B and for the float32 Oracle A against the same truth (each under
its own decisions on the pairs just named), the larger of the two per tensor and per case, computed live and never from the HIP result; the HIP path must stay within FACTOR = 16 times
it (the package's standing margin for another summation order, fused multiply-adds and float atomics:
spatial_softmax_cases.FACTOR).  Fragile Gaussians (oracle_b.fragile_gaussians at 2e-5) keep the tensor-wide
util.FRAGILE_GRAD_TOL, and their share is capped at MAX_FRAGILE_GAUSSIANS per case.

Plain module beside util.py: tests/test_gradient_truth.py holds the tests."""
import functools
import types

import numpy as np
import torch

import util
from manigaussian_amd import synthetic as syn
from oracle import oracle_a, oracle_b
from spatial_softmax_cases import FACTOR

DELTA = 1e-4
REL_EPS = 2e-5
MAX_FRAGILE_GAUSSIANS = 0.02
IMG_CONTRACT = 1e-4            # the bound on an image never exceeds the package's contract, whatever the yardstick says
# ceilings on Oracle B's OWN statistics against the truth (about five times what the cases below measure): not contracts,
# they catch a broken truth -- a pin that no longer pins shows as 1e-2 .. 1 here
CEILING_MAX, CEILING_P99 = 1e-2, 1e-3

# Oracle A's gradient names -> Oracle B's
_A2B = {"shs": "sh", "cov3D_precomp": "cov3D"}

BG = (0.1, 0.2, 0.3)

# The smallest shapes that still cross each seam of the kernels (opacity_scale / opacity_fill edit the generated scene).
CASES = {
    "production_16k_f3_negfocal": dict(P=16384, F=3),
    "mfma_blend_f32": dict(P=6000, F=32),
    "padded_width_f5": dict(P=2000, F=5, W=64, H=64),
    "partial_blocks_17x33_f64": dict(P=70, F=64, W=17, H=33),
    "precomp_rgb_no_feature": dict(P=1000, F=3, colors_precomp=True, include_feature=False, W=64, H=64),
    "sh3_unnormalised_quat": dict(P=800, F=3, M=16, sh_degree=3, unnormalized_rot=True, W=64, H=64),
    "cov3d_precomp_72x40": dict(P=600, F=3, cov3d=True, W=72, H=40),
    "scale_modifier_1p7": dict(P=1500, F=3, W=64, H=64, scale_modifier=1.7),
    "black_background_posfocal_f32": dict(P=1200, F=32, W=48, H=48, neg=False, bg=(0.0, 0.0, 0.0)),
    "translucent_long_lists_f3": dict(P=30000, F=3, W=32, H=32, opacity_scale=0.1),
    "translucent_long_lists_f32": dict(P=30000, F=32, W=32, H=32, opacity_scale=0.1),
    "one_block_40k_f32_8x8": dict(P=40000, F=32, W=8, H=8, opacity_fill=0.0045),
}
VARIANT_CASES = ("mfma_blend_f32", "cov3d_precomp_72x40")
VIEW_BATCHES = {"3_views_f3_72x40": dict(P=3000, F=3, V=3, W=72, H=40), "4_views_f32_128": dict(P=6000, F=32, V=4, W=128, H=128)}
DEFECT_CASE = dict(P=1500, F=3, W=64, H=64)
IDENTITY_CASES = {
    "sh1_f3_negfocal_48x40": dict(P=300, F=3, W=48, H=40),
    "cov3d_f5_precomp_posfocal_33x17": dict(P=150, F=5, W=33, H=17, neg=False, cov3d=True, colors_precomp=True),
}


def scene(case):
    """util.scene_case plus the two scene edits of the long-list cases: (sc, cam, kw, dC, dF)."""
    case = dict(case)
    scale, fill = case.pop("opacity_scale", None), case.pop("opacity_fill", None)
    sc, cam, kw, dC, dF = util.scene_case(**case)
    if scale is not None:
        sc["opacities"] = (sc["opacities"] * scale).contiguous()
    if fill is not None:
        sc["opacities"] = torch.full_like(sc["opacities"], fill)
    return sc, cam, kw, dC, dF


# ---- the measure ----------------------------------------------------------------------------------------------------------

def per_gaussian(g, g64):
    """r_i of the module docstring, float64 [P] (0 where a Gaussian and the whole tensor are exactly zero on both sides)."""
    g64 = g64.double()
    n = g64.shape[0]
    e = (g.double().reshape(g64.shape) - g64).abs().reshape(n, -1).max(1)[0]
    s = g64.abs().reshape(n, -1).max(1)[0]
    den = s + DELTA * s.max()
    return torch.where(den > 0, e / den.clamp_min(1e-300), torch.where(e > 0, torch.full_like(e, float("inf")), e))


def measure(g, g64, fragile):
    """(max, 99th percentile) of r_i over the Gaussians not marked fragile."""
    r = per_gaussian(g, g64)[~fragile]
    if r.numel() == 0:
        return 0.0, 0.0
    return r.max().item(), torch.quantile(r, 0.99).item()


def fragile_error(g, g64, fragile):
    """(max |g - g64| over the fragile Gaussians, max |g64|): what util.FRAGILE_GRAD_TOL is applied to."""
    g64 = g64.double()
    e = (g.double().reshape(g64.shape) - g64).abs().reshape(g64.shape[0], -1).max(1)[0]
    return (e[fragile].max().item() if fragile.any() else 0.0), g64.abs().max().item()


def oracle_b_statistics(T):
    """{name: (max, p99)} of Oracle B against the truth under Oracle B's own decisions (T.b_truth_grads: follow())."""
    out = {}
    for k, g64 in T.b_truth_grads.items():
        if k == "means2D" and g64.dim() == 3:
            out.update({f"means2D[{v}]": measure(T.b_grads[k][v], g64[v], T.fragile_g) for v in range(g64.shape[0])})
        else:
            out[k] = measure(T.b_grads[k], g64, T.fragile_g)
    return out


def yardsticks(T):
    """{name: (max, p99)}: the larger of Oracle B's and the float32 Oracle A's statistics, per tensor, each against the
    truth under its own decisions (the float32 Oracle A's are the pinned ones).  means2D of a view batch is measured view
    by view ("means2D[v]")."""
    out = oracle_b_statistics(T)
    for k, g64 in T.grads.items():
        if k == "means2D" and g64.dim() == 3:
            for v in range(g64.shape[0]):
                a, b = measure(T.a32_grads[k][v], g64[v], T.fragile_g), out[f"means2D[{v}]"]
                out[f"means2D[{v}]"] = (max(b[0], a[0]), max(b[1], a[1]))
            continue
        a, b = measure(T.a32_grads[k], g64, T.fragile_g), out[k]
        out[k] = (max(b[0], a[0]), max(b[1], a[1]))
    return out


# ---- the truth ------------------------------------------------------------------------------------------------------------

def structurally_identical(aux, radii, st, radii_b):
    """The structural checks of test_oracle._ab between a run of Oracle A and Oracle B's state."""
    assert aux["num_rendered"] == st.num_rendered
    assert np.array_equal(aux["point_list"].numpy(), st.array("point_list"))
    assert np.array_equal(aux["n_contrib"].numpy().ravel(), st.array("n_contrib"))
    assert torch.equal(radii, radii_b)


def _a_grads(ga, like, mod):
    """Oracle A's gradients under Oracle B's names and in the reference's conventions: the reference's dL/dscale omits the
    scale_modifier its forward applies (backward.cu:295,325-327), autograd's carries it (test_oracle.py, third quirk)."""
    out = {}
    for k, v in ga.items():
        key = _A2B.get(k, k)
        if v.numel() == 0 or key not in like:
            continue
        out[key] = v / mod if key == "scales" else v
    return out


def _one_view(sc, kw, dC, dF):
    st_ = types.SimpleNamespace(**kw)
    inc = bool(kw["include_feature"])
    mod = float(kw.get("scale_modifier", 1.0))
    cb, fb, rb, gb, st = util.run_oracle_b(sc, kw, dC, dF)
    # The float32 run sorts by Oracle B's float32 depths: its own come out of a torch matrix product whose last bit follows
    # the host's BLAS, and on some hosts near-ties of the long lists then swap against Oracle B's (seen on an MI355X host).
    rec = {}
    depth_b = torch.from_numpy(np.ascontiguousarray(st.array("depths"), dtype=np.float32))
    c32, f32, r32, g32, aux32 = oracle_a.forward_backward(sc, st_, dC, dF if inc else None, record=rec,
                                                          pin={"depth_key": depth_b})
    structurally_identical(aux32, r32, st, rb)

    def run64(pin, backward=True):
        """The pinned float64 run: (color, feature, gradients under Oracle B's names), forward only on request."""
        if not backward:
            with torch.no_grad():
                c, f, _, _ = oracle_a.rasterize(
                    sc["means3D"], sc["opacities"], st_, shs=sc.get("shs"), colors_precomp=sc.get("colors_precomp"),
                    language_feature=sc.get("language_feature"), scales=sc.get("scales"), rotations=sc.get("rotations"),
                    cov3D_precomp=sc.get("cov3D_precomp"), dtype=torch.float64, pin=pin)
            return c, f, None
        c, f, r, g, aux = oracle_a.forward_backward(sc, st_, dC, dF if inc else None, dtype=torch.float64, pin=pin)
        if pin is rec:  # (under follow()'s edited pins a flipped pair may be a pixel's last contributor)
            structurally_identical(aux, r, st, rb)
        return c, f, _a_grads(g, gb, mod)

    c64, f64, t64 = run64(rec)
    a32 = _a_grads(g32, gb, mod)
    b = {k: gb[k].reshape(t64[k].shape) for k in t64}
    imgs = {"color": (c64, cb, c32)}
    if inc:
        imgs["feature"] = (f64, fb, f32)
    o = types.SimpleNamespace(imgs=imgs, grads=t64, b_grads=b, a32_grads=a32, radii=rb, state=st, aux32=aux32, rec=rec,
                              run64=run64, fragile_px=oracle_b.fragile_mask(st, REL_EPS),
                              fragile_g=oracle_b.fragile_gaussians(st, REL_EPS))
    o.pairs = _alpha_band_pairs(o)
    return o


def _alpha_band_pairs(o):
    """[(tile, row in the tile, position in the tile's list, y, x)]: the pairs whose alpha lies within REL_EPS of 1/255 by
    Oracle B's own test (mgs_oracle.c orc_fragile_mask, evaluated here on Oracle B's float32 state for the marked pixels
    only) and that the walk reaches.  Whether such a pair is blended is implementation-defined."""
    st = o.state
    ys, xs = o.fragile_px.nonzero(as_tuple=True)
    if ys.numel() == 0:
        return []
    m2, co = st.array("means2D").astype(np.float32), st.array("conic_opacity").astype(np.float32)
    plist, ranges, ncon = st.array("point_list"), st.array("ranges"), st.array("n_contrib").reshape(st.H, st.W)
    gx = (st.W + oracle_a.BLOCK - 1) // oracle_a.BLOCK
    pairs = []
    for y, x in zip(ys.tolist(), xs.tolist()):
        tile = (y // oracle_a.BLOCK) * gx + x // oracle_a.BLOCK
        ids = plist[int(ranges[tile, 0]):int(ranges[tile, 1])][:int(ncon[y, x])].astype(np.int64)
        dx, dy = m2[ids, 0] - np.float32(x), m2[ids, 1] - np.float32(y)
        c = co[ids]
        power = np.float32(-0.5) * (c[:, 0] * dx * dx + c[:, 2] * dy * dy) - c[:, 1] * dx * dy
        alpha = np.minimum(np.float32(0.99), c[:, 3] * np.exp(np.minimum(power, np.float32(0))))
        y1 = min((y // oracle_a.BLOCK + 1) * oracle_a.BLOCK, st.H)
        x0, x1 = (x // oracle_a.BLOCK) * oracle_a.BLOCK, min((x // oracle_a.BLOCK + 1) * oracle_a.BLOCK, st.W)
        row = (y % oracle_a.BLOCK) * (x1 - x0) + (x - x0)
        assert y < y1
        for j in np.nonzero((np.abs(alpha * np.float32(255.0) - np.float32(1.0)) < REL_EPS) & (power <= 0))[0].tolist():
            pairs.append((tile, row, j, y, x))
    return pairs


def _combine(views):
    """One truth of V views of the same Gaussians: images and means2D stacked per view, parameter gradients summed over the
    views (the truth in float64, the two float32 oracles in float32, as a float32 implementation would), fragile Gaussians
    the union, fragile pixels per view."""
    T = types.SimpleNamespace()
    T.views = views
    T.images = {n: torch.stack([o.imgs[n][0] for o in views]) for n in views[0].imgs}
    T.fragile_px = torch.stack([o.fragile_px for o in views])
    T.fragile_g = functools.reduce(torch.logical_or, [o.fragile_g for o in views])
    T.radii = torch.stack([o.radii for o in views])
    T.states = [o.state for o in views]
    T.followed = 0
    # image yardstick: the larger of max |B - c64| and max |A32 - c64| on the pixels not marked fragile, over all views
    T.image_yard = {}
    for n in T.images:
        worst = 0.0
        for o in views:
            c64, cb, c32 = o.imgs[n]
            for other in (cb, c32):
                e = (other.double() - c64).abs().max(0)[0][~o.fragile_px]
                worst = max(worst, e.max().item() if e.numel() else 0.0)
        T.image_yard[n] = worst
    T.grads, T.b_grads, T.a32_grads = {}, {}, {}
    for k in views[0].grads:
        for dst, src in ((T.grads, "grads"), (T.b_grads, "b_grads"), (T.a32_grads, "a32_grads")):
            ts = [getattr(o, src)[k] for o in views]
            dst[k] = torch.stack(ts) if k == "means2D" else functools.reduce(torch.add, ts)
    return T


def _squeeze(T):
    T.images = {n: v[0] for n, v in T.images.items()}
    T.fragile_px, T.radii = T.fragile_px[0], T.radii[0]
    for d in (T.grads, T.b_grads, T.a32_grads):
        d["means2D"] = d["means2D"][0]
    T.single = True
    return T


def truth(sc, kw, dC, dF):
    """Single view.  Returns a namespace with: images {"color", "feature"} (float64), grads (float64, Oracle B's key
    names and the reference's conventions), fragile_px [H,W] / fragile_g [P] (Oracle B at REL_EPS), yard {tensor:
    (max, p99)} and image_yard {image: max abs error} (the yardsticks), b_grads / a32_grads (what the yardsticks were
    measured on), radii, states."""
    T = _squeeze(_combine([_one_view(sc, kw, dC, dF)]))
    o = T.views[0]
    T.b_truth_grads = follow(T, o.imgs["color"][1], o.imgs["feature"][1] if "feature" in o.imgs else None).grads
    T.yard = yardsticks(T)
    return T


def truth_views(sc, kws, dC, dF):
    """View batch: kws one settings dict per view, dC [V,3,H,W], dF [V,F,H,W].  As truth(), with images / fragile_px /
    radii / means2D carrying a leading view dimension and the parameter gradients summed over the views."""
    T = _combine([_one_view(sc, kw, dC[v], dF[v]) for v, kw in enumerate(kws)])
    T.single = False
    T.b_truth_grads = follow(T, torch.stack([o.imgs["color"][1] for o in T.views]),
                             torch.stack([o.imgs["feature"][1] for o in T.views])).grads
    T.yard = yardsticks(T)
    return T


def follow(T, colors, features=None):
    """The truth under the implementation's own decision on the pairs whose decision is implementation-defined.

    A pair whose alpha lies within REL_EPS of 1/255 may be blended by one correct implementation and skipped by another
    (util.py, "tolerances").  That moves its pixel by up to T |c| / 255 -- which FRAGILE_TOL allows for -- but it also
    rescales the transmittance of every Gaussian behind it at that pixel and the dL/dalpha of every Gaussian in front by
    ~4e-3: Gaussians that are NOT marked fragile then sit at 1e-3 .. 1e-2 in the per-Gaussian measure (seen on the MI355X in
    the set batch: one such pair, every figure reproduced on the CPU by flipping that pair in the pin).  So the truth follows
    the implementation there, and only there: for each marked pixel that holds such pairs, the implementation's images
    (colors [3,H,W] or [V,3,H,W], and features likewise where there is a feature image) decide between the recorded decision
    and its opposite by which of the two float64 pixels is nearer over all channels; every other decision stays pinned to the float32 oracle's, and the yardsticks stay those
    of the two float32 oracles against the truth under THEIR decisions.  Returns a new truth (T itself when nothing flips)
    with .followed = the number of pixels whose decision was flipped."""
    colors = colors[None] if T.single else colors
    if features is not None and "feature" in T.views[0].imgs:
        colors = torch.cat([colors, features[None] if T.single else features], 1)
    new_views, followed = [], 0
    for v, o in enumerate(T.views):
        new_views.append(o)
        if not o.pairs:
            continue
        def pin_with(pixels):
            pin = dict(o.rec, valid=dict(o.rec["valid"]), keep=dict(o.rec["keep"]))
            for tile, row, j, y, x in o.pairs:
                if (y, x) in pixels:
                    if pin["valid"][tile] is o.rec["valid"][tile]:
                        pin["valid"][tile], pin["keep"][tile] = o.rec["valid"][tile].clone(), o.rec["keep"][tile].clone()
                    pin["valid"][tile][row, j] = ~pin["valid"][tile][row, j]
                    pin["keep"][tile][row, j] = pin["valid"][tile][row, j]
            return pin
        pixels = sorted({(y, x) for _, _, _, y, x in o.pairs})
        c1, c0 = o.run64(pin_with(set(pixels)), backward=False)[:2], (o.imgs["color"][0],)
        if colors.shape[1] > 3:
            c1, c0 = torch.cat(c1), torch.cat([c0[0], o.imgs["feature"][0]])
        else:
            c1, c0 = c1[0], c0[0]
        flip = {(y, x) for y, x in pixels
                if (colors[v][:, y, x].double() - c1[:, y, x]).abs().max() < (colors[v][:, y, x].double() - c0[:, y, x]).abs().max()}
        if not flip:
            continue
        followed += len(flip)
        c, f, g = o.run64(pin_with(flip))
        imgs = dict(o.imgs, color=(c,) + o.imgs["color"][1:])
        if "feature" in imgs:
            imgs["feature"] = (f,) + o.imgs["feature"][1:]
        n = types.SimpleNamespace(**vars(o))
        n.imgs, n.grads = imgs, g
        new_views[-1] = n
    if not followed:
        return T
    N = _combine(new_views)
    N.single = T.single
    if T.single:
        _squeeze(N)
    N.image_yard, N.followed = T.image_yard, followed
    N.yard, N.b_truth_grads = getattr(T, "yard", None), getattr(T, "b_truth_grads", None)
    return N


@functools.lru_cache(maxsize=None)
def case_truth(name):
    """(scene tuple, truth) of CASES[name], computed once per process and shared by every test that needs it; nothing in
    it is modified afterwards."""
    s = scene(CASES[name])
    sc, cam, kw, dC, dF = s
    return s, truth(sc, kw, dC, dF)


def batch_scene(P, F, V, W, H, seed=2):
    """The view-batch inputs of test_gpu_parity._batch_case: one scene, V cameras of a circle, random cotangents."""
    sc = syn.make_scene(P, F=F, M=4, seed=seed)
    cams = syn.circle_cameras(max(V, 4), W, H, negative_focal=True)[:V]
    g = torch.Generator().manual_seed(4)
    return sc, cams, torch.randn(V, 3, H, W, generator=g), torch.randn(V, F, H, W, generator=g)


@functools.lru_cache(maxsize=None)
def batch_truth(name):
    c = VIEW_BATCHES[name]
    sc, cams, dC, dF = batch_scene(c["P"], c["F"], c["V"], c["W"], c["H"])
    kws = [syn.camera_settings_kwargs(cam, 1, True, bg=BG) for cam in cams]
    return (sc, cams, dC, dF), truth_views(sc, kws, dC, dF)


# ---- the gates ------------------------------------------------------------------------------------------------------------

def gate_gradients(tag, T, got):
    """got: {Oracle B's name (or "means2D[v]"): tensor}.  Asserts the measure on every tensor, reports every figure first."""
    share = T.fragile_g.float().mean().item()
    if T.followed:
        print(f"  {tag}: the truth follows the implementation at {T.followed} pixel(s) with a pair inside the 1/255 band")
    assert share <= MAX_FRAGILE_GAUSSIANS, f"{tag}: {share:.3%} of the Gaussians are threshold-fragile (re-seed the case)"
    failures = []
    for k, g in got.items():
        if k.startswith("means2D["):
            g64 = T.grads["means2D"][int(k[8:-1])]
        else:
            g64 = T.grads[k]
        mx, p99 = measure(g, g64, T.fragile_g)
        ymx, yp99 = T.yard[k]
        fe, mag = fragile_error(g, g64, T.fragile_g)
        util.report(tag, tensor=k, hip_max=mx, hip_p99=p99, yard_max=ymx, yard_p99=yp99, bound_max=FACTOR * ymx,
                    bound_p99=FACTOR * yp99, fragile_share=share, followed_pixels=T.followed, fragile_err_over_max=fe / mag if mag else 0.0)
        print(f"  {tag} {k}: max {mx:.3g} (yardstick {ymx:.3g}), p99 {p99:.3g} (yardstick {yp99:.3g}), fragile {share:.3%}")
        if not (mx <= FACTOR * ymx and p99 <= FACTOR * yp99):
            failures.append(f"{k}: max r {mx:.3g} vs {FACTOR:g} x {ymx:.3g}, p99 {p99:.3g} vs {FACTOR:g} x {yp99:.3g}")
        if not fe <= util.FRAGILE_GRAD_TOL * mag + 1e-7:
            failures.append(f"{k} (threshold-fragile): {fe:.3g} vs max {mag:.3g}")
    assert not failures, f"{tag}: " + "; ".join(failures)


def gate_image(tag, name, img, c64, fragile_px, yard, max_fragile_pixels=None):
    """One image [C,H,W] of one view against the truth: robust pixels within FACTOR x yardstick (never above the 1e-4
    contract), fragile ones within util.FRAGILE_TOL, their share capped (for the one-block image: their number)."""
    e = (img.double() - c64).abs().max(0)[0]
    robust = e[~fragile_px].max().item() if (~fragile_px).any() else 0.0
    frag = e[fragile_px].max().item() if fragile_px.any() else 0.0
    bound = min(FACTOR * yard, IMG_CONTRACT)
    util.report(tag, image=name, hip_max=robust, yard_max=yard, bound=bound, fragile_max=frag,
                fragile_share=fragile_px.float().mean().item())
    print(f"  {tag} {name}: {robust:.3g} (yardstick {yard:.3g}, bound {bound:.3g}), fragile pixels {int(fragile_px.sum())}")
    assert robust <= bound, f"{tag} {name}: {robust:.3g} on threshold-robust pixels, bound {bound:.3g}"
    assert frag <= util.FRAGILE_TOL, f"{tag} {name}: {frag:.3g} on threshold-fragile pixels"
    if max_fragile_pixels is not None:
        assert int(fragile_px.sum()) <= max_fragile_pixels, (tag, int(fragile_px.sum()))
    else:
        assert fragile_px.float().mean().item() <= util.FRAGILE_MAX_FRACTION, (tag, fragile_px.float().mean().item())
