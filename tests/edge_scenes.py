"""Scenes in the regimes that synthetic.make_scene seen from synthetic.circle_cameras never reaches, for the float64 truth of
gradient_truth.py.

make_scene draws centres inside the scene bounds, scales <= 0.05 and opacities sigmoid(-2 + N(0,1)) <= 0.91, and
circle_cameras looks at them from 1.58 away: no Gaussian is culled by the near plane (the smallest view depth is 0.78), no
alpha saturates at 0.99 (quirk Q1 of oracle_a.py), next to none has an opacity below 1/255, no covariance is degenerate and
no footprint is wider than the image.  Each case below starts from util.scene_case (or a camera of its own through
syn.look_at_c2w / syn.novel_calib), edits the result, and comes with conditions(): assertions, taken from Oracle B's state
and the truth's recorded decisions, that the case still IS in the regime it is named after.  Seeds and multipliers were
adjusted until the conditions held with Oracle B alone, and then left.

Every case has at most 3000 Gaussians and at most 72x64 pixels.  Plain module beside gradient_truth.py:
tests/test_edge_scenes.py holds the tests."""
import functools
import math

import numpy as np
import torch

import gradient_truth as gt
import util
from manigaussian_amd import synthetic as syn
from oracle import oracle_a

# the camera INSIDE the scene bounds (x -0.3..0.7, y -0.5..0.5, z 0.6..1.6)
INSIDE_EYE, INSIDE_TARGET = (0.2, 0.0, 1.1), (0.2, 0.45, 1.0)
NEAR = 0.2                      # auxiliary.h:154: view_z <= 0.2 is culled
AXIS_DEPTHS = (NEAR - 1e-4, NEAR + 1e-4, 0.21, 0.25)   # +-1e-4: a thousand times the float32 rounding of the view transform

CASES = ("saturated_alpha_f32", "saturated_alpha_f3", "near_plane_negfocal", "near_plane_posfocal", "opacity_band",
         "degenerate_covariance", "huge_footprints_72x40", "sh_clamped_degree3")
VARIANT_CASES = ("saturated_alpha_f32", "near_plane_negfocal", "opacity_band")
VIEW_BATCH = "mixed_visibility_3_views"


def camera(eye, target, W, H, neg, fov_deg=40.0):
    """One look-at camera as synthetic.circle_cameras builds its own."""
    f = (W / 2) / math.tan(math.radians(fov_deg / 2))
    fs = -f if neg else f
    K = np.array([[fs, 0, W / 2], [0, fs, H / 2], [0, 0, 1]], np.float64)
    return syn.novel_calib(syn.look_at_c2w(eye, target, flip_xy=neg), K, W, H)


def _settings(cam, sh_degree=1):
    kw = syn.camera_settings_kwargs(cam, sh_degree, True, bg=gt.BG)
    kw["scale_modifier"] = 1.0
    return kw


def _saturated(F, W, seed):
    sc, cam, kw, dC, dF = util.scene_case(P=150, F=F, W=W, H=W, seed=seed)
    g = torch.Generator().manual_seed(seed + 100)
    op = 0.97 + 0.03 * torch.rand(150, 1, generator=g)
    op[::2] = 1.0
    sc["opacities"] = op.float().contiguous()
    sc["scales"] = (sc["scales"] * 20.0).clamp_max(0.6).contiguous()
    return sc, cam, kw, dC, dF


def axis_rows():
    """[8, 3] world positions at view depths AXIS_DEPTHS of the inside camera: four on its optical axis, four 0.02 to the
    side of it (a shift at right angles to the axis: the same view depth)."""
    eye, tgt = np.asarray(INSIDE_EYE, np.float64), np.asarray(INSIDE_TARGET, np.float64)
    fwd = (tgt - eye) / np.linalg.norm(tgt - eye)
    side = np.cross(fwd, np.array([0.0, 0.0, 1.0]))
    side /= np.linalg.norm(side)
    rows = [eye + d * fwd for d in AXIS_DEPTHS] + [eye + d * fwd + 0.02 * side for d in AXIS_DEPTHS]
    return torch.tensor(np.stack(rows), dtype=torch.float32)


def _near_plane(neg):
    sc, _, _, dC, dF = util.scene_case(P=2000, F=3, W=64, H=64, neg=neg, seed=32)
    rows = axis_rows()
    sc["means3D"][:8] = rows
    sc["opacities"][:8] = 0.1           # (they lie in front of everything at the image centre: keep what is behind visible)
    cam = camera(INSIDE_EYE, INSIDE_TARGET, 64, 64, neg)
    return sc, cam, _settings(cam), dC, dF


def _opacity_band():
    sc, cam, kw, dC, dF = util.scene_case(P=3000, F=3, W=64, H=64, seed=22)
    g = torch.Generator().manual_seed(122)
    op = (3.0 / 255.0) * torch.rand(3000, 1, generator=g)
    op[0::11] = 0.0
    op[1::11] = 1.0 / 255.0
    sc["opacities"] = op.float().contiguous()
    return sc, cam, kw, dC, dF


def _degenerate():
    sc, cam, kw, dC, dF = util.scene_case(P=400, F=3, W=64, H=64, seed=23, unnormalized_rot=True)
    sc["rotations"][0::5] = 0.0         # the reference does not normalise: R = identity
    sc["scales"][1::5] = 0.0            # the covariance is the 0.3 low-pass alone
    return sc, cam, kw, dC, dF


def _huge():
    """Every 10th Gaussian has scale 2.0 and opacity 0.05 (scale 1.0 gives radii of 170 .. 420 px at this camera: 7 of the 30
    above 300), and its centre is moved to twice its distance from the middle of the scene bounds.  Where such a Gaussian's
    pixel mean lies INSIDE the 72x40 image, the nearest pixel has |power| < 2e-5 (conic ~ 7e-5) and Oracle B marks the pair
    as sitting on the power > 0 decision: with the centres as make_scene draws them 16 of the 30 are marked, 5 % of the case
    against MAX_FRAGILE_GAUSSIANS = 2 %.  Spread out, most means fall outside the image -- which the case wants anyway."""
    sc, cam, kw, dC, dF = util.scene_case(P=300, F=3, W=72, H=40, seed=26)
    middle = torch.tensor([0.2, 0.0, 1.1])
    sc["scales"][::10] = 2.0
    sc["opacities"][::10] = 0.05
    sc["means3D"][::10] = middle + 2.0 * (sc["means3D"][::10] - middle)
    return sc, cam, kw, dC, dF


def _sh_clamped():
    sc, cam, kw, dC, dF = util.scene_case(P=800, F=3, M=16, W=64, H=64, sh_degree=3, seed=25)
    sc["shs"] = (sc["shs"] * 6.0).contiguous()
    return sc, cam, kw, dC, dF


_BUILDERS = {
    "saturated_alpha_f32": lambda: _saturated(32, 48, 37),
    "saturated_alpha_f3": lambda: _saturated(3, 64, 27),
    "near_plane_negfocal": lambda: _near_plane(True),
    "near_plane_posfocal": lambda: _near_plane(False),
    "opacity_band": _opacity_band,
    "degenerate_covariance": _degenerate,
    "huge_footprints_72x40": _huge,
    "sh_clamped_degree3": _sh_clamped,
}
assert tuple(_BUILDERS) == CASES


def scene(name):
    """(sc, cam, kw, dC, dF) of a named case, as util.scene_case returns them."""
    return _BUILDERS[name]()


def batch_scene():
    """The view batch: one scene of 1500 Gaussians under a circle camera, the inside camera and a camera that looks away from
    the scene.  Returns (sc, cams, kws, dC [3,3,H,W], dF [3,F,H,W])."""
    W = H = 64
    sc = syn.make_scene(1500, F=3, M=4, seed=28)
    circle = syn.circle_cameras(4, W, H, negative_focal=True)[1]
    eye = np.array([0.2, 0.0, 0.9]) + np.array([1.3, 0.0, 0.9])
    away = camera(eye, 2 * eye - np.array([0.2, 0.0, 0.9]), W, H, True)
    cams = [circle, camera(INSIDE_EYE, INSIDE_TARGET, W, H, True), away]
    g = torch.Generator().manual_seed(4)
    return sc, cams, [_settings(c) for c in cams], torch.randn(3, 3, H, W, generator=g), torch.randn(3, 3, H, W, generator=g)


@functools.lru_cache(maxsize=None)
def case_truth(name):
    """(scene tuple, truth), computed once per process and shared by every test that needs it; nothing in it is modified."""
    s = scene(name)
    sc, cam, kw, dC, dF = s
    return s, gt.truth(sc, kw, dC, dF)


@functools.lru_cache(maxsize=None)
def batch_truth():
    sc, cams, kws, dC, dF = batch_scene()
    return (sc, cams, kws, dC, dF), gt.truth_views(sc, kws, dC, dF)


# ---- what a case is, from Oracle B's state and the recorded decisions -----------------------------------------------------

def view_space(sc, kw):
    """float64 [P,3]: the centres in the camera's frame (auxiliary.h:58-66)."""
    hom = torch.cat([sc["means3D"].double(), torch.ones(sc["means3D"].shape[0], 1, dtype=torch.float64)], 1)
    return hom @ kw["viewmatrix"].double().reshape(4, 4)[:, :3]


def blended(o):
    """bool [P]: the Gaussians blended at one pixel or more (the recorded decisions of the float32 Oracle A, which the truth
    is pinned to and which are checked against Oracle B's sorted lists and last contributors)."""
    out = torch.zeros(o.radii.numel(), dtype=torch.bool)
    plist, ranges = o.aux32["point_list"], o.aux32["ranges"]
    for tile, keep in o.rec["keep"].items():
        out[plist[int(ranges[tile, 0]):int(ranges[tile, 1])][keep.any(0)]] = True
    return out


def stopped_pixels(o):
    """How many pixels stop before the end of their list: a pair that passes alpha >= 1/255 is not blended."""
    return sum(int((o.rec["valid"][t] & ~keep).any(1).sum()) for t, keep in o.rec["keep"].items())


def saturated_pairs(o):
    """[(y, x)] of the blended pairs whose raw alpha o * exp(power) is >= 0.99, one entry per pair: Oracle B's float32
    state walked pixel by pixel up to the last contributor, as gradient_truth._alpha_band_pairs walks it."""
    st = o.state
    m2, co = st.array("means2D").astype(np.float32), st.array("conic_opacity").astype(np.float32)
    plist, ranges, ncon = st.array("point_list"), st.array("ranges"), st.array("n_contrib").reshape(st.H, st.W)
    gx = (st.W + oracle_a.BLOCK - 1) // oracle_a.BLOCK
    out = []
    for y in range(st.H):
        for x in range(st.W):
            tile = (y // oracle_a.BLOCK) * gx + x // oracle_a.BLOCK
            ids = plist[int(ranges[tile, 0]):int(ranges[tile, 1])][:int(ncon[y, x])].astype(np.int64)
            dx, dy = m2[ids, 0] - np.float32(x), m2[ids, 1] - np.float32(y)
            c = co[ids]
            power = np.float32(-0.5) * (c[:, 0] * dx * dx + c[:, 2] * dy * dy) - c[:, 1] * dx * dy
            raw = c[:, 3] * np.exp(np.minimum(power, np.float32(0)))
            out += [(y, x)] * int(((raw >= np.float32(0.99)) & (power <= 0)).sum())
    return out


def _zero_rows(T, rows):
    """The truth's gradient is EXACTLY zero on these Gaussians, on every tensor."""
    for k, g in T.grads.items():
        assert bool((g[rows] == 0).all()), f"{k}: a non-zero truth gradient where there must be none"


def conditions(name, sc, kw, T):
    """Asserts that the case still is what its name says; returns the counts it found ({name: int})."""
    o = T.views[0]
    st, radii = o.state, T.radii
    P, W, H = radii.numel(), st.W, st.H
    vis = radii > 0
    pv = view_space(sc, kw)
    n = {}
    if name.startswith("saturated_alpha"):
        assert bool((sc["opacities"][::2] == 1.0).all()) and sc["opacities"].min().item() >= 0.97
        pairs = saturated_pairs(o)
        n["saturated_pairs"] = len(pairs)
        n["saturated_pixels"] = len(set(pairs))
        n["saturated_blocks_8x8"] = len({(y // 8, x // 8) for y, x in pairs})
        n["stopped_pixels"] = stopped_pixels(o)
        assert n["saturated_pairs"] >= 50 and n["saturated_blocks_8x8"] >= 3, n
        assert n["stopped_pixels"] >= 0.9 * W * H, n
    elif name.startswith("near_plane"):
        z = pv[:, 2]
        for i, d in enumerate(AXIS_DEPTHS + AXIS_DEPTHS):
            assert abs(z[i].item() - d) < 2e-6, (i, z[i].item(), d)
            assert (radii[i].item() > 0) == (d > NEAR), (i, d, radii[i].item())
        n["culled_by_depth"] = int((z <= NEAR).sum())
        n["visible_below_0p4"] = int((vis & (z > NEAR) & (z < 0.4)).sum())
        n["max_radius"] = int(radii.max())
        # oracle_a._clamp_q2's own test, signs and all: under a negative focal length tanfov is negative and EVERY Gaussian
        # counts as clamped (the production regime); under a positive one only those outside 1.3 x the frustum do
        lx, ly = 1.3 * kw["tanfovx"], 1.3 * kw["tanfovy"]
        vx, vy = pv[:, 0] / z, pv[:, 1] / z
        q2 = (vx < -lx) | (vx > lx) | (vy < -ly) | (vy > ly)
        moved = T.grads["means3D"].abs().reshape(P, -1).max(1)[0] > 0
        n["q2_visible_with_gradient"] = int((q2 & vis & moved).sum())
        assert n["culled_by_depth"] >= 1000 and n["visible_below_0p4"] >= 50, n
        assert bool((radii[z <= NEAR] == 0).all())
        assert n["q2_visible_with_gradient"] >= 20, n
    elif name == "opacity_band":
        op = sc["opacities"][:, 0]
        assert bool((op[0::11] == 0).all()) and bool((op[1::11] == np.float32(1.0 / 255.0)).all())
        above = torch.from_numpy(op.numpy() * np.float32(255.0) >= np.float32(0.999))
        n["below_gate"], n["above_gate"] = int((~above).sum()), int(above.sum())
        assert bool(above[1::11].all()) and n["below_gate"] >= 500 and n["above_gate"] >= 500, n
        _zero_rows(T, ~above)
        assert not bool(blended(o)[~above].any())
        # the reference's radius does not look at the opacity (forward.cu:218-224): a Gaussian below the gate keeps it
        n["below_gate_with_radius"] = int((vis & ~above).sum())
        assert bool((vis == (torch.from_numpy(st.array("tiles_touched").astype(np.int64)) > 0)).all())
        assert n["below_gate_with_radius"] >= 0.9 * int(vis.sum()) * n["below_gate"] / P, n
        n["blended_above_gate"] = int(blended(o).sum())
        assert n["blended_above_gate"] >= 200, n
    elif name == "degenerate_covariance":
        b = blended(o)
        zq = (sc["rotations"] == 0).all(1)
        zs = (sc["scales"] == 0).all(1)
        assert int(zq.sum()) == 80 and int(zs.sum()) == 80 and not bool((zq & zs).any())
        n["zero_quaternion_blended"], n["zero_scale_blended"] = int((zq & vis & b).sum()), int((zs & vis & b).sum())
        assert n["zero_quaternion_blended"] >= 50 and n["zero_scale_blended"] >= 50, n
        assert bool((radii[zs & vis] == 3).all())      # ceil(3 sqrt(0.3 + sqrt(max(0.1, 0)))): the low-pass alone
    elif name == "huge_footprints_72x40":
        tiles = ((W + oracle_a.BLOCK - 1) // oracle_a.BLOCK) * ((H + oracle_a.BLOCK - 1) // oracle_a.BLOCK)
        touched = torch.from_numpy(st.array("tiles_touched").astype(np.int64))
        n["radius_above_300_all_tiles"] = int(((radii > 300) & (touched == tiles)).sum())
        n["max_radius"] = int(radii.max())
        m2 = torch.from_numpy(st.array("means2D").astype(np.float32))
        outside = (m2[:, 0] < 0) | (m2[:, 0] > W - 1) | (m2[:, 1] < 0) | (m2[:, 1] > H - 1)
        n["mean_outside_image_blended"] = int((outside & vis & blended(o)).sum())
        assert n["radius_above_300_all_tiles"] >= 20 and n["mean_outside_image_blended"] >= 10, n
    elif name == "sh_clamped_degree3":
        cl = torch.from_numpy(st.array("clamped").astype(bool))
        n["clamped_channels"], n["channels"] = int(cl.sum()), cl.numel()
        n["gaussians_all_clamped"] = int(cl.all(1).sum())
        assert 4 * n["clamped_channels"] >= n["channels"] and n["gaussians_all_clamped"] >= 30, n
        assert bool((T.grads["sh"][cl.all(1)] == 0).all())
        n["all_clamped_and_blended"] = int((cl.all(1) & blended(o)).sum())
        assert n["all_clamped_and_blended"] >= 10, n
    else:
        raise KeyError(name)
    n["fragile_gaussians"], n["fragile_pixels"] = int(T.fragile_g.sum()), int(T.fragile_px.sum())
    util.report(f"edge/{name}/conditions", **n)
    return n


def batch_conditions(sc, kws, T):
    """The view batch: a populated view, a view from inside with a near-culled majority, a view with no instance at all."""
    n = {"visible": [int((r > 0).sum()) for r in T.radii], "num_rendered": [int(s.num_rendered) for s in T.states],
         "culled_by_depth": [int((view_space(sc, kw)[:, 2] <= NEAR).sum()) for kw in kws]}
    assert n["visible"][0] >= 1000 and 20 <= n["visible"][1] <= 500 and n["visible"][2] == 0, n
    assert n["num_rendered"][0] > 0 and n["num_rendered"][1] > 0 and n["num_rendered"][2] == 0, n
    assert n["culled_by_depth"][0] == 0 and n["culled_by_depth"][1] >= 1000 and n["culled_by_depth"][2] == 1500, n
    n["fragile_gaussians"], n["fragile_pixels"] = int(T.fragile_g.sum()), int(T.fragile_px.sum())
    util.report(f"edge/{VIEW_BATCH}/conditions", **n)
    return n
