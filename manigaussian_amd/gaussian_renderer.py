"""render(): the per-view Python prologue ManiGaussian runs before the rasterizer.

Mirror of agents/manigaussian_bc/gaussian_renderer/__init__.py:17-94 (same signature, same returned dict,
same choices: sh_degree = 3 unless SH features are given, features L2-normalised with a 1e-12 guard, a
zeros [N,3] placeholder when no language features are given).  The reference file itself is executed
unmodified against this repository's `diff_gaussian_rasterization` package on the GPU by
tests/test_integration.py (from a build-time byte copy that is never committed).

render_sets(): several such renders -- ManiGaussian's current frame and deformed next frame -- in ONE rasterizer call (a set
batch, manigaussian_amd.views).
"""
import math

import torch

from .rasterizer import GaussianRasterizationSettings, GaussianRasterizer
from .views import GaussianRasterizerBatch


def _settings(data, idx, bg, sh_degree, include_feature):
    view = data["novel_view"]
    if "tanfov_host" in view:  # manigaussian_amd.camera.TargetCache: host copies, no device read-back per view
        tanfovx, tanfovy = view["tanfov_host"][idx]
        height, width = view["size_host"][idx]
    else:                      # the reference's dict: four scalar device reads (gaussian_renderer/__init__.py:35-39)
        tanfovx, tanfovy = math.tan(view["FovX"][idx] * 0.5), math.tan(view["FovY"][idx] * 0.5)
        height, width = int(view["height"][idx]), int(view["width"][idx])
    return GaussianRasterizationSettings(
        image_height=height, image_width=width, tanfovx=tanfovx, tanfovy=tanfovy,
        bg=bg, scale_modifier=1.0, viewmatrix=view["world_view_transform"][idx],
        projmatrix=view["full_proj_transform"][idx], sh_degree=sh_degree,
        campos=view["camera_center"][idx], prefiltered=False, debug=False, include_feature=include_feature)


def render(data, idx, pts_xyz, rotations, scales, opacity, bg_color, pts_rgb=None, features_color=None,
           features_language=None):
    device = pts_xyz.device
    bg = torch.tensor(bg_color, dtype=torch.float32, device=device)
    # gradient holder for the 2D means (gaussian_renderer/__init__.py:28-32)
    screenspace_points = torch.zeros_like(pts_xyz, dtype=torch.float32, requires_grad=True, device=device) + 0
    try:
        screenspace_points.retain_grad()
    except Exception:
        pass
    settings = _settings(data, idx, bg, 3 if features_color is None else 1, features_language is not None)
    rasterizer = GaussianRasterizer(raster_settings=settings)
    shs = colors_precomp = None
    if features_color is not None:
        shs = features_color
    else:
        assert pts_rgb is not None
        colors_precomp = pts_rgb
    if features_language is not None:
        feats = features_language / (features_language.norm(dim=-1, keepdim=True) + 1e-12)
    else:
        feats = torch.zeros((opacity.shape[0], 3), dtype=opacity.dtype, device=opacity.device)
    image, feature_image, radii = rasterizer(means3D=pts_xyz, means2D=screenspace_points, shs=shs,
                                             colors_precomp=colors_precomp, language_feature_precomp=feats,
                                             opacities=opacity, scales=scales, rotations=rotations,
                                             cov3D_precomp=None)
    return {"render": image, "render_embed": feature_image, "viewspace_points": screenspace_points, "radii": radii}


_ITEM = ("data", "idx", "pts_xyz", "rotations", "scales", "opacity", "pts_rgb", "features_color", "features_language")


def render_sets(items, bg_color):
    """[render(*item, bg_color) ...] in ONE rasterizer call: every item is render()'s argument list without bg_color --
    (data, idx, pts_xyz, rotations, scales, opacity, pts_rgb, features_color, features_language), a sequence in this order
    or a dict with these keys -- and is one Gaussian set rendered in one view (ManiGaussian's step: pts2render(data) and
    pts2render(data['next']), agents/manigaussian_bc/neural_rendering.py:283,324).  Returns the dicts render() returns, with
    the same images bit for bit.  The items must agree on image size, on SH versus precomputed colours and on whether
    language features are given; their Gaussian counts must be equal.  Gradients reach each item's tensors as they would
    through its own render() call: a leaf shared by several items gets the sum, a detached tensor gets none.
    'viewspace_points' of item v is row v of the batch's [V,P,3] gradient holder."""
    return _render_sets(items, bg_color)[0]


def render_sets_stacked(items, bg_color):
    """render_sets(items, bg_color) together with the batch tensors its dicts are slices of: returns (list, batch) with
    batch = {"render": [V,3,H,W], "render_embed": [V,F,H,W] (the rasterizer's [1] placeholder without language features),
    "viewspace_points": [V,P,3], "radii": [V,P]}.  A loss taken on the batch tensors (manigaussian_amd.losses) hands autograd
    the whole batch gradient at once; taken on the per-view slices, autograd first rebuilds it with a zero-fill and an add
    per slice."""
    return _render_sets(items, bg_color)


def _render_sets(items, bg_color):
    its = [dict(it) if isinstance(it, dict) else dict(zip(_ITEM, it)) for it in items]
    if not its:
        return [], None
    first = its[0]
    device = first["pts_xyz"].device
    sh = first["features_color"] is not None
    feat = first["features_language"] is not None
    # (a float32 device tensor is taken as it is: building one from a list is a host-to-device copy, which a graph capture
    #  of the step cannot hold)
    bg = bg_color if isinstance(bg_color, torch.Tensor) else torch.tensor(bg_color, dtype=torch.float32, device=device)
    settings = [_settings(it["data"], it["idx"], bg, 1 if sh else 3, feat) for it in its]
    for v, (it, st) in enumerate(zip(its, settings)):
        if (st.image_height, st.image_width) != (settings[0].image_height, settings[0].image_width):
            raise ValueError(f"render_sets: item {v} renders {st.image_height}x{st.image_width}, item 0 "
                             f"{settings[0].image_height}x{settings[0].image_width}: the items must share the image size")
        if (it["features_color"] is not None) != sh:
            raise ValueError(f"render_sets: item {v} and item 0 differ in SH versus precomputed colours")
        if (it["features_language"] is not None) != feat:
            raise ValueError(f"render_sets: item {v} and item 0 differ in whether language features are given")
        if not sh and it["pts_rgb"] is None:
            raise ValueError(f"render_sets: item {v} gives neither features_color nor pts_rgb")
    V = len(its)
    stack = lambda k: torch.stack([it[k] for it in its])  # noqa: E731
    if feat:  # render()'s normalisation, item by item (the same arithmetic as its own call)
        feats = torch.stack([f / (f.norm(dim=-1, keepdim=True) + 1e-12) for f in (it["features_language"] for it in its)])
    else:
        op = first["opacity"]
        feats = torch.zeros((V, op.shape[0], 3), dtype=op.dtype, device=op.device)
    means3D = stack("pts_xyz")
    # gradient holder for the 2D means of every view (render(): one [P,3] holder per call)
    screenspace_points = torch.zeros((V,) + tuple(first["pts_xyz"].shape), dtype=torch.float32, requires_grad=True,
                                     device=device) + 0
    try:
        screenspace_points.retain_grad()
    except Exception:
        pass
    rasterizer = GaussianRasterizerBatch(settings, view_sets=list(range(V)))
    image, feature_image, radii = rasterizer(
        means3D=means3D, means2D=screenspace_points, shs=stack("features_color") if sh else None,
        colors_precomp=None if sh else stack("pts_rgb"), language_feature_precomp=feats, opacities=stack("opacity"),
        scales=stack("scales"), rotations=stack("rotations"), cov3D_precomp=None)
    views = [{"render": image[v], "render_embed": feature_image[v] if feat else feature_image,
              "viewspace_points": screenspace_points[v], "radii": radii[v]} for v in range(V)]
    return views, {"render": image, "render_embed": feature_image, "viewspace_points": screenspace_points, "radii": radii}
