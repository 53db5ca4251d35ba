"""Multi-view batches: V views of ONE Gaussian set rasterized in one call.

The reference renders strictly one view per call (agents/manigaussian_bc/neural_rendering.py:386 `assert bs == 1`,
and again for the next-frame scene, :324); ManiGaussian's BASELINE configs render 4-16 views per step.  At 128x128 a
single view cannot fill 256 CUs (64 tiles), so batching is the natural unit on MI355X: the views are stacked into an
atlas, every launch covers all of them, and the per-Gaussian gradients are summed over the views on the device.

    rast = GaussianRasterizerBatch([settings_0, ..., settings_{V-1}])     # same H, W, sh_degree, scale_modifier, bg
    color, feature, radii = rast(means3D, means2D, opacities, shs=..., language_feature_precomp=..., scales=..., rotations=...)
    # color [V,3,H,W], feature [V,F,H,W] (or [1]), radii [V,P] int32; means2D: [V,P,3] gradient holder (or None)

Results per view are those of GaussianRasterizer (same kernels); gradients w.r.t. the Gaussian parameters are the sums
over the views; `means2D.grad` is per view.

Set batches: the views may render DIFFERENT Gaussian sets of one size P (ManiGaussian's step renders the current frame and
the deformed next frame).  Every Gaussian input then carries a leading set dimension S, and view v renders set view_sets[v]:

    rast = GaussianRasterizerBatch([settings_0, ..., settings_{V-1}], view_sets=[0, 1, ...])   # None: view v renders set v
    color, feature, radii = rast(means3D [S,P,3], means2D [V,P,3], opacities [S,P,1], shs=[S,P,M,3], ...)

Images and radii are per view as above, bit for bit those of a GaussianRasterizer call of the view on its set; every
per-Gaussian gradient is [S,P,.]: row (s, i) sums the views of set s, and a set no view renders gets zeros.
"""
import ctypes
from typing import Optional, Sequence

import torch
import torch.nn as nn

from . import _C, _lib
from .rasterizer import GaussianRasterizationSettings, _EMPTY, _check_inputs, _or_empty

_F32 = torch.float32


class _RasterizeViews(torch.autograd.Function):
    """The autograd glue of a batch: the forward and backward are the ctypes shim's (manigaussian_amd/_C.py), given the
    per-view cameras."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, language_feature, opacities, scales, rotations, cov3D_precomp,
                settings, view_sets):
        if not means3D.is_cuda:
            raise RuntimeError("GaussianRasterizerBatch needs tensors on a HIP device; there is no CPU path")
        dev, s0, V = means3D.device, settings[0], len(settings)
        views, cams = (_lib.MgsView * V)(), []
        for v, s in enumerate(settings):
            vm, pm, cp = (_C._f32c(s.viewmatrix, "viewmatrix", dev), _C._f32c(s.projmatrix, "projmatrix", dev),
                          _C._f32c(s.campos, "campos", dev))
            cams += [vm, pm, cp]
            views[v].tanfovx, views[v].tanfovy = float(s.tanfovx), float(s.tanfovy)
            views[v].viewmatrix, views[v].projmatrix, views[v].campos = vm.data_ptr(), pm.data_ptr(), cp.data_ptr()
        sets = None
        if view_sets is not None:  # a set batch: the Gaussian inputs are [S,P,.]
            sets = (int(means3D.size(0)), (ctypes.c_int32 * V)(*view_sets))
        # (a batch ignores settings.debug; the cameras travel in `views`)
        handle, color, feature, radii, geom, binning, img, grad_buffer = _C._forward(
            s0.bg, means3D, colors_precomp, language_feature, opacities, scales, rotations, s0.scale_modifier, cov3D_precomp,
            _EMPTY, _EMPTY, 0.0, 0.0, s0.image_height, s0.image_width, sh, s0.sh_degree, _EMPTY, s0.prefiltered, False,
            s0.include_feature, any(ctx.needs_input_grad[:9]), views=(views, V, cams), sets=sets)
        ctx.settings, ctx.num_rendered, ctx.grad_buffer = settings, handle, grad_buffer
        ctx.mark_non_differentiable(radii)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(colors_precomp, language_feature, means3D, scales, rotations, cov3D_precomp, radii, sh, geom,
                              binning, img)
        return color, feature, radii

    @staticmethod
    def backward(ctx, g_color, g_feat, _g_radii):
        colors_precomp, language_feature, means3D, scales, rotations, cov3D_precomp, radii, sh = ctx.saved_tensors[:8]
        s0, V, P = ctx.settings[0], len(ctx.settings), int(means3D.size(-2))
        if P == 0 or (g_color is None and g_feat is None):
            return (None,) * 11
        H, W, inc = s0.image_height, s0.image_width, bool(s0.include_feature)
        if g_color is None:
            g_color = torch.zeros((V, 3, H, W), dtype=_F32, device=means3D.device)
        if inc and g_feat is None:
            g_feat = torch.zeros((V, language_feature.size(-1), H, W), dtype=_F32, device=means3D.device)
        grad_buffer, ctx.grad_buffer = ctx.grad_buffer, None
        (d_means2D, d_colors, d_feat, d_opacity, d_means3D, d_cov3D, d_sh, d_scales, d_rot) = _C._backward(
            s0.bg, means3D, radii, colors_precomp, language_feature, scales, rotations, s0.scale_modifier, cov3D_precomp,
            _EMPTY, _EMPTY, 0.0, 0.0, g_color, g_feat, sh, s0.sh_degree, _EMPTY, None, ctx.num_rendered, None, None, False,
            inc, grad_buffer)
        given = lambda g, t: g if t.numel() else None  # noqa: E731
        # (per-view colour gradients only feed the SH backward)
        return (d_means3D, d_means2D, given(d_sh, sh), given(d_colors, colors_precomp), d_feat if inc else None, d_opacity,
                given(d_scales, scales), given(d_rot, rotations), given(d_cov3D, cov3D_precomp), None, None)


class GaussianRasterizerBatch(nn.Module):
    """V views per call; see the module docstring.  Argument names and exclusivity rules are GaussianRasterizer's
    (RAST/diff_gaussian_rasterization/__init__.py:197-233).  view_sets: the set each view renders when the Gaussian inputs
    carry a leading set dimension (None: view v renders set v)."""

    def __init__(self, raster_settings: Sequence[GaussianRasterizationSettings], view_sets: Optional[Sequence[int]] = None):
        super().__init__()
        rs = list(raster_settings)
        if not 1 <= len(rs) <= _lib.MAX_VIEWS:
            raise ValueError(f"GaussianRasterizerBatch takes 1..{_lib.MAX_VIEWS} views, got {len(rs)}")
        s0 = rs[0]
        for s in rs[1:]:
            same = (s.image_height == s0.image_height and s.image_width == s0.image_width and s.sh_degree == s0.sh_degree
                    and s.scale_modifier == s0.scale_modifier and s.include_feature == s0.include_feature
                    and s.prefiltered == s0.prefiltered and (s.bg is s0.bg or torch.equal(s.bg, s0.bg)))
            if not same:
                raise ValueError("all views of a batch must share image size, sh_degree, scale_modifier, bg, "
                                 "include_feature and prefiltered")
        self.raster_settings = tuple(rs)
        self.view_sets = None if view_sets is None else tuple(int(s) for s in view_sets)
        if self.view_sets is not None and len(self.view_sets) != len(rs):
            raise ValueError(f"view_sets has {len(self.view_sets)} entries for {len(rs)} views")

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, language_feature_precomp=None,
                scales=None, rotations=None, cov3D_precomp=None):
        _check_inputs(shs, colors_precomp, scales, rotations, cov3D_precomp)
        view_sets = _set_layout(self.view_sets, len(self.raster_settings), means3D, means2D, opacities, shs, colors_precomp,
                                language_feature_precomp, scales, rotations, cov3D_precomp)
        return _RasterizeViews.apply(means3D, _or_empty(means2D), _or_empty(shs), _or_empty(colors_precomp),
                                     _or_empty(language_feature_precomp), opacities, _or_empty(scales), _or_empty(rotations),
                                     _or_empty(cov3D_precomp), self.raster_settings, view_sets)


def _set_layout(view_sets, V, means3D, means2D, opacities, shs, colors_precomp, language_feature, scales, rotations,
                cov3D_precomp):
    """Which path a batch takes, checked on the shapes alone (before any device work): None for Gaussian inputs without a
    set dimension (a view batch of one set), else the V views' set indices."""
    if means3D.ndimension() != 3:
        if view_sets is not None:
            raise ValueError("view_sets needs Gaussian inputs with a leading set dimension: means3D [S,P,3]")
        return None
    S, P = int(means3D.size(0)), int(means3D.size(1))
    if not 1 <= S <= _lib.MAX_VIEWS:
        raise ValueError(f"a set batch takes 1..{_lib.MAX_VIEWS} Gaussian sets, got S = {S}")
    named = {"opacities": (opacities, 3), "shs": (shs, 4), "colors_precomp": (colors_precomp, 3),
             "language_feature_precomp": (language_feature, 3), "scales": (scales, 3), "rotations": (rotations, 3),
             "cov3D_precomp": (cov3D_precomp, 3)}
    for name, (t, nd) in named.items():
        if t is None or t.numel() == 0:
            continue
        if t.ndimension() != nd or tuple(t.shape[:2]) != (S, P):
            raise ValueError(f"{name} has shape {tuple(t.shape)}: every Gaussian input of a set batch is [S,P,...] with the "
                             f"leading dimensions of means3D, ({S}, {P})")
    if means2D is not None and means2D.numel() != 0 and tuple(means2D.shape) != (V, P, 3):
        raise ValueError(f"means2D has shape {tuple(means2D.shape)}: a set batch needs [V,P,3] = [{V},{P},3] (or None)")
    if view_sets is None:
        if S != V:
            raise ValueError(f"{S} Gaussian sets for {V} views: without view_sets view v renders set v, which needs S == V")
        return tuple(range(V))
    if len(view_sets) != V:
        raise ValueError(f"view_sets has {len(view_sets)} entries for {V} views")
    for v, s in enumerate(view_sets):
        if not 0 <= s < S:
            raise ValueError(f"view {v} renders set {s}, outside [0, {S})")
    return tuple(view_sets)
