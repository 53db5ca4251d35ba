"""Scenes for tests/test_fwd_reachable_chunks.py: stacks of large, low-opacity Gaussians in front of the camera, so that how many
64-survivor chunks a block of the render forward visits is chosen by the opacity -- the transmittance after n entries is
about (1 - alpha)^n -- and a CPU model of the chunk walk, built on Oracle B's own preprocess and lists, that says what each
scene reaches.  Shared by the tests and by tests/tools/reachable_chunks_graph_check.py."""
import math
import types

import numpy as np
import torch

from manigaussian_amd import synthetic as syn

CHUNK = 64          # survivors per chunk (csrc/mgs_common.h)
T_STOP = 1e-4       # the reference's stop threshold (forward.cu:372)


def _quat_of(Rm):
    """(w, x, y, z) of a rotation matrix."""
    w = math.sqrt(max(0.0, 1.0 + Rm[0, 0] + Rm[1, 1] + Rm[2, 2])) / 2
    x = math.copysign(math.sqrt(max(0.0, 1.0 + Rm[0, 0] - Rm[1, 1] - Rm[2, 2])) / 2, Rm[2, 1] - Rm[1, 2])
    y = math.copysign(math.sqrt(max(0.0, 1.0 - Rm[0, 0] + Rm[1, 1] - Rm[2, 2])) / 2, Rm[0, 2] - Rm[2, 0])
    z = math.copysign(math.sqrt(max(0.0, 1.0 - Rm[0, 0] - Rm[1, 1] + Rm[2, 2])) / 2, Rm[1, 0] - Rm[0, 1])
    return torch.tensor([w, x, y, z], dtype=torch.float32)


def stack_scene(n, opacity, W=16, H=16, F=32, sigma_px=(60.0, 60.0), centre_px=(0.0, 0.0), seed=3):
    """n Gaussians on the optical axis at increasing depths (list order = index order), axes aligned with the camera's, screen
    footprint sigma_px = (sx, sy) pixels at depth 2, centred centre_px pixels off the image centre; opacity: a float or [n].
    Returns (scene, cam, settings kwargs, d_color, d_feat)."""
    cam = syn.circle_cameras(4, W, H, negative_focal=True)[1]
    sc = syn.make_scene(n, F=F, M=4, seed=seed)
    c2w = torch.linalg.inv(cam["world_view_transform"].T).double()
    right, down, fwd, eye = c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3]
    f = (W / 2) / math.tan(math.radians(20.0))                 # pixels (circle_cameras: fov 40 degrees)
    depth = torch.linspace(2.0, 2.5, n, dtype=torch.float64)
    off = (depth / f)[:, None]                                 # world units per pixel at that depth
    sc["means3D"] = (eye + depth[:, None] * fwd + centre_px[0] * off * right + centre_px[1] * off * down).float().contiguous()
    sc["rotations"] = _quat_of(c2w[:3, :3].numpy()).repeat(n, 1).contiguous()
    s = torch.tensor([sigma_px[0], sigma_px[1], min(sigma_px)], dtype=torch.float64) * 2.0 / f
    sc["scales"] = s.float().repeat(n, 1).contiguous()
    sc["opacities"] = (torch.as_tensor(opacity, dtype=torch.float32) * torch.ones(n)).reshape(n, 1).contiguous()
    kw = syn.camera_settings_kwargs(cam, 1, F > 0, bg=(0.1, 0.2, 0.3))
    dC, dF = syn.make_cotangents(W, H, F)
    return sc, cam, kw, dC, dF


def oracle_forward(sc, kw):
    from oracle import oracle_b
    return oracle_b.forward(sc["means3D"], sc["opacities"], types.SimpleNamespace(**kw), shs=sc["shs"],
                            language_feature=sc.get("language_feature"), scales=sc["scales"], rotations=sc["rotations"])


def chunk_model(state):
    """What the chunk walk does on Oracle B's lists, in float32: per pixel the transmittance ENTERING every chunk of its tile's
    list (the plain product of 1 - alpha over the entries before it, skipped entries count 1: forward.cu:345-356), hence the
    chunks the pixel visits (those it enters with T >= 1e-4).  The model holds for scenes whose every list entry reaches every
    8x8 block of its tile with alpha >= 1/255 at some pixel (asserted): then every block's survivors are the whole list.
    Returns a namespace: n [T] list lengths, enter [T][chunks, 16, 16], vis [H, W], chunks, pixel_chunks, incidences (the
    three counts of mgs_forward_stats), block_vis {(tile, by, bx): visited chunks}, margin (the least |T / 1e-4 - 1| over every
    pixel and chunk boundary: how far the scene is from a decision that rounding could flip) and block_margin (the same over
    each block's most transparent pixel, which alone decides whether the block visits the chunk)."""
    W, H = state.W, state.H
    co, m2 = state.array("conic_opacity").astype(np.float32), state.array("means2D").astype(np.float32)
    pl, rg = state.array("point_list").astype(np.int64), state.array("ranges").astype(np.int64)
    tx = (W + 15) // 16
    out = types.SimpleNamespace(n=[], enter=[], vis=np.zeros((H, W), np.int64), chunks=0, pixel_chunks=0, incidences=0,
                                block_vis={}, margin=np.inf, block_margin=np.inf)
    for t, (lo, hi) in enumerate(rg):
        ids = pl[lo:hi]
        n = len(ids)
        out.n.append(n)
        x0, y0 = (t % tx) * 16, (t // tx) * 16
        px = np.arange(x0, x0 + 16, dtype=np.float32)[None, None, :]
        py = np.arange(y0, y0 + 16, dtype=np.float32)[None, :, None]
        inside = ((px < W) & (py < H))[0]
        dx, dy = m2[ids, 0][:, None, None] - px, m2[ids, 1][:, None, None] - py
        c = co[ids]
        power = np.float32(-0.5) * (c[:, 0, None, None] * dx * dx + c[:, 2, None, None] * dy * dy) - c[:, 1, None, None] * dx * dy
        alpha = np.minimum(np.float32(0.99), c[:, 3, None, None] * np.exp(power))
        alpha = np.where((power > 0) | (alpha < np.float32(1.0 / 255.0)), np.float32(0), alpha).astype(np.float32)
        nch = (n + CHUNK - 1) // CHUNK
        prod = np.cumprod(np.float32(1) - alpha, axis=0, dtype=np.float32) if n else np.zeros((0, 16, 16), np.float32)
        enter = np.ones((max(nch, 1), 16, 16), np.float32)
        for k in range(1, nch):
            enter[k] = prod[CHUNK * k - 1]
        out.enter.append(enter)
        alive = (enter[:nch] >= np.float32(T_STOP)) & inside[None]
        vis = alive.sum(0)
        if nch:
            out.margin = min(out.margin, float(np.abs(enter[:nch][:, inside] / np.float32(T_STOP) - 1).min()))
        for by in range(2):
            for bx in range(2):
                blk = (slice(8 * by, 8 * by + 8), slice(8 * bx, 8 * bx + 8))
                if not inside[blk].any():
                    continue
                assert n == 0 or (alpha[(slice(None),) + blk] * inside[blk]).reshape(n, -1).max(1).min() > 0, \
                    "an entry misses a block: the model's survivors are not the list"
                vmax = int(vis[blk].max())
                if nch:
                    top = np.where(inside[blk][None], enter[(slice(0, nch),) + blk], 0).reshape(nch, -1).max(1)
                    out.block_margin = min(out.block_margin, float(np.abs(top / np.float32(T_STOP) - 1).min()))
                out.block_vis[(t, by, bx)] = vmax
                out.chunks += vmax
                out.incidences += min(n, vmax * CHUNK)
        out.pixel_chunks += int(vis.sum())
        out.vis[y0:y0 + 16, x0:x0 + 16][inside[:H - y0, :W - x0]] = vis[inside]
    return out


def die_after(entries):
    """The opacity of a uniform stack whose centre pixel's transmittance falls below 1e-4 after about `entries` entries."""
    return 1.0 - math.exp(math.log(T_STOP) / entries)
