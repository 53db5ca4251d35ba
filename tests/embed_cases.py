"""Cases, float64 truths and bounds of the per-point ("embed path") kernels and the fused ResnetFC, shared by
tests/test_embed_kernels.py -- TEST INFRASTRUCTURE.  CPU only, torch only; every truth is computed from seeded inputs.

The rule of every toleranced comparison is tests/volume_cases.py's, unchanged: the truth is the plain torch formulation in float64
on the CPU, fed the same float32 inputs; ref_err is the relative max error of the same formulation in float32 on the CPU; ours
must lie within FACTOR x max(ref_err, 2^-23) x max|truth|, and a case whose ref_err exceeds REF_ERR_CEILING is refused here.
The error is taken per GROUP (a set of rows and columns of one tensor), never per tensor, so that a small-magnitude group --
the scale columns of g_raw, one frequency of the positional code -- cannot hide behind a large one.  Rows whose truth is of
another order of magnitude by construction (a zero quaternion's gradient is g / 1e-12) are groups of their own.

Hard decisions do not sit within float32 rounding of their threshold (the *_conditions functions assert it), except the rows
put there on purpose, whose expected values are stated where they are made.

What is a copy, one float32 add, a select or a relu has one correct float32 result and is compared with torch.equal in the
tests; the expected tensors of those comparisons are built here too (`*_exact`).

The positional code is a function of the float32 canonical coordinate, as in the reference (world_to_canonical runs in float32
before PositionalEncoding): the canonical coordinate itself is pinned bit for bit (`canon32`), and the truth of the code is
sin(x f + phase) in float64 of that float32 coordinate with the module's float32 frequencies and phases, upcast.  sin of the far
point's coordinate (1e6 x 32 pi) has no float32 meaning; that row is left out of the code's groups.
"""
import copy
import math

import torch
import torch.nn.functional as F

from volume_cases import FACTOR, FLOOR, REF_ERR_CEILING, bound, rel_err  # noqa: F401  (the rule, taken unchanged)

POINT_N = (0, 1, 255, 256, 257, 4099)        # per-point kernels: one thread per point, workgroups of 256
EDGE_ROWS_FROM = 255                          # cases of at least this many rows carry the rows put on a threshold on purpose


class Group:
    """A set of rows (bool mask or None = all) and columns (slice) of the 2-D tensor `key` of a result dict."""

    def __init__(self, name, key, cols=slice(None), rows=None):
        self.name, self.key, self.cols, self.rows = name, key, cols, rows

    def of(self, tensors):
        t = tensors[self.key]
        t = t.reshape(t.shape[0], -1) if t.dim() != 2 else t
        t = t[:, self.cols]
        return t if self.rows is None else t[self.rows.to(t.device)]


def group_errors(groups, got, truth, ref=None):
    """{group name: rel_err of got against truth}; with ref (the float32 formulation's results), that one's instead."""
    return {g.name: rel_err(g.of(ref if ref is not None else got).detach().cpu(), g.of(truth)) for g in groups if g.of(truth).numel()}


def _yardsticks(case, groups, ref, truth):
    errs = group_errors(groups, None, truth, ref)
    assert max(errs.values(), default=0.0) <= REF_ERR_CEILING, (case, {k: v for k, v in errs.items() if v > REF_ERR_CEILING})
    return errs


# ---- the regressor epilogue (mgs_regress.hip) -----------------------------------------------------------------------------------
RAW_GROUPS = {"xyz": slice(0, 3), "opacity": slice(3, 4), "scale": slice(4, 7), "rot": slice(7, 11), "f_dc": slice(11, 14),
              "feature": slice(14, 17), "f_rest": slice(17, 26)}
EPILOGUE_OUTPUTS = ("xyz", "opacity", "scale", "rot", "sh", "feature", "feature_normalized")
LOG_SCALE_MAX = math.log(0.05)
SATURATED_LOGITS = (30.0, -30.0, 100.0, -100.0)
# rows of a case with edge rows: 0 a zero quaternion, 1 a zero feature vector, 2 / 3 log-scales 1e-3 above / below ln 0.05,
# 4..7 the saturated opacity logits


def epilogue_inputs(N):
    """raw [N, 26], xyz_in [N, 3] and one cotangent per output, float32."""
    g = torch.Generator().manual_seed(7000 + N)
    raw = torch.randn(N, 26, generator=g)
    s = raw[:, 4:7] * 1.5 - 3.5                                  # exp() on both sides of the 0.05 clamp
    s = torch.where((s - LOG_SCALE_MAX).abs() < 2e-3, s + 0.01, s)
    raw[:, 4:7] = s
    if N >= EDGE_ROWS_FROM:
        raw[0, 7:11] = 0.0
        raw[1, 14:17] = 0.0
        raw[2, 4:7] = LOG_SCALE_MAX + 1e-3
        raw[3, 4:7] = LOG_SCALE_MAX - 1e-3
        raw[4:8, 3] = torch.tensor(SATURATED_LOGITS)
    xyz_in = torch.randn(N, 3, generator=g)
    shapes = dict(xyz=(N, 3), opacity=(N, 1), scale=(N, 3), rot=(N, 4), sh=(N, 4, 3), feature=(N, 3), feature_normalized=(N, 3))
    cot = {k: torch.randn(*shapes[k], generator=g) for k in EPILOGUE_OUTPUTS}
    return raw, xyz_in, cot


def epilogue_conditions(raw):
    r = raw.double()
    assert ((r[:, 4:7] - LOG_SCALE_MAX).abs() >= 1e-4).all(), "a log-scale within 1e-4 of ln 0.05"
    for cols in (slice(7, 11), slice(14, 17)):
        n = r[:, cols].norm(dim=1)
        assert not ((n > 0) & (n < 1e-6)).any(), "a norm between 0 and 1e-6"


def epilogue_fn(raw, xyz_in):
    """The reference's torch ops (models_embed.py:233-253, gaussian_renderer/__init__.py:66-68), in raw's dtype."""
    lead = raw.shape[:-1]
    dxyz, op, sc, rt, fdc, feat, frest = raw.split([3, 1, 3, 4, 3, 3, 9], dim=-1)
    return dict(xyz=xyz_in + dxyz, opacity=torch.sigmoid(op), scale=torch.clamp_max(torch.exp(sc), 0.05),
                rot=F.normalize(rt, dim=-1), sh=torch.cat([fdc.unsqueeze(-2), frest.reshape(*lead, 3, 3)], dim=-2), feature=feat,
                feature_normalized=feat / (feat.norm(dim=-1, keepdim=True) + 1e-12))


def epilogue_restated(raw, cot):
    """(outputs, g_raw) in float64 from the closed forms the kernels implement, without autograd."""
    r = raw.double()
    c = {k: v.double() for k, v in cot.items()}
    N = r.shape[0]
    sig = 1.0 / (1.0 + torch.exp(-r[:, 3:4]))
    e = torch.exp(r[:, 4:7])
    q, f = r[:, 7:11], r[:, 14:17]
    nq, nf = q.norm(dim=1, keepdim=True), f.norm(dim=1, keepdim=True)
    big = nq > 1e-12
    inv = 1.0 / torch.where(big, nq, torch.full_like(nq, 1e-12))
    g = torch.zeros(N, 26, dtype=torch.float64)
    g[:, 0:3] = c["xyz"]
    g[:, 3:4] = c["opacity"] * sig * (1 - sig)
    g[:, 4:7] = torch.where(e <= 0.05, c["scale"] * e, torch.zeros_like(e))
    d = (q * c["rot"]).sum(1, keepdim=True) * inv * inv
    g[:, 7:11] = torch.where(big, (c["rot"] - q * d) * inv, c["rot"] * 1e12)
    sh = c["sh"].reshape(N, 12)
    g[:, 11:14], g[:, 17:26] = sh[:, :3], sh[:, 3:]
    dnm = nf + 1e-12
    k = torch.where(nf > 0, (f * c["feature_normalized"]).sum(1, keepdim=True) / (nf.clamp_min(1e-300) * dnm * dnm), torch.zeros_like(nf))
    g[:, 14:17] = c["feature_normalized"] / dnm - f * k + c["feature"]
    out = dict(opacity=sig, scale=e.clamp_max(0.05), rot=q * inv, feature_normalized=f / dnm)
    return out, g


def with_grads(fn, leaves, cot, dtype):
    """(outputs of fn(*leaves) in dtype, the gradients of sum(out cot) towards every leaf), detached."""
    xs = [t.detach().to(dtype).clone().requires_grad_(True) for t in leaves]
    out = fn(*xs)
    keys = list(out) if isinstance(out, dict) else range(len(out))
    loss = sum((out[k] * cot[k].to(dtype)).sum() for k in keys)
    grads = torch.autograd.grad(loss, xs, allow_unused=True)
    return ({k: out[k].detach() for k in keys} if isinstance(out, dict) else [o.detach() for o in out]), list(grads)


def epilogue_groups(raw):
    zq = raw[:, 7:11].abs().sum(1) == 0
    zf = raw[:, 14:17].abs().sum(1) == 0
    gs = [Group("out." + k, k) for k in ("xyz", "opacity", "scale", "sh", "feature")]
    gs += [Group("out.rot", "rot", rows=~zq), Group("out.rot.zero_rows", "rot", rows=zq),
           Group("out.feature_normalized", "feature_normalized", rows=~zf),
           Group("out.feature_normalized.zero_rows", "feature_normalized", rows=zf)]
    for name, cols in RAW_GROUPS.items():
        if name in ("rot", "feature"):
            z = zq if name == "rot" else zf
            gs += [Group("g_raw." + name, "g_raw", cols, ~z), Group(f"g_raw.{name}.zero_rows", "g_raw", cols, z)]
        else:
            gs.append(Group("g_raw." + name, "g_raw", cols))
    return gs


_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def epilogue_truth(N):
    """Computed once and shared (do not modify): raw, xyz_in, cot, truth (outputs, g_raw, g_xyz_in in float64), groups, ref_err."""
    def make():
        raw, xyz_in, cot = epilogue_inputs(N)
        epilogue_conditions(raw)
        res = {}
        for dt in (torch.float64, torch.float32):
            out, (g_raw, g_xyz) = with_grads(epilogue_fn, [raw, xyz_in], cot, dt)
            res[dt] = dict(out, g_raw=g_raw, g_xyz_in=g_xyz)
        groups = epilogue_groups(raw)
        return dict(raw=raw, xyz_in=xyz_in, cot=cot, truth=res[torch.float64], ref32=res[torch.float32], groups=groups,
                    ref_err=_yardsticks(("epilogue", N), groups, res[torch.float32], res[torch.float64]))
    return _cached(("epilogue", N), make)


# ---- deform_apply (mgs_deform.hip) ---------------------------------------------------------------------------------------------
def apply_inputs(N):
    """delta [N, 7], xyz [N, 3], rot [N, 4] and the cotangents (wx, wr); with edge rows, rot + delta == 0 in row 0."""
    g = torch.Generator().manual_seed(7100 + N)
    delta, xyz, rot = torch.randn(N, 7, generator=g) * 0.3, torch.randn(N, 3, generator=g), torch.randn(N, 4, generator=g)
    if N >= EDGE_ROWS_FROM:
        delta[0, 3:] = -rot[0]
    return delta, xyz, rot, [torch.randn(N, 3, generator=g), torch.randn(N, 4, generator=g)]


def apply_conditions(delta, rot):
    n = (rot + delta[:, 3:]).double().norm(dim=1)
    assert not ((n > 0) & (n < 1e-6)).any(), "a norm between 0 and 1e-6"


def apply_fn(delta, xyz, rot):
    return [xyz + delta[:, :3], F.normalize(rot + delta[:, 3:], dim=-1)]       # models_embed.py:297-299


def apply_restated(delta, rot, wr):
    """g_delta[:, 3:] in float64 from the closed form."""
    q, g = rot.double() + delta[:, 3:].double(), wr.double()
    n = q.norm(dim=1, keepdim=True)
    inv = 1.0 / n.clamp_min(1e-300)
    return torch.where(n > 1e-12, g * inv - q * (q * g).sum(1, keepdim=True) * inv ** 3, g * 1e12)


def apply_truth(N):
    def make():
        delta, xyz, rot, cot = apply_inputs(N)
        apply_conditions(delta, rot)
        res = {}
        for dt in (torch.float64, torch.float32):
            (nx, nr), grads = with_grads(apply_fn, [delta, xyz, rot], cot, dt)
            res[dt] = dict(xyz=nx, rot=nr, g_delta=grads[0])
        z = (rot + delta[:, 3:]).abs().sum(1) == 0
        groups = [Group("out.rot", "rot", rows=~z), Group("out.rot.zero_rows", "rot", rows=z),
                  Group("g_delta.rot", "g_delta", slice(3, 7), ~z), Group("g_delta.rot.zero_rows", "g_delta", slice(3, 7), z)]
        return dict(delta=delta, xyz=xyz, rot=rot, cot=cot, truth=res[torch.float64], ref32=res[torch.float32], groups=groups,
                    ref_err=_yardsticks(("apply", N), groups, res[torch.float32], res[torch.float64]))
    return _cached(("apply", N), make)


# ---- input assembly (mgs_deform.hip): a copy ---------------------------------------------------------------------------------------
def assembly_inputs(N, DL, DZ, DA, has_feat):
    g = torch.Generator().manual_seed(7200 + N + 10 * DL + DZ)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    return dict(point_latent=rn(N, DL), z_feature=rn(N, DZ), xyz=rn(N, 3), sh=rn(N, 4, 3), rot=rn(N, 4), scale=rn(N, 3),
                opacity=rn(N, 1), feature=rn(N, 3) if has_feat else None, action=rn(1, DA) if DA else None)


def assembly_exact(d):
    """models_embed.py:258-287 in torch."""
    N = d["xyz"].shape[0]
    parts = [d["point_latent"], d["xyz"], d["sh"][:, 0], d["sh"][:, 1:].reshape(N, 9), d["rot"], d["scale"], d["opacity"]]
    parts += ([d["feature"]] if d["feature"] is not None else []) + [d["z_feature"]]
    if d["action"] is not None:
        parts.append(d["action"].repeat(N, 1))
    return torch.cat(parts, -1)


# ---- the per-point latent (mgs_voxel.hip) ------------------------------------------------------------------------------------------
BOUNDS = (-0.3, -0.5, 0.6, 0.7, 0.5, 1.6)     # the production scene bounds
VOXEL_GRIDS = ((1, 1, 2), (2, 3, 4), (20, 21, 22))
VOXEL_C, VOXEL_K, VOXEL_N = (1, 8, 64), (0, 6), (1, 257, 4099)
VOXEL_CASES = [(grid, C, K, N) for grid in VOXEL_GRIDS for C in VOXEL_C for K in VOXEL_K for N in VOXEL_N]
VOXEL_LARGE = ((20, 21, 22), 64, 6, 70001)    # forward 70001 x 103 = 7.2 M, backward 70001 x 64 = 4.5 M > 16384 x 256 = 4.2 M
VOXEL_GRID_LIMIT = 16384 * 256                # elements one trip of either grid-stride loop covers
FAR_ROW, SPECIAL_ROWS = 3, 6                  # rows 0..5 of a case with edge rows are put on or outside the box on purpose
FAR = 1.0e6


def _lo_hi(dtype=torch.float32):
    b = torch.tensor(BOUNDS, dtype=torch.float32)
    return b[:3].to(dtype), b[3:].to(dtype)


def voxel_grid_coords(xyz, grid):
    """float64 grid coordinates [N, 3] (x -> W, y -> H, z -> D; align_corners=True)."""
    lo, hi = _lo_hi(torch.float64)
    D, H, W = grid
    return (xyz.double() - lo) / (hi - lo) * torch.tensor([W - 1, H - 1, D - 1], dtype=torch.float64)


def voxel_special_rows(N):
    m = torch.zeros(N, dtype=torch.bool)
    if N >= EDGE_ROWS_FROM:
        m[:SPECIAL_ROWS] = True
    return m


def voxel_conditions(xyz, grid):
    """No grid coordinate of an ordinary point within 1e-4 of an integer (an axis of length 1 has no corner to choose)."""
    D, H, W = grid
    c = voxel_grid_coords(xyz, grid)
    live = torch.tensor([W > 1, H > 1, D > 1])
    near = (((c - c.round()).abs() < 1e-4) & live).any(1) & ~voxel_special_rows(xyz.shape[0])
    return near


def voxel_inputs(case):
    """voxel [1, C, D, H, W], xyz [N, 3] (world), cot [N, C + 3 + 6 K], float32."""
    grid, C, K, N = case
    g = torch.Generator().manual_seed(7300 + (VOXEL_CASES + [VOXEL_LARGE]).index(case))
    lo, hi = _lo_hi()
    draw = lambda n: lo + (hi - lo) * (torch.rand(n, 3, generator=g) * 1.3 - 0.15)  # noqa: E731  (up to 15 % outside the box)
    vox = torch.randn(1, C, *grid, generator=g)
    xyz = draw(N)
    if N >= EDGE_ROWS_FROM:
        xyz[0], xyz[1] = lo, hi                                           # canonical 0 and 1: exactly on the bounds
        xyz[2] = torch.stack([lo[0], hi[1], lo[2]])
        xyz[FAR_ROW] = FAR                                                # far outside: contributes exactly 0
        xyz[4], xyz[5] = lo - 0.15 * (hi - lo), hi + 0.15 * (hi - lo)
    for _ in range(50):
        near = voxel_conditions(xyz, grid)
        if not near.any():
            break
        xyz[near] = draw(int(near.sum()))
    assert not voxel_conditions(xyz, grid).any(), (case, "a grid coordinate within 1e-4 of an integer")
    cot = torch.randn(N, C + 3 + 6 * K, generator=g)
    return vox, xyz, cot


def canon32(xyz):
    """The canonical coordinate as the kernels compute it: one float32 expression, compared bit for bit."""
    lo, hi = _lo_hi()
    return (xyz - lo) * (1.0 / (hi - lo))


def trilinear(vox, xyz, dtype):
    """[N, C]: F.grid_sample of the canonical coordinate (models_embed.py:147-188), all in dtype."""
    lo, hi = _lo_hi(dtype)
    canon = (xyz.to(dtype) - lo) / (hi - lo)
    grid = (canon * 2 - 1.0).view(1, -1, 1, 1, 3)
    out = F.grid_sample(vox.to(dtype), grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    return out.reshape(vox.shape[1], -1).t()


def trilinear_restated(vox, xyz):
    """The eight-corner sum the kernels implement, in float64; differentiable towards vox."""
    _, C, D, H, W = vox.shape
    c = voxel_grid_coords(xyz, (D, H, W))
    fl = c.floor()
    fr = c - fl
    x0, y0, z0 = (fl[:, k].long() for k in range(3))
    out = torch.zeros(xyz.shape[0], C, dtype=torch.float64)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                x, y, z = x0 + dx, y0 + dy, z0 + dz
                w = (fr[:, 0] if dx else 1 - fr[:, 0]) * (fr[:, 1] if dy else 1 - fr[:, 1]) * (fr[:, 2] if dz else 1 - fr[:, 2])
                ok = (x >= 0) & (x < W) & (y >= 0) & (y < H) & (z >= 0) & (z < D)
                v = vox[0][:, z.clamp(0, D - 1), y.clamp(0, H - 1), x.clamp(0, W - 1)]          # [C, N]
                out = out + (w * ok)[:, None] * v.t()
    return out


def pe_constants(K):
    """The module's float32 frequencies and phases (utils.py:133-169: freq_factor pi, num_freqs K), each repeated for sin, cos."""
    freqs = torch.repeat_interleave(math.pi * 2.0 ** torch.arange(0, K), 2)
    phases = torch.zeros(2 * K)
    phases[1::2] = math.pi * 0.5
    assert freqs.dtype == phases.dtype == torch.float32
    return freqs, phases


def positional(canon, K, dtype):
    """[N, 6 K]: sin(x f + phase) of the float32 canonical coordinate, computed in dtype (blocks of 3: sin f0, cos f0, sin f1 ..)."""
    N = canon.shape[0]
    if K == 0:
        return torch.zeros(N, 0, dtype=dtype)
    freqs, phases = pe_constants(K)
    x = canon.to(dtype)
    return torch.sin(torch.addcmul(phases.to(dtype).view(1, -1, 1), x.unsqueeze(1).repeat(1, 2 * K, 1),
                                   freqs.to(dtype).view(1, -1, 1))).reshape(N, -1)


def voxel_groups(case):
    grid, C, K, N = case
    not_far = torch.ones(N, dtype=torch.bool)
    if N >= EDGE_ROWS_FROM:
        not_far[FAR_ROW] = False
    gs = [Group("latent.trilinear", "latent", slice(0, C)), Group("g_voxel", "g_voxel")]
    for k in range(K):
        gs.append(Group(f"latent.sin.f{k}", "latent", slice(C + 3 + 6 * k, C + 6 + 6 * k), not_far))
        gs.append(Group(f"latent.cos.f{k}", "latent", slice(C + 6 + 6 * k, C + 9 + 6 * k), not_far))
    return gs


def voxel_truth(case):
    """Shared (do not modify): vox, xyz, cot, truth / ref32 (latent [N, C + 3 + 6 K] and g_voxel), groups, ref_err."""
    def make():
        grid, C, K, N = case
        vox, xyz, cot = voxel_inputs(case)
        x32 = canon32(xyz)
        res = {}
        for dt in (torch.float64, torch.float32):
            leaf = vox.to(dt).clone().requires_grad_(True)
            tri = trilinear(leaf, xyz, dt)
            (g_vox,) = torch.autograd.grad(tri, leaf, cot[:, :C].to(dt))
            res[dt] = dict(latent=torch.cat([tri.detach(), x32.to(dt), positional(x32, K, dt)], 1), g_voxel=g_vox.reshape(C, -1).t())
        groups = voxel_groups(case)
        return dict(vox=vox, xyz=xyz, cot=cot, canon32=x32, truth=res[torch.float64], ref32=res[torch.float32], groups=groups,
                    ref_err=_yardsticks(case, groups, res[torch.float32], res[torch.float64]))
    return _cached(("voxel", case), make)


# ---- the elementwise passes of the MLP (mgs_mlp.hip) -------------------------------------------------------------------------------
MLP_M, MLP_HIDDEN = (1, 127, 128, 129, 1000), (4, 16, 64, 512, 1024)   # 128 rows per workgroup; n4 = hidden / 4 = 1 .. 256


def mlp_inputs(M, hidden):
    """x / act (with exact zeros and negative zeros: relu'(0) = 0), bias, g_pre, g_res, float32."""
    g = torch.Generator().manual_seed(7400 + 3 * M + hidden)
    act = torch.randn(M, hidden, generator=g)
    flat = act.view(-1)
    flat[::7] = 0.0
    flat[3::11] = -0.0
    return dict(act=act, bias=torch.randn(hidden, generator=g), g_pre=torch.randn(M, hidden, generator=g),
                g_res=torch.randn(M, hidden, generator=g))


def relu_backward_exact(d, with_res):
    g = torch.where(d["act"] > 0, d["g_pre"], torch.zeros_like(d["g_pre"]))
    return g + d["g_res"] if with_res else g


def colsum_truth(M, hidden, with_res):
    """(float64 column sums, ref_err of the float32 column sums): one group per call."""
    def make():
        d = mlp_inputs(M, hidden)
        g64 = torch.where(d["act"] > 0, d["g_pre"], torch.zeros_like(d["g_pre"])).double()
        if with_res:
            g64 = g64 + d["g_res"].double()
        truth = g64.sum(0)
        ref_err = rel_err(relu_backward_exact(d, with_res).sum(0), truth)
        assert ref_err <= REF_ERR_CEILING, (M, hidden, with_res, ref_err)
        return truth, ref_err
    return _cached(("colsum", M, hidden, with_res), make)


# ---- the fused ResnetFC: exact cases -----------------------------------------------------------------------------------------------
# Integer-valued networks: every weight row has two entries of +-1, biases in {-1, 0, 1}, inputs in {-2 .. 2}, cotangents of
# delta in {-1, 0, 1}, cotangents of the features a sparse 0/1 mask.  The same network with every weight, bias, input and
# cotangent replaced by its absolute value bounds every partial sum of every GEMM and column sum of the signed one (ReLU of a
# non-negative number is the identity); while that stays below 2^24, every float32 summation order is exact and the fused path has
# ONE correct answer: the float64 truth, bit for bit.  Exactly-zero pre-activations are plentiful and must act as relu'(0) = 0.
INT_D_IN, INT_D_LATENT = 10, 8
INT_LIMIT = 2.0 ** 24
INT_STRUCTURES = ((5, 3), (5, 0), (5, 5), (1, 1), (2, 3))                 # (n_blocks, combine_layer)
# (M, hidden, n_blocks, combine_layer).  With deform._WGRAD_MIN_ROWS = 16, M = 136 (8 x 17) and 1032 (8 x 129) take the split-K
# weight gradient.
INT_CASES = [(M, 64, 5, 3) for M in (1, 127, 129, 136, 1032)] + [(136, 16, 5, 3), (136, 16, 2, 0)] + \
            [(136, h, nb, cl) for h in (4, 16, 64) for nb, cl in INT_STRUCTURES if (h, nb, cl) not in ((64, 5, 3), (16, 5, 3))]
INT_MODES = ("delta", "features", "both", "frozen", "input_is_data")
FROZEN = ("lin_out.weight", "lin_out.bias", "blocks.1.fc_0.weight", "blocks.1.fc_0.bias")


def _frozen_names(m):
    names = {n for n, _ in m.named_parameters()}
    return [n if n in names else n.replace("blocks.1", "blocks.0") for n in FROZEN]


def integer_network(case, attempt=None):
    """(module on the CPU in float32, zx [M, d_latent + d_in], wd [M, 7], wx [M, hidden]) of the case's seed: the first of
    INT_SEEDS_TRIED whose absolute-value bound stays below 2^24 (integer_seed)."""
    from manigaussian_amd import deform
    M, hidden, n_blocks, combine_layer = case
    attempt = integer_seed(case) if attempt is None else attempt
    g = torch.Generator().manual_seed(7500 + 100 * INT_CASES.index(case) + attempt)
    m = deform.ResnetFC(INT_D_IN, d_out=7, n_blocks=n_blocks, d_latent=INT_D_LATENT, d_hidden=hidden, combine_layer=combine_layer)
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 2:
                cols = torch.rand(p.shape, generator=g).topk(2, dim=1).indices
                signs = torch.randint(0, 2, cols.shape, generator=g).float() * 2 - 1
                p.zero_().scatter_(1, cols, signs)
            else:
                p.copy_(torch.randint(-1, 2, p.shape, generator=g).float())
    zx = torch.randint(-2, 3, (M, INT_D_LATENT + INT_D_IN), generator=g).float()
    wd = torch.randint(-1, 2, (M, 7), generator=g).float()
    wx = (torch.rand(M, hidden, generator=g) < 0.05).float()
    return m, zx, wd, wx


def run_network(m, zx, wd, wx, mode, dtype=None, fused=False):
    """{"delta", "x", "grad zx" (unless the input is data), "grad <parameter>" ...} of module m (left as it was found) on zx's
    device in dtype (default float32); a frozen parameter's gradient is None."""
    dtype = dtype or torch.float32
    mod = copy.deepcopy(m).to(device=zx.device, dtype=dtype)
    mod.fused = fused
    frozen = _frozen_names(mod) if mode == "frozen" else []
    for n, p in mod.named_parameters():
        p.requires_grad_(n not in frozen)
    zin = zx.to(dtype).clone().requires_grad_(mode != "input_is_data")
    delta, x = mod(zin)
    loss = 0.0
    if mode != "features":
        loss = loss + (delta * wd.to(dtype)).sum()
    if mode != "delta":
        loss = loss + (x * wx.to(dtype)).sum()
    named = [(n, p) for n, p in mod.named_parameters() if p.requires_grad]
    leaves = ([zin] if zin.requires_grad else []) + [p for _, p in named]
    grads = list(torch.autograd.grad(loss, leaves, allow_unused=True))
    res = {"delta": delta.detach(), "x": x.detach()}
    if zin.requires_grad:
        res["grad zx"] = grads.pop(0)
    res.update({"grad " + n: None for n in frozen})
    res.update({"grad " + n: g_ for (n, _), g_ in zip(named, grads)})
    return res


INT_SEEDS_TRIED = 20


def integer_seed(case):
    def make():
        for attempt in range(INT_SEEDS_TRIED):
            if integer_abs_bound(case, attempt) < INT_LIMIT:
                return attempt
        raise AssertionError((case, "no seed keeps the absolute-value network below 2^24"))
    return _cached(("int_seed", case), make)


def integer_abs_bound(case, attempt=None):
    """The largest output, gradient or hidden pre-activation of the absolute-value network (float64).  Its bias gradients are
    column sums of the non-negative hidden cotangents, so those are bounded with them."""
    m, zx, wd, wx = integer_network(case, attempt)
    a = copy.deepcopy(m).double()
    with torch.no_grad():
        for p in a.parameters():
            p.abs_()
        hidden = max(float(v.max()) for v in preactivations(a, zx.abs().double()))
    res = run_network(a, zx.abs(), wd.abs(), wx.abs(), "both", torch.float64)
    return max([hidden] + [float(v.abs().max()) for v in res.values()])


def integer_truth(case, mode):
    """Shared (do not modify): the float64 plain path's results; the case is refused unless its absolute-value bound < 2^24."""
    def make():
        b = _cached(("int_bound", case), lambda: integer_abs_bound(case))
        assert b < INT_LIMIT, (case, b)
        m, zx, wd, wx = integer_network(case)
        return run_network(m, zx, wd, wx, mode, torch.float64)
    return _cached(("int", case, mode), make)


def same_values(got, truth):
    """got (float32, any device) holds exactly truth's (float64) numbers; None matches None."""
    if got is None or truth is None:
        return got is None and truth is None
    return got.shape == truth.shape and got.dtype == torch.float32 and torch.equal(got.detach().cpu().double(), truth)


# ---- the fused ResnetFC and the DeformationField: real-valued -------------------------------------------------------------------------
PREACT_MARGIN = 1e-5
REAL_M, REAL_HIDDEN = 1000, 64
FIELD_N, FIELD_HIDDEN = 257, 64
FIELD_VARIANTS = {"action_and_feature": (True, True), "neither": (False, False)}
SEEDS_TRIED = 200


def seeded_parameters(m, g):
    """The existing fused test's weights (the reference's initialisation zeroes fc_1 and the biases: exercise them)."""
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.5 / p.shape[-1] ** 0.5 if p.dim() == 2 else 0.1))


def preactivations(m, zx):
    """Every tensor a ReLU of the plain path is applied to, for module m and input zx (same dtype)."""
    z, x = zx[..., :m.d_latent], zx[..., m.d_latent:]
    x = m.lin_in(x)
    pre = []
    for i in range(m.n_blocks):
        if i < m.combine_layer and i < len(m.lin_z):
            x = x + m.lin_z[i](z)
        net = m.blocks[i].fc_0(torch.relu(x))
        pre += [x, net]
        x = x + m.blocks[i].fc_1(torch.relu(net))
    return pre + [x]


def _near_zero_rows(m, zx):
    """The rows of zx with a float64 pre-activation within PREACT_MARGIN of zero."""
    with torch.no_grad():
        pre = preactivations(copy.deepcopy(m).double(), zx.double())
    return torch.stack([(p.abs() < PREACT_MARGIN).any(1) for p in pre]).any(0)


def _clear_of_zero(m, zx):
    return not _near_zero_rows(m, zx).any()


def real_network():
    """(module, zx [1000, 198], wd, wx, seed), chosen so that no float64 pre-activation lies within 1e-5 of zero: no ReLU can
    then be decided differently by a correct float32 path, and the rule applies to every element.  The case has 704 000
    pre-activations of scale 0.5, about eleven of which fall inside the margin for any seed, so a seed is not rejected as a whole:
    the rows of zx that own such a pre-activation (about 1 % of them) are drawn again from the same generator until none is left.
    Seeds are tried in order; the first one that gets there within 20 redraws is taken."""
    def make():
        from manigaussian_amd import deform
        m = deform.ResnetFC(70, d_hidden=REAL_HIDDEN)
        for seed in range(SEEDS_TRIED):
            g = torch.Generator().manual_seed(seed)
            seeded_parameters(m, g)
            zx = torch.randn(REAL_M, 198, generator=g)
            for _ in range(20):
                near = _near_zero_rows(m, zx)
                if not near.any():
                    break
                zx[near] = torch.randn(int(near.sum()), 198, generator=g)
            if _clear_of_zero(m, zx):
                wd, wx = torch.randn(REAL_M, 7, generator=g), torch.randn(REAL_M, REAL_HIDDEN, generator=g) / REAL_HIDDEN
                return m, zx, wd, wx, seed
        raise AssertionError("no seed keeps every pre-activation 1e-5 away from zero")
    return _cached("real_network", make)


def real_truth():
    """Shared: (truth, ref_err per tensor) of the real-valued case, mode "both"."""
    def make():
        m, zx, wd, wx, _ = real_network()
        truth = run_network(m, zx, wd, wx, "both", torch.float64)
        ref = run_network(m, zx, wd, wx, "both", torch.float32)
        errs = {k: rel_err(ref[k], truth[k]) for k in truth}
        assert max(errs.values()) <= REF_ERR_CEILING, errs
        return truth, errs
    return _cached("real_truth", make)


def field_pipeline(mlp, lat, z, xyz, sh, rot, scale, op, feat, action):
    from test_deform_mlp import _torch_pipeline
    return list(_torch_pipeline(mlp, lat, z, xyz, sh, rot, scale, op, feat, action))


def field_case(variant):
    """Shared: the DeformationField (CPU, float32), its inputs, cotangents, the float64 truth of _torch_pipeline (next xyz, next
    rot, the gradients towards point_latent, z_feature and every parameter) and ref_err per tensor.  Seeds are tried in order
    until no float64 pre-activation of the MLP lies within 1e-5 of zero."""
    def make():
        from manigaussian_amd import deform
        use_action, use_feat = FIELD_VARIANTS[variant]
        N = FIELD_N
        field = deform.DeformationField(use_action=use_action, use_semantic_feature=use_feat, d_hidden=FIELD_HIDDEN)
        for seed in range(SEEDS_TRIED):
            g = torch.Generator().manual_seed(9000 + seed)
            seeded_parameters(field.mlp, g)
            d = assembly_inputs(N, 128, 39, 8 if use_action else 0, use_feat)
            if _clear_of_zero(field.mlp, assembly_exact(d)):
                break
        else:
            raise AssertionError("no seed keeps every pre-activation 1e-5 away from zero")
        cot = [torch.randn(N, 3, generator=g), torch.randn(N, 4, generator=g)]
        names = [n for n, _ in field.mlp.named_parameters()]
        res = {}
        for dt in (torch.float64, torch.float32):
            mlp = copy.deepcopy(field.mlp).to(dt)
            c = {k: (None if v is None else v.to(dt)) for k, v in d.items()}
            lat, z = c["point_latent"].requires_grad_(True), c["z_feature"].requires_grad_(True)
            nx, nr = field_pipeline(mlp, lat, z, c["xyz"], c["sh"], c["rot"], c["scale"], c["opacity"], c["feature"], c["action"])
            grads = torch.autograd.grad((nx * cot[0].to(dt)).sum() + (nr * cot[1].to(dt)).sum(), [lat, z] + list(mlp.parameters()))
            res[dt] = dict({"xyz": nx.detach(), "rot": nr.detach(), "grad point_latent": grads[0], "grad z_feature": grads[1]},
                           **{"grad " + n: g_ for n, g_ in zip(names, grads[2:])})
        errs = {k: rel_err(res[torch.float32][k], res[torch.float64][k]) for k in res[torch.float64]}
        assert max(errs.values()) <= REF_ERR_CEILING, (variant, errs)
        return dict(field=field, inputs=d, cot=cot, truth=res[torch.float64], ref_err=errs, seed=seed)
    return _cached(("field", variant), make)
