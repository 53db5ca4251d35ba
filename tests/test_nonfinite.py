"""Non-finite values: one NaN, +inf or -inf in one element of one operand of a fused op, and the op must put NaN and infinities where
the op it replaces puts them.  tests/nonfinite.py holds the contract and the machinery: every element of every result and gradient
is classed finite / NaN / +inf / -inf; ours must have the class of the reference's float64 run at every element that is not FREE
(whose non-finite class in the reference rests on the taint times an exact zero), and where that class is finite it must lie within the
op's existing bound, taken over the finite elements.  A case is admitted only if the reference's own float32 and float64 runs agree
on every class and the free elements keep their cap (none for an op without padding, interpolation or dropout, else an eighth of the
non-finite elements of a result); test_the_reference_speaks_clearly runs both checks without a GPU.  The truths are the ops' existing
ones: torch's compositions at test time, and for the spatial softmax and LAMB the restatements of their own test files, which the
reference's modules are held to class for class (tests/golden/nonfinite/*.npz, tests/golden/make_golden_nonfinite.py).

Per operand: the three values at two positions at least -- the first element and one on a seam of the kernel's tiling (the second
workgroup's only row or point, a row's scalar tail, the last output channel's centre tap) -- on the smallest cases the family's table
has for masked lanes and seams.  For the convolutions the taint sits on a centre tap or an interior voxel, where the reference alone
keeps the free elements under their cap; with a ReLU (slope 0) the upstream gradient's taint sits on a live unit.

Where the values of the enrolled operands go, read off the kernels before any of this ran on a GPU.  None reaches an address, a
loop bound or a launch size; those come from the shapes alone ("compare": the value is compared, the outcome selects between values):

op (kernels)                        operand                      where its value goes
----------------------------------  ---------------------------  ---------------------------------------------------------------
mlp (mlp_relu_bias, _relu_bwd)      x, bias                      a select on x <= 0, one add; stored
                                    act, g_pre, g_res            compare act <= 0, select, add; column sums (float atomics)
deform_apply fwd / bwd              delta, rot, xyz, g_*         adds, a norm, a compare of the norm with 1e-12, products; stored
deform_assemble fwd / bwd           all nine inputs, g           copied; the column index comes from the thread index alone
regress_epilogue fwd / bwd          raw, xyz_in, g_*             exp, sigmoid, two norms, compares with 0.05 / 1e-12 / 0; stored
spatial softmax (ss_fwd, combine,   feature                      fmaxf, exp2 of differences, sums; the arg-max INDEX travels with
 ss_bwd)                                                         the maximum and is only ever compared with element indices (the
                                                                 max-pool's gradient is added where index == arg-max), never
                                                                 dereferenced; combine re-reads a row (0 .. N of that row) where
                                                                 its sum is NaN
                                    g_kp, g_max                  products and adds
FusedLamb (lamb_moments, _apply)    p, g                         moments, two sums of squares, sqrt, compares with 10 and 0, the
                                                                 step; chunk map, sizes and pointers are host tables
layer_norm / bias_geglu             x, weight, bias, g, h        sums, rsqrt, erf / exp, products; stored
conv3d, pointwise, narrow, dense,   x, w, b, g                   staged to LDS or registers at offsets computed from the tile
 patch (+ conv_transpose3d)                                      position; fma / MFMA operands; the activation is a compare of
                                                                 the pre-activation (or y) with 0 and a select or a product
resample_pad (vol_fwd, vol_bwd_*)   sources, g                   taps and weights come from the output index and the scale alone;
                                                                 the values are lerped / summed with those weights; stored
batch_norm_act (abn_stats, _apply,  x, residual, weight, bias,   moments by Chan's merge, rsqrt, a compare of z with 0, sums; the
 abn_bwd_*)                          g, the eval buffers          split of a row comes from N alone
Attention (attn_fwd, _delta, _dq,   x, context, the parameters,  torch GEMMs, then scores, fmaxf, exp2, sums, products; the key mask
 _dkv)                               g                            and the dropout stream are not operands (bool, Philox of indices)
voxelize                            features                     summed per voxel and divided by the count; the voxel comes from
                                                                 the COORDINATES, which are not tainted here
point_latent_pe                     volume, g                    eight corners at indices computed from xyz (not tainted), weighted sums
rendering_loss, photometric_loss    images, targets              differences, squares, norms, min / max, window sums; offsets come
                                                                 from the pixel index and the target's strides

What is not enrolled, and why: NOT_ENROLLED below and DESIGN.md "Non-finite values".

Findings (DESIGN.md has the table).  Fixed in this change, each of these tests failing on the kernels before it and naming operand
and class: relu(NaN) = 0 and a NaN unit's gradient dropped (mgs_mlp.hip); clamp_max(exp(NaN)) = 0.05, its gradient 0 where the
reference has 0 x inf = NaN, normalize of a NaN quaternion = q x 1e12 (mgs_regress.hip, mgs_deform.hip); LAMB's clamped weight norm
10 for a tensor that holds a NaN (mgs_optim.hip); a finite global max-pool for a row that holds a NaN, and +-inf where the reference's
softmax backward has NaN under an infinite keypoint gradient (mgs_spatial_softmax.hip); the dense weight gradient's odd last k-step
multiplying a zero of g' by the NEXT voxel's x (mgs_dense.hip); resample_pad's a + t (b - a) turning an infinite voxel into NaN
where (1 - t) a + t b is the infinity (mgs_volume.hip); the l2_norm min / max of the target embedding and the cosine clamps dropping
a NaN (mgs_loss.hip); batch_norm_act's running mean NaN for a channel that holds an infinity (mgs_abn.hip).

Two more, the idiom this file was written to find (masking by a product with zero: invisible at finite inputs, and a NaN in gradients
that do not depend on the tainted element):
  narrow, x tainted: dw had 18-19 (NaN) or 44 (+-inf) elements NaN where the reference is finite or infinite.  nc_bwd_weight_kernel gave a
    voxel outside the volume g = 0 and still multiplied it by the halo box's x, the clamped copy of a border voxel.  Such voxels are
    now skipped: a thread without voxels leaves, a plane past D is skipped per wave, and a thread that straddles W selects zeros.
  dense, w tainted: dx had 26 (one_out_k3), 546 (m_seam) and 96 (n_seam, k_seam) elements NaN where the reference is finite.
    Backward-data is the forward kernel over g' zero-padded by k - 1, and the padding's zeros met the tainted tap in the MFMA.  A
    non-finite weight now enters that GEMM as a zero and dc_dx_nonfinite_kernel adds its products with the real g' alone.

F.leaky_relu(z, 0), the truth of the patch and dense families at slope 0, is z x 0 = NaN at z = -inf where nn.ReLU gives 0; the
kernels follow F.leaky_relu, as their own tests' truth does.
"""
import importlib
import math
import os
import re

import pytest
import torch

import abn_cases as ac
import attention_cases as atc
import conv_family as cf
import embed_cases as ec
import feedforward_cases as fc
import lamb_cases as lac
import loss_cases as lc
import voxelize_cases as vz
import nonfinite as nf
import photometric_cases as phc
import spatial_softmax_cases as ssc
import volume_cases as vc

gpu = pytest.mark.gpu
ROOT = cf.ROOT
dev = cf.dev
VALUES = list(nf.VALUES)


def _mod(name):
    return importlib.import_module("manigaussian_amd." + name)


def cpu(t):
    return None if t is None else t.detach().cpu()


class Subject:
    """One op on one small case.  inputs() -> {operand: float32 CPU tensor (or something that is never tainted)}; ref(inputs, dtype)
    -> {result: CPU tensor or None}: the op's existing truth; ours(inputs) -> the same results from the library, as CPU tensors;
    taints {operand: {position: flat index}}; free_share: 0 or nonfinite.FREE_SHARE; ceiling: the op's REF_ERR_CEILING; parts: see
    nonfinite.compare."""

    def __init__(self, key, module, inputs, ref, ours, taints, free_share=0.0, ceiling=1e-5, parts=None, bound_fn=nf.default_bound,
                 alt=None, refused=(), reference=None, cap_refuses=True):
        self.key, self.module, self._inputs, self.ref, self.ours, self.taints = key, module, inputs, ref, ours, taints
        self.free_share, self.ceiling, self.parts, self.bound_fn = free_share, ceiling, parts, bound_fn
        # may_refuse: the (operand, value) pairs on which the reference is known not to speak clearly at some position.  Only there may
        # admit() raise Refused; a position at which it does is not compared (there is nothing to compare with), every other one is.
        self.alt, self.may_refuse, self.cap_refuses = alt, tuple(refused), cap_refuses
        # reference_module(inputs, dtype): where `ref` is a restatement written in this repository, the reference's own module on the
        # same inputs (it needs a copy of the reference); have_reference(): whether there is one
        self.reference_module, self.have_reference = reference or (None, None)
        self._made = None

    def inputs(self):
        if self._made is None:
            self._made = self._inputs()
        return self._made

    def admit(self, operand, position, value):
        index = self.taints[operand][position]
        return nf.admit(f"{self.key} {operand}[{position}={index}]={value}", self.ref, self.inputs(), operand, index, nf.VALUES[value],
                        self.free_share, clean_key=self.key, alt=self.alt, cap_refuses=self.cap_refuses)

    def tainted(self, operand, position, value):
        t = dict(self.inputs())
        t[operand] = nf.taint(t[operand], self.taints[operand][position], nf.VALUES[value])
        return t


SUBJECTS = {}


def enrol(s):
    assert s.key not in SUBJECTS
    SUBJECTS[s.key] = s
    return s


# ---- the elementwise passes of the MLP (deform._relu_bias, deform._relu_backward: csrc/mgs_mlp.hip) ---------------------------------
MLP_M, MLP_H = 129, 64   # 128 rows per workgroup of the backward: row 128 is the second workgroup's only row
_MLP_SEAM = 128 * MLP_H + 5


def _mlp_inputs():
    g = torch.Generator().manual_seed(31000)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    t = dict(x=rn(MLP_M, MLP_H), bias=rn(MLP_H), g_pre=rn(MLP_M, MLP_H), g_res=rn(MLP_M, MLP_H))
    t["x"].view(-1)[[0, _MLP_SEAM]] = torch.tensor([0.7, 0.9])   # live units: the upstream gradient passes there
    return t


def _mlp_ref(t, dtype):
    x = t["x"].to(dtype).requires_grad_(True)
    a = torch.relu(x)
    (g,) = torch.autograd.grad(a, x, t["g_pre"].to(dtype))
    g = g + t["g_res"].to(dtype)
    return dict(relu=a.detach(), x_plus_bias=x.detach() + t["bias"].to(dtype), g=g, colsum=g.sum(0))


def _mlp_ours(t):
    d, dfm = dev(), _mod("deform")
    a, xb = dfm._relu_bias(t["x"].to(d), t["bias"].to(d))
    colsum = torch.zeros(MLP_H, device=d)
    g = dfm._relu_backward(t["g_pre"].to(d).clone(), a, t["g_res"].to(d), colsum)
    return dict(relu=cpu(a), x_plus_bias=cpu(xb), g=cpu(g), colsum=cpu(colsum))


enrol(Subject("mlp", "deform", _mlp_inputs, _mlp_ref, _mlp_ours,
              dict(x=dict(first=0, seam=_MLP_SEAM), bias=dict(first=0, seam=MLP_H - 1), g_pre=dict(first=0, seam=_MLP_SEAM),
                   g_res=dict(first=0, seam=_MLP_SEAM))))


# ---- deform_apply and the input assembly (csrc/mgs_deform.hip) -----------------------------------------------------------------------
POINTS = 257   # one thread per point, workgroups of 256: row 256 is the second workgroup's only point


def _apply_inputs():
    delta, xyz, rot, (wx, wr) = ec.apply_inputs(POINTS)
    return dict(delta=delta, xyz=xyz, rot=rot, g_xyz=wx, g_rot=wr)


def _apply_ref(t, dtype):
    (nx, nr), grads = ec.with_grads(ec.apply_fn, [t["delta"], t["xyz"], t["rot"]], [t["g_xyz"], t["g_rot"]], dtype)
    return dict(xyz=nx, rot=nr, g_delta=grads[0])


def _apply_ours(t):
    d = dev()
    delta = t["delta"].to(d).requires_grad_(True)
    nx, nr = _mod("deform").deform_apply(delta, t["xyz"].to(d), t["rot"].to(d))
    torch.autograd.backward([nx, nr], [t["g_xyz"].to(d), t["g_rot"].to(d)])
    return dict(xyz=cpu(nx), rot=cpu(nr), g_delta=cpu(delta.grad))


enrol(Subject("deform_apply", "deform", _apply_inputs, _apply_ref, _apply_ours,
              # (row 0 is embed_cases' zero quaternion, whose normalised form is 0 / eps: row 1 stands for the first one)
              dict(delta=dict(first=0, row1_rot=7 + 3, seam=256 * 7 + 4), xyz=dict(first=0, seam=256 * 3 + 1), rot=dict(row1=4, seam=256 * 4 + 2),
                   g_xyz=dict(first=0, seam=256 * 3 + 2), g_rot=dict(first=0, seam=256 * 4 + 3))))

ASSEMBLY = (POINTS, 32, 16, 8, True)
_ASSEMBLY_KEYS = ("point_latent", "z_feature", "xyz", "sh", "rot", "scale", "opacity", "feature", "action")


def _assembly_inputs():
    a = ec.assembly_inputs(*ASSEMBLY)
    width = 32 + 23 + 3 + 16 + 8
    a["g"] = torch.randn(POINTS, width, generator=torch.Generator().manual_seed(31100))
    return a


def _assembly_ref(t, dtype):
    c = {k: t[k].to(dtype) for k in _ASSEMBLY_KEYS}
    lat, z = c["point_latent"].requires_grad_(True), c["z_feature"].requires_grad_(True)
    out = ec.assembly_exact(c)
    g_lat, g_z = torch.autograd.grad(out, [lat, z], t["g"].to(dtype))
    return dict(assembled=out.detach(), g_point_latent=g_lat, g_z_feature=g_z)


def _assembly_ours(t):
    d = dev()
    c = {k: t[k].to(d) for k in _ASSEMBLY_KEYS}
    lat, z = c["point_latent"].requires_grad_(True), c["z_feature"].requires_grad_(True)
    out = _mod("deform").assemble_deform_input(lat, z, c["xyz"], c["sh"], c["rot"], c["scale"], c["opacity"], c["feature"], c["action"])
    out.backward(t["g"].to(d))
    return dict(assembled=cpu(out), g_point_latent=cpu(lat.grad), g_z_feature=cpu(z.grad))


_ASSEMBLY_TAINTS = {k: dict(first=0, last=-1) for k in _ASSEMBLY_KEYS}
_ASSEMBLY_TAINTS["g"] = dict(first=0, last_row_z=256 * 82 + 32 + 23 + 3 + 15)   # (the columns of everything else take no gradient)
enrol(Subject("deform_assembly", "deform", _assembly_inputs, _assembly_ref, _assembly_ours, _ASSEMBLY_TAINTS))


# ---- the regressor's epilogue (csrc/mgs_regress.hip) -----------------------------------------------------------------------------------
def _epilogue_inputs():
    raw, xyz_in, cot = ec.epilogue_inputs(POINTS)
    ec.epilogue_conditions(raw)
    return dict({"raw": raw, "xyz_in": xyz_in}, **{"g_" + k: v for k, v in cot.items()})


def _epilogue_ref(t, dtype):
    cot = {k: t["g_" + k] for k in ec.EPILOGUE_OUTPUTS}
    out, (g_raw, g_xyz) = ec.with_grads(ec.epilogue_fn, [t["raw"], t["xyz_in"]], cot, dtype)
    return dict(out, g_raw=g_raw, g_xyz_in=g_xyz)


def _epilogue_ours(t):
    d = dev()
    raw, xyz_in = t["raw"].to(d).requires_grad_(True), t["xyz_in"].to(d).requires_grad_(True)
    out = _mod("regressor").gaussian_epilogue(raw, xyz_in)
    torch.autograd.backward([out[k] for k in ec.EPILOGUE_OUTPUTS], [t["g_" + k].to(d) for k in ec.EPILOGUE_OUTPUTS])
    r = {k: cpu(out[k]) for k in ec.EPILOGUE_OUTPUTS}
    r.update(g_raw=cpu(raw.grad), g_xyz_in=cpu(xyz_in.grad))
    return r


def _epilogue_parts(name):
    """The groups of tests/embed_cases.py: the columns of g_raw by what they feed, the zero rows on their own."""
    raw = SUBJECTS["gaussian_epilogue"].inputs()["raw"]
    gs = [g for g in ec.epilogue_groups(raw) if g.key == name]
    if not gs:
        return [(name, lambda t: t)]
    return [(g.name, (lambda t, g=g: g.of({name: t}))) for g in gs]


_RAW_TAINTS = dict(first=0, **{"seam_" + k: 256 * 26 + s.start + (1 if s.stop - s.start > 1 else 0) for k, s in ec.RAW_GROUPS.items()})
# a log-scale below the clamp: above it the output is 0.05 whatever the value, and 2^100 in its place shows no dependence
_RAW_TAINTS["row3_scale"] = 3 * 26 + 5
_EPI_TAINTS = {"raw": _RAW_TAINTS, "xyz_in": dict(first=0, seam=256 * 3 + 1)}
_EPI_TAINTS.update({"g_" + k: dict(first=0, last=-1) for k in ec.EPILOGUE_OUTPUTS})
enrol(Subject("gaussian_epilogue", "regressor", _epilogue_inputs, _epilogue_ref, _epilogue_ours, _EPI_TAINTS, parts=_epilogue_parts))


# ---- SpatialSoftmax3D and the global max-pool (csrc/mgs_spatial_softmax.hip) -----------------------------------------------------------
def _ss_subject(case, slices):
    B, C, D, H, W = ssc.CASES[case]["shape"]
    N = D * H * W

    def inputs():
        x, g_k, g_m = ssc.make_inputs(case)
        return dict(feature=x, g_kp=g_k, g_max=g_m)

    def ref(t, dtype):
        x = t["feature"].to(dtype).requires_grad_(True)
        kp, mx = ssc.restatement(x, D, H, W, ssc.TEMPERATURE, dtype)
        (dx,) = torch.autograd.grad([kp, mx], x, [t["g_kp"].to(dtype), t["g_max"].to(dtype)])
        return dict(keypoints=kp.detach(), maxpool=mx.detach(), dx=dx)

    def module(t, dtype):
        r, _ = ssc._run(ssc.load_reference(), t["feature"], t["g_kp"], t["g_max"], dtype)
        return dict(keypoints=r["kp"], maxpool=r["max"], dx=r["dx"])

    def ours(t):
        d = dev()
        x = t["feature"].to(d).requires_grad_(True)
        kp, mx = _mod("spatial_softmax")._spatial_softmax3d(x, ssc.TEMPERATURE, slices=slices)
        torch.autograd.backward([kp, mx], [t["g_kp"].to(d), t["g_max"].to(d)])
        return dict(keypoints=cpu(kp), maxpool=cpu(mx), dx=cpu(x.grad))

    def bound_fn(truth, ref32, ceiling):
        """tests/spatial_softmax_cases.py: keypoints live in [-1, 1] and are bounded absolutely."""
        if truth.numel() == 0:
            return 0.0, 0.0, 0.0
        mag = truth.abs().max().item()
        err = (ref32.double() - truth).abs().max().item()
        assert err <= ssc.REF_ERR_CEILING * max(mag, 1.0), (err, mag)
        return max(ssc.FACTOR * err, ssc.FACTOR * ssc.KP_FLOOR * max(mag, 1.0)), err, mag

    # a row's last element (the scalar tail, the last slice) of the second row, whose start is misaligned where N is odd
    taints = dict(feature=dict(first=0, seam=2 * N - 1, middle=N + N // 2), g_kp=dict(first=0, last=-1), g_max=dict(first=0, last=-1))
    return Subject(f"spatial_softmax {case} slices{slices}", "spatial_softmax", inputs, ref, ours, taints, ceiling=ssc.REF_ERR_CEILING,
                   bound_fn=bound_fn, reference=(module, ssc.have_reference) if slices == 0 else None)


for _case, _slices in (("tiny", 0), ("noncube", 0), ("noncube", 2)):
    enrol(_ss_subject(_case, _slices))


# ---- FusedLamb (csrc/mgs_optim.hip) ---------------------------------------------------------------------------------------------------
LAMB_SHAPES = [(5,), (4097,), (13, 79)]   # one chunk with a ragged group; two chunks, the second of one element; 1027 elements


def _lamb_subject(wd):
    case = dict(shapes=LAMB_SHAPES, groups=[dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=wd)], K=1, seed=41)
    n = len(LAMB_SHAPES)

    def inputs():
        inp = lac.make_inputs(case)
        t = {f"p{i}": p for i, p in enumerate(inp["params"])}
        t.update({f"g{i}": g for i, g in enumerate(lac.gradients(inp, 0))})
        t["inp"] = inp
        return t

    def ref(t, dtype):
        r = lac.restate(t["inp"], dtype, params=[t[f"p{i}"] for i in range(n)], grads_of_step=lambda k: [t[f"g{i}"] for i in range(n)], K=1)
        out = {"stats": r["stats"][0].to(dtype)}
        for i in range(n):
            out[f"p{i}"], out[f"m{i}"], out[f"v{i}"] = r["p"][i], r["m"][i], r["v"][i]
        return out

    def module(t, dtype):
        ps = [torch.nn.Parameter(t[f"p{i}"].to(dtype).clone()) for i in range(n)]
        opt = lac.reference_class()([dict(params=ps, **case["groups"][0])])
        for i, p in enumerate(ps):
            p.grad = t[f"g{i}"].to(dtype).clone()
        opt.step()
        st = [[torch.as_tensor(opt.state[p][k], dtype=dtype).reshape(()) for k in ("weight_norm", "adam_norm", "trust_ratio")] for p in ps]
        out = {"stats": torch.stack([torch.stack(s) for s in st])}
        for i, p in enumerate(ps):
            out[f"p{i}"], out[f"m{i}"], out[f"v{i}"] = p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]
        return out

    def ours(t):
        d = dev()
        ps = [t[f"p{i}"].to(d).requires_grad_(True) for i in range(n)]
        opt = _mod("optim").FusedLamb([dict(params=ps, **{k: v for k, v in case["groups"][0].items()})])
        for i, p in enumerate(ps):
            p.grad = t[f"g{i}"].to(d)
        opt.step()
        out = {"stats": torch.stack([torch.stack([opt.state[p][k] for k in ("weight_norm", "adam_norm", "trust_ratio")]) for p in ps]).cpu()}
        for i, p in enumerate(ps):
            out[f"p{i}"], out[f"m{i}"], out[f"v{i}"] = cpu(p), cpu(opt.state[p]["exp_avg"]), cpu(opt.state[p]["exp_avg_sq"])
        return out

    def parts(name):
        if name != "stats":
            return [(name, lambda t: t)]
        return [(f"stats[{i}].{what}", (lambda t, i=i, j=j: t[i, j].reshape(1))) for i in range(n)
                for j, what in enumerate(("weight_norm", "adam_norm", "trust_ratio"))]

    def bound_fn(truth, ref32, ceiling):
        """tests/lamb_cases.py: EPS_REL of the largest magnitude (one step: the parameter's path is at most its largest step, which
        is itself bounded by EPS_REL of the largest parameter)."""
        if truth.numel() == 0:
            return 0.0, 0.0, 0.0
        mag = truth.abs().max().item()
        return lac.EPS_REL * mag, (ref32.double() - truth).abs().max().item() / mag if mag else 0.0, mag

    taints = {}
    for i, s in enumerate(LAMB_SHAPES):
        numel = 1
        for e in s:
            numel *= e
        taints[f"p{i}"] = dict(first=0, last=numel - 1)
        taints[f"g{i}"] = dict(first=0, last=numel - 1)
    return Subject(f"fused_lamb wd{wd:g}", "optim", inputs, ref, ours, taints, parts=parts, bound_fn=bound_fn,
                   reference=(module, lac.have_reference))


for _wd in (0.0, 1e-2):
    enrol(_lamb_subject(_wd))


# ---- LayerNorm and bias-GEGLU (csrc/mgs_feedforward.hip) -------------------------------------------------------------------------------
def _ff_subject(kind, case):
    ln = kind == "layer_norm"
    names = ("x", "weight", "bias", "g") if ln else ("h", "bias", "g")
    compose = fc.ln_compose if ln else fc.geglu_compose

    def inputs():
        return dict(zip(names, (t.contiguous() for t in (fc.ln_inputs(case) if ln else fc.geglu_inputs(case)))))

    def run(t, dtype, device, fn):
        r = fc.run_op(fn, [t[k] for k in names[:-1]], t["g"], dtype, device)
        return {("out" if k == "out" else "d_" + names[int(k[1:])]): cpu(v) for k, v in r.items()}

    def ref(t, dtype):
        return run(t, dtype, "cpu", compose)

    def decomposed(x, w, b):
        mean, var = x.mean(-1, keepdim=True), x.var(-1, unbiased=False, keepdim=True)
        return (x - mean) / torch.sqrt(var + fc.EPS) * w + b

    def alt(t, dtype):
        return run(t, dtype, "cpu", decomposed)

    def ours(t):
        ff = _mod("feedforward")
        return run(t, torch.float32, dev(), (lambda x, w, b: ff.layer_norm(x, w, b, fc.EPS)) if ln else (lambda h, b: ff.bias_geglu(h, b)))

    shapes = {k: tuple(v.shape) for k, v in inputs().items()}
    rows, width = shapes[names[0]]
    # the last row's last element; a parameter's last element (D and 2 M are no multiples of 4 in these cases: a ragged last group)
    taints = {k: dict(first=0, last=-1) for k in names}
    taints[names[0]]["seam"] = (rows // 2) * width + width // 2
    # F.layer_norm's backward is one fused kernel.  Under an infinite weight or upstream gradient the row's two sums are infinite
    # and d_x = rstd (g w - mean(g w) - xhat mean(g w xhat)) holds inf - inf: NaN or +-inf, element by element, by the order in
    # which a kernel happens to combine the terms.  torch's CPU kernel and the same formula through autograd's primitive ops
    # disagree on those elements of d_x, and they alone are exempt (nonfinite.admit's `alt`).
    return Subject(f"{kind} {case}", "feedforward", inputs, ref, ours, taints, alt=alt if ln else None)


for _case in ("r3_d5", "r65_d130"):
    enrol(_ff_subject("layer_norm", _case))
for _case in ("r3_m3", "r65_m130"):
    enrol(_ff_subject("bias_geglu", _case))


# ---- the five Conv3d families and conv_transpose3d ---------------------------------------------------------------------------------------
CONV_CASES = {
    "conv3d": ("tiny", "seam_tile", "seam_tile_s2", "up_odd"),
    "pointwise": ("one_voxel", "odd", "seam_16"),
    "narrow": ("two", "seam_h", "odd_zeros"),
    "dense": ("one_out_k3", "m_seam", "n_seam", "k_seam"),
    "patch": ("one_patch", "seam_m", "seam_k", "k2"),
}


def _conv_torchs(name, case):
    m = cf.FAMILIES[name].cases
    if name == "conv3d":
        return lambda t, dtype: m.torchs(case, t, dtype)
    if name == "pointwise":
        return m.torchs
    if name == "narrow":
        return lambda t, dtype: m.torchs(t, dtype, m.mode_of(case))
    if name == "dense":
        return lambda t, dtype: m.torchs(t, dtype, m.slope_of(case))
    return lambda t, dtype: m.torchs(t, dtype, case)


def _centre(shape, lead):
    """The flat index of the centre voxel / tap of entry `lead` (a flat index over the two leading dimensions) of a 5-D tensor."""
    d, h, w = shape[2:]
    return lead * d * h * w + (d // 2) * h * w + (h // 2) * w + w // 2


def _conv_subject(name, case):
    family = cf.FAMILIES[name]
    torchs = _conv_torchs(name, case)

    def inputs():
        return {k: v for k, v in family.cases.make_inputs(case).items() if k in ("x", "w", "b", "g")}

    def ref(t, dtype):
        t = dict(t)
        t.setdefault("b", None)
        r = torchs(t, dtype)
        return {q: r[q] for q in family.cases.quantities(case)}

    def ours(t):
        r = cf.run(family, case, **{k: v.to(dev()) for k, v in t.items() if v is not None})
        return {q: r[q] for q in family.cases.quantities(case)}

    t = inputs()
    taints = {}
    for k in ("x", "w", "g"):
        s = t[k].shape
        taints[k] = dict(centre_first=_centre(s, 0), centre_last=_centre(s, s[0] * s[1] - 1))
    if getattr(family.cases, "slope_of", lambda c: None)(case) == 0.0:
        # a ReLU: the upstream gradient of a dead unit is multiplied by the slope, an exact zero -- every element it reaches would be
        # free.  The taint goes to the nearest live unit (the float64 pre-activation of the untainted case is positive there).
        live = (family.cases.reference(case)["z64"].reshape(-1) > 0).nonzero().reshape(-1)
        taints["g"] = {p: int(live[(live - i).abs().argmin()]) for p, i in taints["g"].items()}
    if not (name == "conv3d" and family.cases.is_transposed(case)):
        taints["x"]["first"] = 0     # (conv_transpose3d: torch's float32 and float64 weight gradients disagree on the corner voxel)
    if name in ("pointwise", "dense"):   # no padding: the last voxel is as good as any; with padding it is a corner, mostly free
        taints["g"]["last"] = t["g"].numel() - 1
    if t.get("b") is not None:
        taints["b"] = dict(first=0, last=-1)
    return Subject(f"{name} {case}", name, inputs, ref, ours, taints, free_share=nf.FREE_SHARE, ceiling=family.cases.REF_ERR_CEILING)


for _name, _cases in CONV_CASES.items():
    for _case in _cases:
        enrol(_conv_subject(_name, _case))


# ---- resample_pad: trilinear upsample, concat and replicate pad (csrc/mgs_volume.hip) -------------------------------------------------
def _volume_subject(case):
    shapes, scale, pad = vc.CASES[case]
    n = len(shapes)

    def inputs():
        t = {f"source{k}": s.contiguous() for k, s in enumerate(vc.make_sources(case))}
        t["g"] = vc.make_upstream(case)
        return t

    def ref(t, dtype):
        out, grads = vc.compose_with_grads([t[f"source{k}"] for k in range(n)], t["g"], scale, pad, dtype)
        return dict({"out": out}, **{f"g_source{k}": g for k, g in enumerate(grads)})

    def ours(t):
        d = dev()
        sources = [t[f"source{k}"].to(d).requires_grad_(True) for k in range(n)]
        out = _mod("volume").resample_pad(sources, scale, pad)
        out.backward(t["g"].to(d))
        return dict({"out": cpu(out)}, **{f"g_source{k}": cpu(s.grad) for k, s in enumerate(sources)})

    def at(shape, lead, zyx):
        return ((lead * shape[2] + zyx[0]) * shape[3] + zyx[1]) * shape[4] + zyx[2]

    # At scale 2 the source coordinate of output 0 is clamped to 0: weight 1 on voxel 0 and an exact 0 on voxel 1, so a taint on
    # index 1 of an axis (and an upstream gradient's on the outputs that clamp) is mostly free.  Sources: the first voxel -- a
    # corner, which the replicate pad copies (p + 1)^3 times -- and the far voxel of the last (batch, channel), index 0 where an axis
    # has two; upstream: one output inside the pad's border on every axis (source coordinate 0.25), and the last such one.
    t = inputs()
    taints = {}
    for k, v in t.items():
        s = v.shape
        if k == "g":
            taints[k] = dict(near=at(s, 0, [pad + 1] * 3), far=at(s, s[0] * s[1] - 1, [e - pad - 2 for e in s[2:]]))
        else:
            taints[k] = dict(first=0, far_last=at(s, s[0] * s[1] - 1, [e - 1 if e != 2 else 0 for e in s[2:]]))
    return Subject(f"resample_pad {case}", "volume", inputs, ref, ours, taints, free_share=nf.FREE_SHARE, ceiling=vc.REF_ERR_CEILING)


for _case in ("cat_pad1", "cat3_up2"):   # (an odd scale has weights that are 0 in float64 and not in float32: refused outright)
    enrol(_volume_subject(_case))


# ---- rendering_loss (csrc/mgs_loss.hip) ------------------------------------------------------------------------------------------------
def _loss_restated(t, dtype, c):
    """loss.py's l2_loss and cosine_loss, NeuralRenderer._embed_loss_fn and PSNR_torch in plain torch ops, view by view, accumulated as
    neural_rendering.py:305-329 does; held to the reference's own functions class for class by the fixtures."""
    V = c["V"]
    w = c["weights"] or [(1.0, 1.0)] * V
    col, fea = t["color"].to(dtype).requires_grad_(True), t["feature"].to(dtype).requires_grad_(True)
    gt_rgb, gt_emb = t["gt_rgb"].to(dtype), t["gt_embed"].to(dtype)
    loss, terms = 0.0, []
    for v in range(V):
        x, e = col[v:v + 1].permute(0, 2, 3, 1), fea[v:v + 1].permute(0, 2, 3, 1)
        mse = ((x - gt_rgb[v:v + 1]) ** 2).mean()
        psnr = torch.tensor(100.0, dtype=dtype) if mse == 0 else 20 * torch.log10(1 / torch.sqrt(mse))
        g = gt_emb[v:v + 1]
        if c["fn"] == "cosine":
            emb = 1 - torch.nn.functional.cosine_similarity(e, g, dim=-1).mean()
        else:
            if c["fn"] == "l2_norm":
                g = (g - g.min()) / (g.max() - g.min() + 1e-12)
            emb = ((e - g) ** 2).mean()
        loss = loss + w[v][0] * mse
        loss = loss + w[v][1] * emb
        terms.append(torch.stack([mse.detach(), emb.detach(), psnr.detach()]))
    loss.backward()
    return dict(loss=loss.detach().reshape(1), terms=torch.stack(terms), g_color=col.grad, g_feature=fea.grad)


def _loss_subject(name, c):
    V, H, W, F = c["V"], c["H"], c["W"], c["F"]
    N = H * W

    def inputs():
        return dict(lc.make_inputs(c)[0])

    def ref(t, dtype):
        return _loss_restated(t, dtype, c)

    def module(t, dtype):
        assert dtype == torch.float64
        r = lc.reference(c, t)
        return dict(loss=r["loss"].reshape(1), terms=r["terms"], g_color=r["g_color"], g_feature=r["g_feature"])

    def ours(t):
        d = dev()
        color, feature = t["color"].to(d).requires_grad_(True), t["feature"].to(d).requires_grad_(True)
        gt_rgb, gt_embed = lc.lay_out(t["gt_rgb"], c["layout"][0]).to(d), lc.lay_out(t["gt_embed"], c["layout"][1]).to(d)
        loss, terms = _mod("losses").rendering_loss(color, gt_rgb, feature, gt_embed, weights=c["weights"], embed_loss_fn=c["fn"])
        loss.backward()
        return dict(loss=cpu(loss).reshape(1), terms=torch.stack([cpu(terms[k]) for k in ("loss_rgb", "loss_embed", "psnr")], 1),
                    g_color=cpu(color.grad), g_feature=cpu(feature.grad))

    def parts(k):
        """tests/loss_cases.py's bounds: every scalar on its own; a gradient per view (each view has its own weight); the cosine
        gradient per pixel relative to 1 / max(|e_p|, 1e-8), i.e. multiplied by that norm (the untainted feature's) first."""
        if k == "loss":
            return [(k, lambda t: t)]
        if k == "terms":
            return [(f"terms[{v}].{n}", (lambda t, v=v, j=j: t[v, j].reshape(1))) for v in range(V) for j, n in enumerate(("mse", "embed", "psnr"))]
        out = []
        for v in range(V):
            if k == "g_feature" and c["fn"] == "cosine":
                norm = SUBJECTS[name].inputs()["feature"][v].double().norm(dim=0).clamp_min(lc.COS_EPS)
                out.append((f"{k}[{v}] x |e|", (lambda t, v=v, norm=norm: t[v] if t.dtype == torch.bool else
                                                (t[v].double() * norm).to(t.dtype))))
            else:
                out.append((f"{k}[{v}]", (lambda t, v=v: t[v])))
        return out

    def bound_fn(truth, ref32, ceiling):
        """1e-5 of the largest magnitude (psnr: 1e-4 dB)."""
        if truth.numel() == 0:
            return 0.0, 0.0, 0.0
        mag = truth.abs().max().item()
        return 1e-5 * mag, (ref32.double() - truth).abs().max().item() / mag if mag else 0.0, mag

    # the first element, and the last one of view 0: the last pixel, in the second workgroup of 1024 pixels (the last view of
    # ManiGaussian's weights has an embedding weight of exactly 0: its taint would reach the loss through that zero alone)
    px = N - 1
    taints = dict(color=dict(first=0, view0_last=3 * N - 1), feature=dict(first=0, view0_last=F * N - 1),
                  gt_rgb=dict(first=0, view0_last=3 * N - 1), gt_embed=dict(first=0, view0_last=F * N - 1))
    assert N > 1024 and px >= 1024
    return Subject(name, "losses", inputs, ref, ours, taints, parts=parts, bound_fn=bound_fn, reference=(module, lc.have_reference))


for _name, _c in (("rendering_loss cosine", dict(V=2, H=40, W=27, F=5, fn="cosine", layout=("last", "first"), weights=lc.MANI, seed=21)),
                  ("rendering_loss l2_norm", dict(V=1, H=33, W=32, F=8, fn="l2_norm", layout=("last", "last"), weights=[(1.0, 0.01)], seed=22)),
                  ("rendering_loss l2", dict(V=2, H=40, W=27, F=3, fn="l2", layout=("first", "last"), weights=lc.MANI, seed=23))):
    enrol(_loss_subject(_name, _c))


# ---- the voxelizer's features (csrc/mgs_voxelize.hip) -----------------------------------------------------------------------------------
def _voxelizer_subject(case):
    def inputs():
        coords, features, bounds, V = vz.make_inputs(case)
        return dict(features=features, coords=coords, bounds=bounds, V=V)

    def ref(t, dtype):   # (the op has one correct float32 result: the restatement is float32 whatever is asked for)
        return dict(grid=vz.restate(t["coords"], t["features"], t["bounds"], t["V"]))

    def module(t, dtype):
        return dict(grid=vz.reference_run(t["coords"], t["features"], t["bounds"], t["V"]))

    def ours(t):
        d = dev()
        return dict(grid=cpu(_mod("voxelizer").voxelize(t["coords"].to(d), t["features"].to(d), t["bounds"].to(d), t["V"])).contiguous())

    def bound_fn(truth, ref32, ceiling):
        return 0.0, 0.0, (truth.abs().max().item() if truth.numel() else 0.0)   # bit for bit, as tests/test_voxelizer.py has it

    t = inputs()
    keep, _ = vz.voxel_indices(t["coords"], t["bounds"], t["V"])
    kept = keep.reshape(-1).nonzero().reshape(-1)
    Fc = t["features"].shape[-1]
    # a NaN feature makes exactly its voxel's mean NaN, in that channel: the first and the last point that lands in the grid
    taints = dict(features=dict(first_kept=int(kept[0]) * Fc, last_kept=int(kept[-1]) * Fc + Fc - 1))
    return Subject(f"voxelizer {case}", "voxelizer", inputs, ref, ours, taints, bound_fn=bound_fn, reference=(module, vz.have_reference))


for _case in ("fc8", "dense_v8"):
    enrol(_voxelizer_subject(_case))


# ---- batch_norm_act (csrc/mgs_abn.hip) --------------------------------------------------------------------------------------------------
def _abn_subject(case):
    c = ac.CASES[case]
    training, slope = c.get("training", True), ac.slope_of(case)
    keys = ("x", "residual", "g", "weight", "bias") + (() if training else ("running_mean0", "running_var0"))

    def inputs():
        f = ac.load_fixture(case)
        return {k: f[k] for k in keys if k in f}

    def run_ref(t, dtype, normalise):
        x, w, b = (t[k].to(dtype).requires_grad_(True) for k in ("x", "weight", "bias"))
        res = t["residual"].to(dtype).requires_grad_(True) if "residual" in t else None
        running = None if training else (t["running_mean0"], t["running_var0"])
        y, mean, unbiased = normalise(x, w, b, res, running, dtype)
        out = {"y": y.detach()}
        if training:
            grads = torch.autograd.grad(y, [x, w, b] + ([res] if res is not None else []), t["g"].to(dtype))
            rm, rv = ac.running_after_one_step(mean.detach(), unbiased.detach())
            out.update(dx=grads[0], dweight=grads[1], dbias=grads[2], running_mean=rm, running_var=rv)
            if res is not None:
                out["dres"] = grads[3]
        return out

    def ref(t, dtype):
        def normalise(x, w, b, res, running, dtype):
            y, _, mean, unbiased = ac.restatement(x, w, b, res, slope, dtype, running)
            return y, mean, unbiased
        return run_ref(t, dtype, normalise)

    def alt(t, dtype):
        """nn.BatchNorm3d's own fused op (what the reference's InPlaceABN runs) in place of the restatement's primitive ops."""
        def normalise(x, w, b, res, running, dtype):
            C = x.shape[1]
            rm = torch.zeros(C, dtype=dtype) if running is None else running[0].to(dtype).clone()
            rv = torch.ones(C, dtype=dtype) if running is None else running[1].to(dtype).clone()
            z = torch.nn.functional.batch_norm(x, rm, rv, w, b, training, 1.0, ac.EPS)   # (momentum 1: the buffers ARE the batch's)
            y = torch.nn.functional.leaky_relu(z, slope)
            return (y if res is None else res + y), rm, rv
        return run_ref(t, dtype, normalise)

    def ours(t):
        d = dev()
        x, w, b = (t[k].to(d).clone().requires_grad_(True) for k in ("x", "weight", "bias"))
        res = t["residual"].to(d).clone().requires_grad_(True) if "residual" in t else None
        C = w.numel()
        rm = torch.zeros(C, device=d) if training else t["running_mean0"].to(d).clone()
        rv = torch.ones(C, device=d) if training else t["running_var0"].to(d).clone()
        nbt = torch.zeros((), dtype=torch.int64, device=d)
        y = _mod("encoder")._batch_norm_act(x, w, b, rm, rv, nbt, training, ac.MOMENTUM, ac.EPS, slope, res, slices=0)
        out = {"y": cpu(y)}
        if training:
            y.backward(t["g"].to(d))
            out.update(dx=cpu(x.grad), dweight=cpu(w.grad), dbias=cpu(b.grad), running_mean=cpu(rm), running_var=cpu(rv))
            if res is not None:
                out["dres"] = cpu(res.grad)
        return out

    t = inputs()
    n = t["x"][0, 0].numel()
    taints = {k: dict(first=0, last=-1) for k in t if training or k != "g"}
    taints["x"]["row1_tail"] = 2 * n - 1   # the last element of the second (batch, channel) row: its scalar tail where n is odd
    # Under an infinite g the backward's dx = w rstd (g - mean(g) - xhat mean(g xhat)) holds inf - inf, as layer_norm's does, and under
    # an infinite weight y = x (w rstd) + (b - mean w rstd) does in torch's fused batch_norm: the elements on which that op and the
    # restatement disagree are exempt, every other one is compared.
    return Subject(f"batch_norm_act {case}", "encoder", inputs, ref, ours, taints, ceiling=ac.REF_ERR_CEILING, alt=alt)


for _case in ("tiny", "odd", "eval"):
    enrol(_abn_subject(_case))


# ---- point_latent_pe's volume (csrc/mgs_voxel.hip) --------------------------------------------------------------------------------------
PL_CASE = ((2, 3, 4), 8, 6, POINTS)
assert PL_CASE in ec.VOXEL_CASES


def _pl_inputs():
    vox, xyz, cot = ec.voxel_inputs(PL_CASE)
    return dict(volume=vox, g=cot, xyz=xyz)


def _pl_ref(t, dtype):
    _, C, K, _ = PL_CASE
    leaf = t["volume"].to(dtype).clone().requires_grad_(True)
    tri = ec.trilinear(leaf, t["xyz"], dtype)
    (g_vox,) = torch.autograd.grad(tri, leaf, t["g"][:, :C].to(dtype))
    x32 = ec.canon32(t["xyz"])
    return dict(latent=torch.cat([tri.detach(), x32.to(dtype), ec.positional(x32, K, dtype)], 1), g_voxel=g_vox.reshape(C, -1).t())


def _pl_ours(t):
    d = dev()
    _, C, K, _ = PL_CASE
    vox = t["volume"].to(d).requires_grad_(True)
    out = _mod("voxel").point_latent_pe(vox, t["xyz"].to(d), ec.BOUNDS, K)
    out.backward(t["g"].to(d))
    return dict(latent=cpu(out), g_voxel=cpu(vox.grad).reshape(C, -1).t())


def _pl_parts(name):
    gs = [g for g in ec.voxel_groups(PL_CASE) if g.key == name]
    return [(g.name, (lambda t, g=g: g.of({name: t}))) for g in gs]


def _pl_at(c, z, y, x):
    D, H, W = PL_CASE[0]
    return ((c * D + z) * H + y) * W + x


# Voxels no point put on the box on purpose (rows 0 to 5 of tests/embed_cases.py's inputs) has as a corner of weight exactly 0 or 1;
# upstream rows of ordinary points, in the columns of the trilinear part.
_PL_WIDTH = PL_CASE[1] + 3 + 6 * PL_CASE[2]
enrol(Subject("point_latent_pe", "voxel", _pl_inputs, _pl_ref, _pl_ours,
              dict(volume=dict(inner_first=_pl_at(0, 0, 1, 1), inner_last=_pl_at(PL_CASE[1] - 1, 1, 1, 2)),
                   g=dict(row6=6 * _PL_WIDTH, last_row=256 * _PL_WIDTH + PL_CASE[1] - 1)),
              free_share=nf.FREE_SHARE, parts=_pl_parts))


# ---- the Perceiver's attention (csrc/mgs_attention.hip) ----------------------------------------------------------------------------------
def _attention_subject(case):
    c = atc.CASES[case]
    B, H, Nq, Nk, p = c["B"], c["H"], c["Nq"], c["Nk"], c["p"]
    p32 = float(torch.tensor(p, dtype=torch.float32))
    keep = torch.from_numpy(atc.keep_mask(*c["rng"], B * H, Nq, Nk, p)).view(B, H, Nq, Nk) if p > 0 else None
    operands = ("x",) + (("context",) if c["cd"] is not None else ()) + atc.PARAMS + ("g",)

    def inputs():
        x, context, mask, grad, params = atc.make_inputs(case)
        t = dict(params, x=x, g=grad, mask=mask)
        if context is not None:
            t["context"] = context
        return t

    def ref(t, dtype):
        """perceiver_lang_io.py:102's Attention in plain torch calls, the parameters as leaves; the dropout mask is the library's."""
        leaves = {k: t[k].to(dtype).requires_grad_(True) for k in operands if k != "g"}
        x, ctx = leaves["x"], leaves.get("context", leaves["x"])
        q = x @ leaves["to_q.weight"].t()
        k, v = (ctx @ leaves["to_kv.weight"].t()).chunk(2, dim=-1)
        q, k, v = (u.reshape(B, u.shape[1], H, -1).transpose(1, 2) for u in (q, k, v))
        sim = q @ k.transpose(-1, -2) * atc.DIM_HEAD ** -0.5
        if t["mask"] is not None:
            sim = sim.masked_fill(~t["mask"][:, None, None, :], -torch.finfo(dtype).max)
        attn = sim.softmax(dim=-1)
        if p > 0:
            attn = attn * (keep.to(dtype) / (1.0 - p32))
        out = (attn @ v).transpose(1, 2).reshape(B, Nq, -1) @ leaves["to_out.weight"].t() + leaves["to_out.bias"]
        names = list(leaves)
        grads = torch.autograd.grad(out, [leaves[n] for n in names], t["g"].to(dtype))
        return dict({"out": out.detach()}, **{"d" + n: g for n, g in zip(names, grads)})

    def module(t, dtype):
        m = atc.load_reference().Attention(c["qd"], context_dim=c["cd"], heads=H, dim_head=atc.DIM_HEAD, dropout=p)
        m.load_state_dict({n: t[n] for n in atc.PARAMS}, strict=True)
        m.train()
        if p > 0:
            m.dropout = atc.FixedDropout(keep.reshape(B * H, Nq, Nk), p32)
        return atc._run(m, t["x"], t.get("context"), t["mask"], t["g"], dtype)

    def ours(t):
        from manigaussian_amd import Attention
        d = dev()
        m = Attention(c["qd"], context_dim=c["cd"], heads=H, dim_head=atc.DIM_HEAD, dropout=p)
        m.load_state_dict({n: t[n] for n in atc.PARAMS}, strict=True)
        m = m.to(d).train()
        if p > 0:
            m.manual_seed(*c["rng"])
        x = t["x"].to(d).requires_grad_(True)
        context = t["context"].to(d).requires_grad_(True) if "context" in t else None
        out = m(x, context=context, mask=None if t["mask"] is None else t["mask"].to(d))
        out.backward(t["g"].to(d))
        r = dict(out=cpu(out), dx=cpu(x.grad))
        if context is not None:
            r["dcontext"] = cpu(context.grad)
        r.update({"d" + n: cpu(prm.grad) for n, prm in m.named_parameters()})
        return r

    # the first element and the last: the last query, the last key (the ragged end of the last 64-wide tile), the last output column.
    # With a key mask or dropout a third or more of the keys have a weight of exactly 0, and with one live key the softmax is 1
    # whatever the logit: at every position most of what a taint reaches is free, and the cap of an eighth refuses nearly every
    # taint of these four cases.  They are compared all the same, at every element that is not free (cap_refuses=False); one_query,
    # without mask or dropout, is held to the cap.
    taints = {k: dict(first=0, last=-1) for k in operands}
    key = f"attention {case}"

    def bound_fn(truth, ref32, ceiling):
        """tests/attention_cases.py's rule for a gradient that is exactly zero (one key: the softmax is 1 whatever q): ZERO_BOUND of the
        largest magnitude among the untainted case's gradients."""
        bnd, yard, mag = nf.default_bound(truth, ref32, ceiling)
        if truth.numel() and mag == 0.0:
            other = max(v.abs().max().item() for k, v in nf._CLEAN[key].items() if k != "out")
            return atc.ZERO_BOUND * other, yard, mag
        return bnd, yard, mag

    return Subject(key, "attention", inputs, ref, ours, taints, free_share=nf.FREE_SHARE, ceiling=1e-4, bound_fn=bound_fn,
                   reference=(module, atc.have_reference), cap_refuses=case == "one_query")


for _case in ("one_key", "one_query", "masked", "last_tiles_masked", "dropout_p50_masked"):
    enrol(_attention_subject(_case))


# ---- photometric_loss (csrc/mgs_photometric.hip) ----------------------------------------------------------------------------------------
PHOTO = dict(V=1, C=3, H=23, W=37, cls="smooth", layout="last", weights=[(0.3, 1.0, 0.5)], seed=3)   # odd_37x23's second view: no zero weight


def _photo_window(dtype):
    """The 11 x 11 Gaussian window (sigma 1.5) as the reference builds it: float32 values, whatever the images' type."""
    k = torch.tensor([math.exp(-(i - 5) ** 2 / (2 * 1.5 ** 2)) for i in range(11)])
    k = (k / k.sum()).unsqueeze(1)
    return k.mm(k.t()).float().to(dtype)


def _photo_restated(t, dtype):
    """L1, L2, SSIM (Gaussian window, zero padding, C1 = 0.01^2, C2 = 0.03^2) and PSNR in plain torch ops, view by view; held to the
    reference's own functions class for class by the fixtures."""
    c, conv = PHOTO, torch.nn.functional.conv2d
    col, tgt = t["color"].to(dtype).requires_grad_(True), t["target"].to(dtype)
    win = _photo_window(dtype).expand(c["C"], 1, 11, 11).contiguous()
    loss, terms = 0.0, []
    for v, (w1, w2, w3) in enumerate(phc.weights_of(c)):
        x, y = col[v:v + 1], tgt[v:v + 1]
        l1, l2 = (x - y).abs().mean(), ((x - y) ** 2).mean()
        blur = lambda a: conv(a, win, padding=5, groups=c["C"])  # noqa: E731
        m1, m2 = blur(x), blur(y)
        s1, s2, s12 = blur(x * x) - m1.pow(2), blur(y * y) - m2.pow(2), blur(x * y) - m1 * m2
        ss = (((2 * m1 * m2 + 1e-4) * (2 * s12 + 9e-4)) / ((m1.pow(2) + m2.pow(2) + 1e-4) * (s1 + s2 + 9e-4))).mean()
        psnr = 20 * torch.log10(1.0 / torch.sqrt(l2)) if l2.item() != 0 else torch.tensor(100.0, dtype=dtype)
        loss = loss + w1 * l1
        loss = loss + w2 * l2
        loss = loss + w3 * (1 - ss)
        terms.append(torch.stack([l1.detach(), l2.detach(), ss.detach(), psnr.detach().reshape(())]))
    (g,) = torch.autograd.grad(loss, [col])
    return dict(loss=loss.detach().reshape(1), terms=torch.stack(terms), g_color=g)


def _photo_module(t, dtype):
    r = phc.reference(PHOTO, t, dtype)
    return dict(loss=r["loss"].reshape(1), terms=r["terms"], g_color=r["g"])


def _photo_ours(t):
    d = dev()
    color = t["color"].to(d).requires_grad_(True)
    loss, terms = _mod("photometric").photometric_loss(color, phc.lay_out(t["target"], PHOTO["layout"]).to(d), weights=PHOTO["weights"])
    loss.backward()
    return dict(loss=cpu(loss).reshape(1), terms=torch.stack([cpu(terms[k]) for k in ("l1", "l2", "ssim", "psnr")], 1), g_color=cpu(color.grad))


def _photo_parts(k):
    if k != "terms":
        return [(k, lambda t: t)]
    return [(f"terms.{n}", (lambda t, j=j: t[:, j])) for j, n in enumerate(("l1", "l2", "ssim", "psnr"))]


# the first pixel (a corner: its windows are mostly padding) and one in the middle of the image, across tile seams both ways
_PHOTO_MID = (1 * 23 + 16) * 37 + 17
enrol(Subject("photometric_loss", "photometric", lambda: dict(phc.make_inputs(PHOTO)), _photo_restated, _photo_ours,
              dict(color=dict(first=0, middle=_PHOTO_MID), target=dict(first=0, middle=_PHOTO_MID)), ceiling=1e-4, parts=_photo_parts,
              reference=(_photo_module, phc.have_reference)))


# ---- enrolment -----------------------------------------------------------------------------------------------------------------------------
# module -> operands whose values are tainted here.  An operand is enrolled iff no kernel turns its value into an address, a loop bound
# or a discrete choice other than an activation branch or a maximum.
ENROLLED = {
    "conv3d": ("x", "w", "g"), "pointwise": ("x", "w", "b", "g"), "narrow": ("x", "w", "b", "g"), "dense": ("x", "w", "b", "g"),
    "patch": ("x", "w", "b", "g"),
    "feedforward": ("x", "weight", "bias", "g", "h"),
    "spatial_softmax": ("feature", "g_kp", "g_max"),
    "regressor": ("raw", "xyz_in") + tuple("g_" + k for k in ec.EPILOGUE_OUTPUTS),
    "deform": ("x", "bias", "g_pre", "g_res", "delta", "xyz", "rot", "g_xyz", "g_rot", "g") + _ASSEMBLY_KEYS,
    "optim": tuple(f"{q}{i}" for q in "pg" for i in range(len(LAMB_SHAPES))),
    "volume": ("source0", "source1", "source2", "g"),
    "losses": ("color", "feature", "gt_rgb", "gt_embed"),
    "voxelizer": ("features",),
    "encoder": ("x", "residual", "g", "weight", "bias", "running_mean0", "running_var0"),
    "voxel": ("volume", "g"),
    "attention": ("x", "context", "g") + atc.PARAMS,
    "photometric": ("color", "target"),
}
NOT_ENROLLED = {
    "_C": "the rasterizer: a non-finite mean, scale or rotation makes the reference's own tile ranges undefined (float -> int of NaN), so "
          "there is no class to hold ours to; its colours and opacities wait for a truth that speaks about them",
    "_lib": "the ctypes table: no op",
    "_state": "the rasterizer's host pipeline (see _C)",
    "augmentation": "the draws and bounds decide acceptance and become voxel indices: discrete choices",
    "camera": "host-side calibration of a handful of matrices whose inverse the reference takes with torch.inverse, which raises on a "
              "non-finite matrix where ours returns one",
}


def _op_modules():
    out = set()
    folder = os.path.join(ROOT, "manigaussian_amd")
    for name in sorted(os.listdir(folder)):
        if name.endswith(".py"):
            with open(os.path.join(folder, name)) as f:
                if re.search(r"_ops\.call\(|lib\(\)\.mgs_|\bL\.mgs_", f.read()):
                    out.add(name[:-3])
    return out


def test_every_module_that_calls_the_library_is_enrolled_operand_by_operand_or_listed_with_a_reason():
    mods = _op_modules()
    assert not set(ENROLLED) & set(NOT_ENROLLED)
    assert mods == set(ENROLLED) | set(NOT_ENROLLED), sorted(mods ^ (set(ENROLLED) | set(NOT_ENROLLED)))
    assert all(len(r) > 20 for r in NOT_ENROLLED.values())
    tainted = {}
    for s in SUBJECTS.values():
        tainted.setdefault(s.module, set()).update(s.taints)
        assert all(len(p) >= 2 for p in s.taints.values()), (s.key, "two positions per operand")
    assert {m: set(o) for m, o in ENROLLED.items()} == tainted, "the table and the subjects name different operands"


# ---- the cases -------------------------------------------------------------------------------------------------------------------------------
PARAMS = [(s.key, operand, position) for s in SUBJECTS.values() for operand, positions in s.taints.items() for position in positions]
IDS = [f"{k}-{o}-{p}".replace(" ", "_") for k, o, p in PARAMS]
# ops without padding, interpolation or dropout: no free element at all
NO_FREE = ("mlp", "deform_apply", "deform_assembly", "gaussian_epilogue", "spatial_softmax", "fused_lamb", "layer_norm", "bias_geglu",
           "rendering_loss", "voxelizer", "batch_norm_act", "photometric_loss")


@pytest.mark.parametrize("key, operand, position", PARAMS, ids=IDS)
def test_the_reference_speaks_clearly(key, operand, position):
    """Admission, without a GPU: the reference's float32 and float64 runs agree on every class, and the free elements keep their cap."""
    s = SUBJECTS[key]
    assert (s.free_share == 0.0) == key.startswith(NO_FREE), key
    shown = 0
    for value in VALUES:
        try:
            adm = s.admit(operand, position, value)
        except nf.Refused as e:
            assert (operand, value) in s.may_refuse, e
            print("refused:", e)
            continue
        counts = {k: torch.bincount(c.reshape(-1).long(), minlength=4).tolist() for k, c in adm.want.items()}
        print(f"{adm.tag}: (finite, nan, +inf, -inf) {counts}, free or unclear {sum(int(f.sum()) for f in adm.free.values())}, "
              f"unclear {adm.unclear}" + (f", over the cap of free elements: {adm.over_cap}" if adm.over_cap else ""))
        shown += adm.nonfinite()
    assert shown, (key, operand, position, "no value of the taint reaches any result: the case shows nothing")


def test_what_may_be_refused_is_refused_somewhere():
    """A declaration that nothing backs would let a position go uncompared for no reason."""
    for s in SUBJECTS.values():
        for operand, value in s.may_refuse:
            hits = 0
            for position in s.taints[operand]:
                try:
                    s.admit(operand, position, value)
                except nf.Refused:
                    hits += 1
            print(s.key, operand, value, "refused at", hits, "of", len(s.taints[operand]), "positions")
            assert hits, (s.key, operand, value)


# ---- the restatements against the reference's own modules --------------------------------------------------------------------------------
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden", "nonfinite")
RESTATED = [k for k, s in SUBJECTS.items() if s.reference_module is not None]


def golden_path(key):
    return os.path.join(GOLDEN_DIR, key.replace(" ", "_") + ".npz")


def class_maps(s, run):
    """{"operand|position|value|result": uint8 classes} of run(tainted inputs, float64) over every taint of the subject."""
    out = {}
    for operand, positions in s.taints.items():
        for position in positions:
            for value in VALUES:
                r = run(nf._fresh(s.tainted(operand, position, value)), torch.float64)
                for name, t in r.items():
                    out[f"{operand}|{position}|{value}|{name}"] = nf.classes(t).numpy()
    return out


def load_golden(key):
    import numpy as np
    with np.load(golden_path(key)) as z:
        return {k: z[k] for k in z.files}


def _same_maps(got, want):
    assert sorted(got) == sorted(want)
    bad = [k for k in want if got[k].shape != want[k].shape or got[k].dtype != want[k].dtype or (got[k] != want[k]).any()]
    assert not bad, bad[:8]


@pytest.mark.parametrize("key", RESTATED)
def test_the_restatement_has_the_classes_the_reference_module_was_recorded_with(key):
    """tests/golden/nonfinite/<subject>.npz: what the reference's own module gave on every tainted input, as classes.  The
    restatement that serves as the truth on the GPU machine, where the reference is not, gives the same."""
    _same_maps(class_maps(SUBJECTS[key], SUBJECTS[key].ref), load_golden(key))


@pytest.mark.parametrize("key", RESTATED)
def test_the_fixtures_regenerate_from_the_reference_module(key):
    s = SUBJECTS[key]
    if not s.have_reference():
        pytest.skip("no copy of the reference on this machine")
    _same_maps(class_maps(s, s.reference_module), load_golden(key))


@gpu
@pytest.mark.parametrize("value", VALUES)
@pytest.mark.parametrize("key, operand, position", PARAMS, ids=IDS)
def test_one_tainted_element(key, operand, position, value):
    """Ours has the reference's class at every element that is not free, and lies within the op's own bound where that is finite."""
    s = SUBJECTS[key]
    try:
        adm = s.admit(operand, position, value)
    except nf.Refused as e:
        assert (operand, value) in s.may_refuse, e
        print("refused, nothing to compare with:", e)
        return
    nf.compare(s.ours(s.tainted(operand, position, value)), adm, s.ceiling, s.parts, s.bound_fn)
