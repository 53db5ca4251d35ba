"""The per-point ("embed path") kernels -- mgs_voxel.hip, mgs_regress.hip, mgs_deform.hip, mgs_mlp.hip -- and the hand-issued
forward and backward of deform._FusedResnetFC, through the public wrappers, against float64 truths and exact cases
(tests/embed_cases.py).

Toleranced comparisons follow tests/volume_cases.py's rule, per column group:
  |ours - truth| <= 16 x max(ref_err, 2^-23) x max|truth of the group|
with the truth the plain torch formulation in float64 on the CPU and ref_err the same formulation's float32 error.  What is a copy,
one float32 add, a select or a relu is compared with torch.equal.  The fused ResnetFC is pinned bit for bit on integer-valued
networks whose every float32 summation order is exact (row seams of the column sums, split-K weight gradients, every branch of
the backward), and by the rule on one real-valued case whose pre-activations keep clear of zero.

The measured rel_err and ref_err of every group go through util.report (profiles/embed_kernels_parity.jsonl is one GPU run).
"""
import copy
import ctypes
import math

import pytest
import torch

import embed_cases as ec
from numerics import dev
import util

gpu = pytest.mark.gpu


# ---- CPU: the truths, the cases' conditions ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [257, 4099])
def test_the_closed_forms_equal_float64_autograd_epilogue_and_apply(N):
    t = ec.epilogue_truth(N)
    out, g_raw = ec.epilogue_restated(t["raw"], t["cot"])
    for k, v in out.items():
        assert ec.rel_err(v, t["truth"][k]) <= 1e-12, k
    for g in t["groups"]:
        if g.key == "g_raw" and g.of(t["truth"]).numel():
            assert ec.rel_err(g.of({"g_raw": g_raw}), g.of(t["truth"])) <= 1e-12, g.name
    a = ec.apply_truth(N)
    restated = {"g_delta": torch.cat([a["cot"][0].double(), ec.apply_restated(a["delta"], a["rot"], a["cot"][1])], 1)}
    for g in a["groups"]:
        if g.key == "g_delta":
            assert ec.rel_err(g.of(restated), g.of(a["truth"])) <= 1e-12, g.name
    assert torch.equal(a["truth"]["g_delta"][:, :3], a["cot"][0].double())


@pytest.mark.parametrize("case", [c for c in ec.VOXEL_CASES if c[1] == 8 and c[3] == 257 and c[2] == 0])
def test_the_eight_corner_sum_equals_float64_grid_sample(case):
    grid, C, K, N = case
    t = ec.voxel_truth(case)
    leaf = t["vox"].double().clone().requires_grad_(True)
    out = ec.trilinear_restated(leaf, t["xyz"])
    (g,) = torch.autograd.grad(out, leaf, t["cot"][:, :C].double())
    assert ec.rel_err(out.detach(), t["truth"]["latent"][:, :C]) <= 1e-12
    assert ec.rel_err(g.reshape(C, -1).t(), t["truth"]["g_voxel"]) <= 1e-12


@pytest.mark.parametrize("N", [n for n in ec.POINT_N if n])
def test_per_point_cases_keep_their_conditions(N):
    t, a = ec.epilogue_truth(N), ec.apply_truth(N)
    ec.epilogue_conditions(t["raw"])
    ec.apply_conditions(a["delta"], a["rot"])
    assert max(t["ref_err"].values()) <= ec.REF_ERR_CEILING and max(a["ref_err"].values()) <= ec.REF_ERR_CEILING
    raw = t["raw"]
    if N >= ec.EDGE_ROWS_FROM:
        assert raw[0, 7:11].abs().sum() == 0 and raw[1, 14:17].abs().sum() == 0
        assert (raw[2, 4:7].double() - ec.LOG_SCALE_MAX - 1e-3).abs().max() < 1e-6
        assert (raw[3, 4:7].double() - ec.LOG_SCALE_MAX + 1e-3).abs().max() < 1e-6
        assert raw[4:8, 3].tolist() == list(ec.SATURATED_LOGITS)
        # the sigmoid is saturated: the gradient is 0 (in float32 exactly so at +30 and +-100; at -30 it is 9.4e-14 g)
        assert (t["truth"]["g_raw"][4:8, 3].abs() < 1e-12).all() and (t["ref32"]["g_raw"][[4, 6, 7], 3] == 0).all()
        assert ((a["rot"] + a["delta"][:, 3:])[0] == 0).all()
        # the zero rows' expected values: the outputs are 0, the gradients the cotangent over the guard
        assert (t["truth"]["rot"][0] == 0).all() and (t["truth"]["feature_normalized"][1] == 0).all()
        assert ec.rel_err(t["truth"]["g_raw"][0, 7:11], t["cot"]["rot"][0].double() * 1e12) <= 1e-12
        assert ec.rel_err(t["truth"]["g_raw"][1, 14:17], t["cot"]["feature_normalized"][1].double() * 1e12
                          + t["cot"]["feature"][1].double()) <= 1e-12
        assert ec.rel_err(a["truth"]["g_delta"][0, 3:], a["cot"][1][0].double() * 1e12) <= 1e-12
    above = raw[:, 4:7] > ec.LOG_SCALE_MAX
    assert N < 16 or (above.any() and not above.all()), "log-scales on both sides of the clamp"


@pytest.mark.parametrize("case", ec.VOXEL_CASES + [ec.VOXEL_LARGE], ids=str)
def test_voxel_cases_keep_their_conditions(case):
    grid, C, K, N = case
    t = ec.voxel_truth(case)
    assert not ec.voxel_conditions(t["xyz"], grid).any()
    assert max(t["ref_err"].values()) <= ec.REF_ERR_CEILING, t["ref_err"]
    assert t["truth"]["latent"].shape == (N, C + 3 + 6 * K)
    if N >= ec.EDGE_ROWS_FROM:
        assert (t["canon32"][0] == 0).all() and (t["canon32"][1] - 1).abs().max() <= 2.0 ** -23
        assert (t["truth"]["latent"][ec.FAR_ROW, :C] == 0).all() and (t["canon32"][ec.FAR_ROW] > 1e5).all()
        c = t["canon32"][ec.SPECIAL_ROWS:]
        assert c.min() < -0.1 and c.max() > 1.1 and c.min() >= -0.151 and c.max() <= 1.151, "up to 15 % outside the box"
    if case == ec.VOXEL_LARGE:
        assert N * (C + 3 + 6 * K) > ec.VOXEL_GRID_LIMIT and N * C > ec.VOXEL_GRID_LIMIT, "both grid-stride loops take a second trip"
    else:
        assert N * (C + 3 + 6 * K) <= ec.VOXEL_GRID_LIMIT


def test_positional_constants_are_the_modules_float32_ones():
    freqs, phases = ec.pe_constants(6)
    f32 = torch.tensor(math.pi, dtype=torch.float32)
    assert torch.equal(freqs[0::2], f32 * 2.0 ** torch.arange(6)) and torch.equal(freqs[1::2], freqs[0::2])
    assert torch.equal(phases[1::2], torch.full((6,), math.pi / 2, dtype=torch.float32)) and (phases[0::2] == 0).all()


@pytest.mark.parametrize("hidden", ec.MLP_HIDDEN)
def test_column_sum_yardsticks_stay_under_the_ceiling(hidden):
    for M in ec.MLP_M:
        d = ec.mlp_inputs(M, hidden)
        assert M * hidden < 7 or ((d["act"] == 0).any() and (d["g_pre"][d["act"] == 0] != 0).any()), "exact zeros carry a gradient to drop"
        for with_res in (False, True):
            truth, ref_err = ec.colsum_truth(M, hidden, with_res)
            assert truth.shape == (hidden,) and ref_err <= ec.REF_ERR_CEILING


@pytest.mark.parametrize("case", ec.INT_CASES, ids=str)
def test_integer_networks_stay_below_2_to_24_and_the_plain_path_is_exact(case):
    M, hidden, n_blocks, combine_layer = case
    assert ec.integer_abs_bound(case) < ec.INT_LIMIT
    m, zx, wd, wx = ec.integer_network(case)
    for p in m.parameters():
        assert torch.equal(p, p.round()) and (p.dim() == 1 or ((p != 0).sum(1) == 2).all()) and p.abs().max() <= 1
    assert len(m.lin_z) == min(combine_layer, n_blocks)
    with torch.no_grad():
        pre = ec.preactivations(m, zx)
    assert M * hidden < 64 or sum(int((p == 0).sum()) for p in pre) >= 3, "exactly-zero pre-activations: relu'(0) = 0 is exercised"
    both = ec.integer_truth(case, "both")
    for mode in ec.INT_MODES:
        truth = ec.integer_truth(case, mode)
        got = ec.run_network(m, zx, wd, wx, mode)
        assert set(got) == set(truth)
        for k, v in truth.items():
            assert ec.same_values(got[k], v), (mode, k)
            assert v is None or torch.equal(v, v.round()), (mode, k)
        if mode in ("frozen", "input_is_data"):
            frozen = [k for k, v in truth.items() if v is None]
            assert len(frozen) == (4 if mode == "frozen" else 0) and ("grad zx" in truth) == (mode == "frozen")
            assert all(torch.equal(v, both[k]) for k, v in truth.items() if v is not None), "the other gradients are unchanged"


def test_real_valued_cases_keep_clear_of_every_relu():
    m, zx, wd, wx, seed = ec.real_network()
    assert zx.shape == (ec.REAL_M, 198) and m.d_hidden == ec.REAL_HIDDEN
    with torch.no_grad():
        pre = ec.preactivations(copy.deepcopy(m).double(), zx.double())
    assert len(pre) == 11 and min(float(p.abs().min()) for p in pre) >= ec.PREACT_MARGIN
    truth, errs = ec.real_truth()
    assert max(errs.values()) <= ec.REF_ERR_CEILING
    for variant in ec.FIELD_VARIANTS:
        f = ec.field_case(variant)
        zin = ec.assembly_exact(f["inputs"])
        with torch.no_grad():
            pre = ec.preactivations(copy.deepcopy(f["field"].mlp).double(), zin.double())
        assert min(float(p.abs().min()) for p in pre) >= ec.PREACT_MARGIN and max(f["ref_err"].values()) <= ec.REF_ERR_CEILING


def test_the_library_refuses_bad_arguments_before_any_launch():
    """With fake pointers: a call that got as far as a launch would not come back with MGS_ERR_INVALID_ARG."""
    from manigaussian_amd import _lib
    L = _lib.lib()
    p, INV, OK = 0x10000, _lib.MGS_ERR_INVALID_ARG, _lib.MGS_OK
    b = (ctypes.c_float * 6)(*ec.BOUNDS)

    def refused(rc, word):
        assert rc == INV and word in _lib.last_error(), (rc, word, _lib.last_error())

    def vf(N=5, C=4, K=6, vox=p, xyz=p, out=p, bounds=b):
        return L.mgs_voxel_sample_pe_forward(N, C, 2, 3, 4, K, 3.14, bounds, vox, xyz, out, None)

    def vb(N=5, C=4, stride=4, xyz=p, g=p, gv=p):
        return L.mgs_voxel_sample_backward(N, C, 2, 3, 4, b, xyz, g, stride, gv, None)

    for rc in (vf(N=-1), vf(K=17), vf(K=-1), vf(C=0), vf(bounds=None), vf(vox=None), vf(xyz=None), vf(out=None),
               vb(N=-1), vb(stride=3), vb(xyz=None), vb(g=None), vb(gv=None)):
        refused(rc, "voxel_sample")
    assert vf(K=16, N=0, vox=None, xyz=None, out=None) == OK and vb(N=0, xyz=None, g=None, gv=None) == OK
    assert vf(N=0, K=17) == INV

    def ef(N=5, ptrs=(p,) * 9):
        return L.mgs_regress_epilogue_forward(N, *ptrs, None)

    def eb(N=5, raw=p, g_raw=p):
        return L.mgs_regress_epilogue_backward(N, raw, *(None,) * 7, g_raw, None)   # every cotangent may be absent

    for rc in [ef(N=-1), eb(N=-1), eb(raw=None), eb(g_raw=None)] + [ef(ptrs=(p,) * k + (None,) + (p,) * (8 - k)) for k in range(9)]:
        refused(rc, "regress_epilogue")
    assert ef(N=0, ptrs=(None,) * 9) == OK and eb(N=0, raw=None, g_raw=None) == OK

    def af(N=5, DL=4, DZ=3, DA=2, ptrs=(p,) * 10):
        return L.mgs_deform_assemble_forward(N, DL, DZ, DA, *ptrs, None)

    def ab(N=5, DL=4, DZ=3, DA=2, ptrs=(p,) * 3):
        return L.mgs_deform_assemble_backward(N, DL, DZ, DA, 1, *ptrs, None)

    required = [0, 1, 2, 3, 4, 5, 7, 8, 9]   # the feature pointer (6) is optional
    for rc in [af(N=-1), af(DL=-1), af(DZ=-1), af(DA=-1), ab(N=-1), ab(DL=-1), ab(DZ=-1), ab(DA=-1)] + \
              [af(ptrs=tuple(None if k == j else p for k in range(10))) for j in required] + \
              [ab(ptrs=tuple(None if k == j else p for k in range(3))) for j in range(3)]:
        refused(rc, "deform_assemble")
    assert af(N=0, ptrs=(None,) * 10) == OK and ab(N=0, ptrs=(None,) * 3) == OK

    def pf(N=5, ptrs=(p,) * 5):
        return L.mgs_deform_apply_forward(N, *ptrs, None)

    def pb(N=5, ptrs=(p,) * 5):
        return L.mgs_deform_apply_backward(N, *ptrs, None)

    for call in (pf, pb):
        refused(call(N=-1), "deform_apply")
        for j in range(5):
            refused(call(ptrs=tuple(None if k == j else p for k in range(5))), "deform_apply")
        assert call(N=0, ptrs=(None,) * 5) == OK

    def rb(M=5, N=64, x=p, bias=p, a=p, xb=p):
        return L.mgs_mlp_relu_bias(M, N, x, bias, a, xb, None)

    def rw(M=5, N=64, g_pre=p, act=p, g_res=p, g_out=p, cs=p):
        return L.mgs_mlp_relu_backward(M, N, g_pre, act, g_res, g_out, cs, None)

    for rc in (rb(M=-1), rb(N=0), rb(N=6), rb(N=12), rb(N=2048), rb(x=None), rb(a=None, xb=None)):
        refused(rc, "mlp_relu_bias")
    for rc in (rw(M=-1), rw(N=0), rw(N=6), rw(N=12), rw(N=2048), rw(g_pre=None), rw(act=None), rw(g_out=None)):
        refused(rc, "mlp_relu_backward")
    assert rb(M=0, x=None, bias=None, a=None, xb=None) == OK and rw(M=0, g_pre=None, act=None, g_res=None, g_out=None, cs=None) == OK
    assert rb(M=0, N=6) == INV and rw(M=0, N=12) == INV


# ---- GPU --------------------------------------------------------------------------------------------------------------------------
def check_groups(tag, groups, got, truth, ref_err):
    """Every group of got within the rule's bound of truth; each figure is printed and reported before anything is asserted."""
    failed = []
    for g in groups:
        t = g.of(truth)
        if not t.numel():
            continue
        err, ref = ec.rel_err(g.of(got).detach().cpu(), t), ref_err[g.name]
        allowed = ec.bound(ref)
        print(f"{tag} {g.name}: rel_err {err:.3e}, ref_err {ref:.3e}, bound {allowed:.3e}")
        util.report(f"{tag} {g.name}", rel_err=err, ref_err=ref, bound=allowed)
        if not err <= allowed:
            failed.append((g.name, err, allowed))
    assert not failed, (tag, failed)


def check_tensors(tag, got, truth, ref_err):
    """The same for a dict of whole tensors: one group per tensor."""
    check_groups(tag, [ec.Group(k, k) for k in truth], got, truth, ref_err)


def epilogue_run(raw, xyz_in, cot, outputs=ec.EPILOGUE_OUTPUTS):
    from manigaussian_amd.regressor import gaussian_epilogue
    raw, xyz_in = raw.detach().requires_grad_(True), xyz_in.detach().requires_grad_(True)
    out = gaussian_epilogue(raw, xyz_in)
    loss = sum((out[k] * cot[k].to(device=raw.device, dtype=out[k].dtype).reshape(out[k].shape)).sum() for k in outputs)
    g_raw, g_xyz = torch.autograd.grad(loss, [raw, xyz_in], allow_unused=True)
    return dict({k: v.detach() for k, v in out.items()}, g_raw=g_raw, g_xyz_in=g_xyz)


def same_results(a, b):
    return all((a[k] is None and b[k] is None) or torch.equal(a[k].reshape(b[k].shape).float(), b[k]) for k in b)


@gpu
@pytest.mark.parametrize("N", ec.POINT_N)
def test_epilogue_forward_and_backward(N):
    if N == 0:
        got = epilogue_run(torch.zeros(0, 26, device=dev()), torch.zeros(0, 3, device=dev()),
                           {k: torch.zeros(0) for k in ec.EPILOGUE_OUTPUTS})
        assert got["g_raw"].shape == (0, 26) and got["g_xyz_in"].shape == (0, 3) and got["sh"].shape == (0, 4, 3)
        assert got["opacity"].shape == (0, 1) and got["rot"].shape == (0, 4) and got["feature_normalized"].shape == (0, 3)
        return
    t = ec.epilogue_truth(N)
    got = epilogue_run(t["raw"].to(dev()), t["xyz_in"].to(dev()), t["cot"])
    ref = t["ref32"]
    for k in ("xyz", "sh", "feature"):
        assert got[k].shape == ref[k].shape and torch.equal(got[k].cpu(), ref[k]), (k, "one correct float32 result")
    for name in ("xyz", "f_dc", "f_rest"):
        assert torch.equal(got["g_raw"][:, ec.RAW_GROUPS[name]].cpu(), ref["g_raw"][:, ec.RAW_GROUPS[name]]), name
    assert torch.equal(got["g_xyz_in"].cpu(), t["cot"]["xyz"])
    if N >= ec.EDGE_ROWS_FROM:
        assert (got["scale"][2].cpu() == torch.tensor(0.05)).all() and (got["g_raw"][2, 4:7] == 0).all(), "1e-3 above the clamp"
        assert (got["scale"][3] < 0.05).all() and (got["g_raw"][3, 4:7] != 0).all(), "1e-3 below the clamp"
        assert (got["g_raw"][[4, 6, 7], 3] == 0).all() and got["g_raw"][5, 3].abs() < 1e-12, "saturated sigmoid"
        assert (got["rot"][0] == 0).all() and (got["feature_normalized"][1] == 0).all()
    check_groups(f"epilogue N={N}", t["groups"], got, t["truth"], t["ref_err"])


@gpu
def test_epilogue_layouts_types_and_single_outputs():
    N = 255
    t = ec.epilogue_truth(N)
    raw, xyz_in, cot = t["raw"].to(dev()), t["xyz_in"].to(dev()), t["cot"]
    base = epilogue_run(raw, xyz_in, cot)
    for lead in ((1, N), (3, N // 3)):
        got = epilogue_run(raw.reshape(*lead, 26), xyz_in.reshape(*lead, 3), cot)
        assert got["sh"].shape == (*lead, 4, 3) and got["opacity"].shape == (*lead, 1) and got["g_raw"].shape == (*lead, 26)
        assert same_results(got, base), lead
    got = epilogue_run(raw.double(), xyz_in.double(), cot)
    assert got["g_raw"].dtype == torch.float64 and got["rot"].dtype == torch.float32 and same_results(got, base), "a float64 input"
    wide, wide3 = torch.full((N, 40), float("nan"), device=dev()), torch.full((N, 5), float("nan"), device=dev())
    wide[:, 7:33], wide3[:, 1:4] = raw, xyz_in
    assert not wide[:, 7:33].is_contiguous()
    assert same_results(epilogue_run(wide[:, 7:33], wide3[:, 1:4], cot), base), "a slice of a wider tensor"
    # one output used alone: the others arrive as None, and their columns are exactly 0
    own = dict(xyz=["xyz"], opacity=["opacity"], scale=["scale"], rot=["rot"], sh=["f_dc", "f_rest"], feature=["feature"],
               feature_normalized=["feature"])
    for k in ec.EPILOGUE_OUTPUTS:
        got = epilogue_run(raw, xyz_in, cot, outputs=[k])
        mine = torch.zeros(26, dtype=torch.bool)
        for name in own[k]:
            mine[ec.RAW_GROUPS[name]] = True
        g = got["g_raw"].cpu()
        assert (g[:, ~mine] == 0).all() and (g[:, mine] != 0).any(), k
        assert (got["g_xyz_in"] is None) == (k != "xyz")
        if k == "feature":
            assert torch.equal(g[:, mine], cot["feature"])
        elif k == "feature_normalized":
            truth = {"g_raw": t["truth"]["g_raw"].clone()}
            truth["g_raw"][:, 14:17] -= cot["feature"].double()
            groups = [x for x in t["groups"] if x.name.startswith("g_raw.feature")]
            check_groups("epilogue feature_normalized alone", groups, {"g_raw": g}, truth, t["ref_err"])
        else:
            assert torch.equal(g[:, mine], base["g_raw"].cpu()[:, mine]), k


def apply_run(delta, xyz, rot, cot):
    from manigaussian_amd.deform import deform_apply
    delta = delta.detach().requires_grad_(True)
    nx, nr = deform_apply(delta, xyz, rot)
    (g,) = torch.autograd.grad((nx * cot[0].to(nx.device)).sum() + (nr * cot[1].to(nx.device)).sum(), delta)
    return dict(xyz=nx.detach(), rot=nr.detach(), g_delta=g)


@gpu
@pytest.mark.parametrize("N", ec.POINT_N)
def test_deform_apply_forward_and_backward(N):
    if N == 0:
        got = apply_run(torch.zeros(0, 7, device=dev()), torch.zeros(0, 3, device=dev()), torch.zeros(0, 4, device=dev()),
                        [torch.zeros(0, 3), torch.zeros(0, 4)])
        assert got["xyz"].shape == (0, 3) and got["rot"].shape == (0, 4) and got["g_delta"].shape == (0, 7)
        return
    t = ec.apply_truth(N)
    delta, xyz, rot = (t[k].to(dev()) for k in ("delta", "xyz", "rot"))
    got = apply_run(delta, xyz, rot, t["cot"])
    assert torch.equal(got["xyz"].cpu(), t["ref32"]["xyz"]), "xyz + delta: one float32 add"
    assert torch.equal(got["g_delta"][:, :3].cpu(), t["cot"][0])
    if N >= ec.EDGE_ROWS_FROM:
        assert (got["rot"][0] == 0).all(), "rot + delta == 0"
    check_groups(f"deform_apply N={N}", t["groups"], got, t["truth"], t["ref_err"])
    if N == 257:  # a float64 delta, slices of wider tensors
        wide = torch.full((N, 9), float("nan"), device=dev())
        wide[:, 2:6] = rot
        other = apply_run(delta.double(), xyz.double(), wide[:, 2:6], t["cot"])
        assert other["g_delta"].dtype == torch.float64 and same_results(other, got)


@gpu
@pytest.mark.parametrize("N", ec.POINT_N)
def test_input_assembly_is_a_copy_both_ways(N):
    from manigaussian_amd.deform import assemble_deform_input
    for DL, DZ, DA, has_feat in ((128, 39, 8, False), (128, 39, 8, True), (128, 39, 0, False), (16, 5, 0, True), (0, 1, 8, True)):
        d = ec.assembly_inputs(N, DL, DZ, DA, has_feat)
        want = ec.assembly_exact(d)
        c = {k: (None if v is None else v.to(dev())) for k, v in d.items()}
        lat, z = c["point_latent"].requires_grad_(True), c["z_feature"].requires_grad_(True)
        args = [c[k] for k in ("xyz", "sh", "rot", "scale", "opacity", "feature", "action")]
        out = assemble_deform_input(lat, z, *args)
        assert out.shape == want.shape == (N, DL + 23 + 3 * has_feat + DZ + DA) and torch.equal(out.cpu(), want), (DL, DZ, DA, has_feat)
        w = torch.randn(want.shape, generator=torch.Generator().manual_seed(N + DL))
        g_lat, g_z = torch.autograd.grad(out, [lat, z], w.to(dev()))
        o_z = DL + 23 + 3 * has_feat
        assert torch.equal(g_lat.cpu(), w[:, :DL]) and torch.equal(g_z.cpu(), w[:, o_z:o_z + DZ]), (DL, DZ, DA, has_feat)
        if N == 257 and DL == 128 and has_feat:  # a float64 input and slices of wider tensors
            wide = torch.full((N, DL + 7), float("nan"), device=dev())
            wide[:, 3:3 + DL] = lat.detach()
            wz = z.detach().double().requires_grad_(True)
            wl = wide[:, 3:3 + DL].requires_grad_(True)
            sh_wide = torch.full((N, 4, 5), float("nan"), device=dev())
            sh_wide[:, :, 1:4] = c["sh"]
            args[1] = sh_wide[:, :, 1:4]
            other = assemble_deform_input(wl, wz, *args)
            assert torch.equal(other, out)
            a, b = torch.autograd.grad(other, [wl, wz], w.to(dev()))
            assert torch.equal(a, g_lat) and b.dtype == torch.float64 and torch.equal(b.float(), g_z)


def voxel_run(vox, xyz, cot, K):
    from manigaussian_amd.voxel import point_latent_pe
    vox = vox.detach().requires_grad_(True)
    out = point_latent_pe(vox, xyz, ec.BOUNDS, num_freqs=K)
    (g,) = torch.autograd.grad(out, vox, cot)
    return out.detach(), g


@gpu
@pytest.mark.parametrize("case", ec.VOXEL_CASES + [ec.VOXEL_LARGE], ids=str)
def test_point_latent_forward_and_backward(case):
    """The backward is the wrapper's own call: the cotangent's row stride C + 3 + 6 K is wider than C."""
    grid, C, K, N = case
    t = ec.voxel_truth(case)
    vox, xyz, cot = t["vox"].to(dev()), t["xyz"].to(dev()), t["cot"].to(dev())
    out, g = voxel_run(vox, xyz, cot, K)
    assert out.shape == (N, C + 3 + 6 * K) and g.shape == vox.shape
    assert torch.equal(out[:, C:C + 3].cpu(), t["canon32"]), "the canonical coordinate: the same float32 expression"
    if N >= ec.EDGE_ROWS_FROM:
        assert (out[ec.FAR_ROW, :C] == 0).all(), "far outside the box: exactly 0"
        only_far = torch.zeros_like(cot)
        only_far[ec.FAR_ROW] = cot[ec.FAR_ROW]
        assert (voxel_run(vox, xyz, only_far, K)[1] == 0).all(), "... and it contributes exactly nothing to the gradient"
    assert (voxel_run(vox, xyz, torch.zeros_like(cot), K)[1] == 0).all(), "an all-zero cotangent"
    got = dict(latent=out, g_voxel=g.reshape(C, -1).t())
    check_groups(f"point_latent grid={grid} C={C} K={K} N={N}", t["groups"], got, t["truth"], t["ref_err"])


@gpu
@pytest.mark.parametrize("hidden", ec.MLP_HIDDEN)
@pytest.mark.parametrize("M", ec.MLP_M)
def test_mlp_elementwise_passes(M, hidden):
    from manigaussian_amd import _lib, _ops, deform
    d = ec.mlp_inputs(M, hidden)
    c = {k: v.to(dev()) for k, v in d.items()}
    a, xb = deform._relu_bias(c["act"], c["bias"])
    assert torch.equal(a.cpu(), torch.relu(d["act"])) and torch.equal(xb.cpu(), d["act"] + d["bias"])
    a, xb = deform._relu_bias(c["act"], None)
    assert torch.equal(a.cpu(), torch.relu(d["act"])) and torch.equal(xb, c["act"])
    a, xb = deform._relu_bias(c["act"], None, want_xb=False)
    assert xb is None and torch.equal(a.cpu(), torch.relu(d["act"]))
    a, xb = deform._relu_bias(c["act"], c["bias"], want_relu=False)
    assert a is None and torch.equal(xb.cpu(), d["act"] + d["bias"])
    for with_res in (False, True):
        want = ec.relu_backward_exact(d, with_res)
        res = c["g_res"] if with_res else None
        for with_cs in (True, False):
            g_pre = c["g_pre"].clone()
            cs = torch.zeros(hidden, device=dev()) if with_cs else None
            out = deform._relu_backward(g_pre, c["act"], res, cs)
            assert out is g_pre and torch.equal(out.cpu(), want), ("in place", with_res, with_cs)
            if with_cs:
                truth, ref_err = ec.colsum_truth(M, hidden, with_res)
                check_groups(f"mlp colsum M={M} hidden={hidden} g_res={with_res}", [ec.Group("colsum", "colsum")],
                             {"colsum": cs.reshape(-1, 1)}, {"colsum": truth.reshape(-1, 1)}, {"colsum": ref_err})
        # ... and into a tensor of its own, the residual's buffer as the output
        out, cs = torch.full_like(c["g_pre"], float("nan")), torch.zeros(hidden, device=dev())
        _lib.check(_lib.lib().mgs_mlp_relu_backward(M, hidden, c["g_pre"].data_ptr(), c["act"].data_ptr(),
                                                    res.data_ptr() if with_res else None, out.data_ptr(), cs.data_ptr(),
                                                    _ops.stream(dev())), "mgs_mlp_relu_backward")
        assert torch.equal(out.cpu(), want) and torch.equal(c["g_pre"].cpu(), d["g_pre"])


def _count_calls(monkeypatch, deform):
    calls = []
    real = deform._relu_backward
    monkeypatch.setattr(deform, "_relu_backward", lambda *a: (calls.append(1), real(*a))[1])
    return calls


@gpu
@pytest.mark.parametrize("case", ec.INT_CASES, ids=str)
def test_plain_path_on_the_device_is_exact_on_integers(case):
    """The control: the module's plain torch path (library GEMMs, autograd) meets the equality the fused path is held to."""
    m, zx, wd, wx = ec.integer_network(case)
    for mode in ("both", "features"):
        truth = ec.integer_truth(case, mode)
        got = ec.run_network(m, zx.to(dev()), wd.to(dev()), wx.to(dev()), mode, fused=False)
        wrong = [k for k in truth if not ec.same_values(got[k], truth[k])]
        assert not wrong, (mode, wrong)


@gpu
@pytest.mark.parametrize("case", ec.INT_CASES, ids=str)
def test_fused_resnetfc_is_exact_on_integers(case, monkeypatch):
    """delta, x, grad zx and every parameter gradient, bit for bit, in every gradient mode; M = 136 and 1032 take the split-K
    weight gradient (8 batches of 17 and 129 rows)."""
    from manigaussian_amd import deform
    monkeypatch.setattr(deform, "_WGRAD_MIN_ROWS", 16)
    calls = _count_calls(monkeypatch, deform)
    M = case[0]
    assert (M % deform._WGRAD_SPLIT == 0 and M >= 16 * deform._WGRAD_SPLIT) == (M in (136, 1032))
    m, zx, wd, wx = ec.integer_network(case)
    wrong = []
    for mode in ec.INT_MODES:
        truth = ec.integer_truth(case, mode)
        before = len(calls)
        got = ec.run_network(m, zx.to(dev()), wd.to(dev()), wx.to(dev()), mode, fused=True)
        assert len(calls) > before, "the fused path ran"
        assert set(got) == set(truth)
        wrong += [(mode, k) for k in truth if not ec.same_values(got[k], truth[k])]
        grads = [v for k, v in got.items() if k.startswith("grad") and v is not None and v.numel()]
        assert len({v.data_ptr() for v in grads}) == len(grads), (mode, "two gradients share their memory")
    assert not wrong, wrong


@gpu
def test_fused_resnetfc_real_valued_against_float64():
    """M = 1000, hidden 64, no pre-activation within 1e-5 of zero: the rule holds for every element, no quantile allowance."""
    m, zx, wd, wx, seed = ec.real_network()
    truth, ref_err = ec.real_truth()
    got = ec.run_network(m, zx.to(dev()), wd.to(dev()), wx.to(dev()), "both", fused=True)
    check_tensors(f"fused resnetfc M={ec.REAL_M} hidden={ec.REAL_HIDDEN} seed={seed}", got, truth, ref_err)


@gpu
@pytest.mark.parametrize("variant", list(ec.FIELD_VARIANTS))
def test_deformation_field_end_to_end_against_float64(variant, monkeypatch):
    from manigaussian_amd import deform
    calls = _count_calls(monkeypatch, deform)
    f = ec.field_case(variant)
    field = copy.deepcopy(f["field"]).to(dev())
    c = {k: (None if v is None else v.to(dev())) for k, v in f["inputs"].items()}
    lat, z = c["point_latent"].requires_grad_(True), c["z_feature"].requires_grad_(True)
    nxt = field(lat, z, c["xyz"], c["sh"], c["rot"], c["scale"], c["opacity"], feature=c["feature"], action=c["action"])
    names = [n for n, _ in field.mlp.named_parameters()]
    loss = (nxt["xyz"] * f["cot"][0].to(dev())).sum() + (nxt["rot"] * f["cot"][1].to(dev())).sum()
    grads = torch.autograd.grad(loss, [lat, z] + list(field.mlp.parameters()))
    assert calls, "the fused path ran"
    got = dict({"xyz": nxt["xyz"].detach(), "rot": nxt["rot"].detach(), "grad point_latent": grads[0], "grad z_feature": grads[1]},
               **{"grad " + n: g for n, g in zip(names, grads[2:])})
    check_tensors(f"deformation field {variant} N={ec.FIELD_N}", got, f["truth"], f["ref_err"])
