"""The fused BatchNorm3d + LeakyReLU (+ skip add) of the voxel encoder stem (manigaussian_amd/encoder.py, csrc/mgs_abn.hip) against
ManiGaussian's own InPlaceABN (helpers/network_utils.py:219-231) and MultiLayer3DEncoderShallow (:248-306).

The yardstick is the reference's own fp32 rounding error: a fixture (tests/golden/abn/, tests/abn_cases.py) holds the reference's
float64 results -- the truth -- and how far the reference's float32 run lies from each.  For y, dx, dweight, dbias and the two
running buffers:   |ours - truth| <= max(16 x ref_err, 16 x 2^-23) x max|truth|.
Elements whose float64 activation argument lies within 1e-5 of 0 may take either branch in any float32 run: they are left out of
the dx comparison (and of nothing else); no fixture has one outside `dead_channel`, the full-size cases may have 1e-4 of theirs.
On the GPU machine the reference does not exist: the full-size tests take the same formula in plain torch ops
(abn_cases.restatement, pinned against the fixtures here) in float64 as the truth and in float32 as the yardstick.
"""
import os

import numpy as np
import pytest
import torch

import abn_cases as ac
from child import run_graph_tool
from manigaussian_amd import _lib
from manigaussian_amd import encoder as enc
from numerics import dev

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL = {"site0": ((1, 8, 100, 100, 100), True),      # the stem's largest site, with its skip tensor
        "long_odd": ((2, 3, 51, 49, 53), True)}      # long, odd, misaligned, batched
KINK_SHARE = 1e-4


@pytest.fixture
def route():
    """Sets encoder.FORCE for one test and puts it back."""
    saved = enc.FORCE

    def force(value):
        enc.FORCE = value
    yield force
    enc.FORCE = saved


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not ac.have_reference(), reason="no copy of the reference on this machine")
def test_fixtures_match_the_reference():
    """The generator's computation, re-run.  Inputs and integers bit for bit; the float64 truths to 1e-12 of their magnitude (the
    order of a CPU's sums may follow its thread count); the yardsticks, maxima of float32 rounding errors, within a factor of 2."""
    for case in ac.CASES:
        f, now = ac.load_fixture(case), ac.reference_case(case)
        for q, e in zip(ac.QUANTITIES, now["ref_err"].tolist()):
            c = f["ref_err"][q]
            assert (e == 0 and c == 0) or 0.5 * c <= e <= 2 * c, (case, q, e, c)
            assert e <= ac.REF_ERR_CEILING, (case, q, e)
        for k, v in now.items():
            if k == "ref_err":
                continue
            if v.dtype == np.float64:
                t = torch.from_numpy(v)
                assert (t - f[k]).abs().max().item() <= 1e-12 * max(t.abs().max().item(), 1e-300), (case, k)
            else:
                assert np.array_equal(v, f[k].numpy()), (case, k)
        assert set(now) == set(f), case
    names = list(ac.load_reference().MultiLayer3DEncoderShallow().state_dict())
    assert names == ac.stem_state_dict_names()


def test_fixtures_are_small_and_have_no_element_near_the_kink():
    for case in ac.CASES:
        assert os.path.getsize(ac.fixture_path(case)) <= 1_000_000, case
        with np.load(ac.fixture_path(case), allow_pickle=False) as z:
            assert all(z[k].dtype.kind in "fi" for k in z.files), case
            assert float(z["ref_err"].max()) <= ac.REF_ERR_CEILING, case
            assert tuple(z["x"].shape) == ac.CASES[case]["shape"], case
            assert ("residual" in z.files) == ac.CASES[case].get("residual", True), case
        f = ac.load_fixture(case)
        assert all(ac.same_bits(v, f[k]) for k, v in ac.make_inputs(case, int(f["seed"][0])).items()), case
    f = ac.load_fixture("offset")
    assert abs(f["x"].mean().item() - 37.5) < 0.01 and abs(f["x"].std().item() - 0.05) < 0.005
    assert len(ac.stem_state_dict_names()) == 62


def _restated(f, case, dtype, device="cpu"):
    """The restatement on a fixture's inputs: {quantity: tensor} and z."""
    t = {k: f[k].to(device) for k in ("x", "g", "weight", "bias")}
    x, w, b = (t[k].detach().to(dtype).requires_grad_(True) for k in ("x", "weight", "bias"))
    res = f["residual"].to(device) if "residual" in f else None
    running = (f["running_mean0"].to(device), f["running_var0"].to(device)) if "running_mean0" in f else None
    y, z, mean, unbiased = ac.restatement(x, w, b, res, ac.slope_of(case), dtype, running)
    out = {"y": y.detach()}
    if running is None:
        (y * t["g"].to(dtype)).sum().backward()
        rm, rv = ac.running_after_one_step(mean.detach(), unbiased.detach())
        out.update(dx=x.grad, dweight=w.grad, dbias=b.grad, running_mean=rm, running_var=rv)
    return out, z.detach()


def test_the_float64_restatement_reproduces_every_fixture():
    """Pins restatement(), the GPU tests' stand-in for the reference, including its rule at z == 0 (dead_channel's dbias)."""
    for case in ac.CASES:
        f = ac.load_fixture(case)
        got, z = _restated(f, case, torch.float64)
        for q, v in got.items():
            want = f[q + "64"]
            assert (v - want).abs().max().item() <= 1e-12 * want.abs().max().item(), (case, q)
        near = ac.near_kink(z)
        if case == "dead_channel":
            dead = ac.CASES[case]["dead"]
            assert bool((z[:, dead] == 0).all()) and not bool(near[:, [c for c in range(z.size(1)) if c != dead]].any())
            slope_sum = 0.01 * f["g"][:, dead].double().sum().item()
            assert abs(f["dbias64"][dead].item() - slope_sum) <= 1e-12 * abs(slope_sum), "z == 0 takes the slope"
        else:
            assert not bool(near.any()), case


def _fwd(L, fake, **kw):
    a = dict(B=2, C=3, N=315, x=fake, res=fake, w=fake, b=fake, rm=fake, rv=fake, nbt=fake, training=1, momentum=0.1, eps=1e-5,
             slope=0.01, y=fake, stats=fake, ws=fake, ws_bytes=L.mgs_abn_workspace_bytes(2, 3, 315), slices=0)
    a.update(kw)
    return L.mgs_abn_forward(a["B"], a["C"], a["N"], a["x"], a["res"], a["w"], a["b"], a["rm"], a["rv"], a["nbt"], a["training"],
                             a["momentum"], a["eps"], a["slope"], a["y"], a["stats"], a["ws"], a["ws_bytes"], a["slices"], None)


def _bwd(L, fake, **kw):
    a = dict(B=2, C=3, N=315, x=fake, g=fake, w=fake, b=fake, stats=fake, slope=0.01, dx=fake, dw=fake, db=fake, ws=fake,
             ws_bytes=L.mgs_abn_workspace_bytes(2, 3, 315), slices=0)
    a.update(kw)
    return L.mgs_abn_backward(a["B"], a["C"], a["N"], a["x"], a["g"], a["w"], a["b"], a["stats"], a["slope"], a["dx"], a["dw"],
                              a["db"], a["ws"], a["ws_bytes"], a["slices"], None)


def test_the_library_refuses_bad_arguments_before_any_launch():
    """Every pointer is a fake address: a launch would fault.  Each refusal carries its message."""
    L = _lib.lib()
    fake = 0x10000
    INV = _lib.MGS_ERR_INVALID_ARG
    inf, nan = float("inf"), float("nan")
    both = ((dict(C=0), "C = 0"), (dict(C=65537), "C = 65537"), (dict(B=0), "B = 0"), (dict(N=0), "N = 0"), (dict(N=-5), "N = -5"),
            (dict(N=1 << 31), "2^31 - 1"), (dict(B=1 << 24), "rows"), (dict(slope=nan), "negative_slope"),
            (dict(slope=inf), "negative_slope"), (dict(slices=-1), "slices"), (dict(slices=65), "slices"), (dict(x=None), "NULL"),
            (dict(w=None), "NULL"), (dict(b=None), "NULL"), (dict(stats=None), "NULL"), (dict(ws=None), "NULL"),
            (dict(x=fake + 4), "16-byte aligned"), (dict(ws=fake + 8), "16-byte aligned"))
    for kw, word in both:
        for call in (_fwd, _bwd):
            assert call(L, fake, **kw) == INV, (call.__name__, kw)
            assert word in _lib.last_error(), (call.__name__, kw, _lib.last_error())
    for kw, word in ((dict(y=None), "NULL"), (dict(rm=None), "running_mean or running_var"), (dict(rv=None), "running_mean or running_var"),
                     (dict(training=0, rm=None, rv=None), "eval mode"), (dict(eps=nan), "eps"), (dict(eps=inf), "eps"),
                     (dict(eps=-1e-5), "eps"), (dict(momentum=nan), "momentum"), (dict(momentum=-inf), "momentum"),
                     (dict(y=fake + 4), "16-byte aligned"), (dict(res=fake + 8), "16-byte aligned"),
                     (dict(B=1, N=1), "Expected more than 1 value per channel when training")):
        assert _fwd(L, fake, **kw) == INV and word in _lib.last_error(), (kw, _lib.last_error())
    for kw, word in ((dict(g=None), "NULL"), (dict(dx=None), "NULL"), (dict(dx=fake + 4), "16-byte aligned"),
                     (dict(g=fake + 12), "16-byte aligned")):
        assert _bwd(L, fake, **kw) == INV and word in _lib.last_error(), (kw, _lib.last_error())
    need = L.mgs_abn_workspace_bytes(2, 3, 315)
    for call in (_fwd, _bwd):
        assert call(L, fake, ws_bytes=need - 1) == _lib.MGS_ERR_WORKSPACE and "needed" in _lib.last_error()


def test_the_workspace_size_is_zero_for_illegal_shapes_and_aligned_otherwise():
    W = _lib.lib().mgs_abn_workspace_bytes
    n = 100 ** 3
    sizes = [W(b, c, n) for b, c in ((1, 1), (1, 8), (2, 8), (1, 64), (4, 64), (1, 65536))]
    assert all(s > 0 and s % 256 == 0 for s in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    assert 8 * 64 * 16 <= W(1, 8, n) <= 1 << 16, "records per sub-slice, never anything of the row's length"
    assert W(1, 8, 1) == W(1, 8, n) == W(1, 8, 2 ** 31 - 1), "independent of N"
    for b, c, m in ((0, 8, n), (-1, 8, n), (1, 0, n), (1, -3, n), (1, 65537, n), (1, 8, 0), (1, 8, -1), (1, 8, 2 ** 31),
                    (2 ** 25, 1, n), (2 ** 20, 64, n), (2 ** 62, 2, n)):
        assert W(b, c, m) == 0, (b, c, m)


def test_the_op_refuses_cpu_tensors_other_dtypes_and_one_value_per_channel():
    C = 3
    w, b, rm, rv = torch.ones(C), torch.zeros(C), torch.zeros(C), torch.ones(C)
    with pytest.raises(RuntimeError, match="no CPU path"):
        enc.batch_norm_act(torch.zeros(2, C, 2, 2, 2), w, b, rm, rv, training=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        enc.batch_norm_act(torch.zeros(2, C, 2, 2, 2, dtype=torch.float64), w, b, rm, rv, training=False)


def test_the_drop_in_stem_keeps_the_references_names():
    import manigaussian_amd as mg
    assert mg.MultiLayer3DEncoderShallow is enc.MultiLayer3DEncoderShallow and mg.batch_norm_act is enc.batch_norm_act
    assert mg.InPlaceABN is enc.InPlaceABN and mg.ConvBnReLU3D is enc.ConvBnReLU3D
    m = enc.MultiLayer3DEncoderShallow()
    assert list(m.state_dict()) == ac.stem_state_dict_names()
    assert isinstance(m.conv0.bn.bn, torch.nn.BatchNorm3d) and isinstance(m.conv7[1].bn, torch.nn.BatchNorm3d)
    assert m.out_channels == 64 and m.conv_out.out_channels == 64 and m.conv0.conv.in_channels == 10
    assert enc.MultiLayer3DEncoderShallow(in_channels=4, out_channels=5).conv_out.out_channels == 5
    assert isinstance(enc.InPlaceABN(4, activation="relu").act, torch.nn.ReLU) and enc.InPlaceABN(4).act.negative_slope == 0.01
    with pytest.raises(ValueError):
        enc.InPlaceABN(4, activation="gelu")
    for size in (12, 20):   # (the reference's shapes at both sizes)
        m.eval()
        with torch.no_grad():
            out, voxels = m(torch.zeros(1, 10, size, size, size))
        assert out.shape == (1, 64, size, size, size)
        assert [tuple(v.shape) for v in voxels] == [(1, 10, size, size, size), (1, 32, size // 4, size // 4, size // 4),
                                                    (1, 16, size // 2, size // 2, size // 2)]


@pytest.mark.skipif(not ac.have_reference(), reason="no copy of the reference on this machine")
def test_a_reference_state_dict_loads_strict_both_ways_and_the_cpu_stem_equals_the_reference_bit_for_bit(route):
    ref = ac.load_reference()
    torch.manual_seed(11)
    theirs = ref.MultiLayer3DEncoderShallow()
    torch.manual_seed(11)
    ours = enc.MultiLayer3DEncoderShallow()
    assert all(torch.equal(a, b) for a, b in zip(ours.state_dict().values(), theirs.state_dict().values())), "the same initialisation"
    torch.manual_seed(12)
    fresh = ref.MultiLayer3DEncoderShallow()
    ours.load_state_dict(fresh.state_dict(), strict=True)
    theirs.load_state_dict(ours.state_dict(), strict=True)   # ... and the other way round
    x = torch.randn(2, 10, 12, 12, 12, generator=torch.Generator().manual_seed(13))
    for force in (None, True):   # (a CPU tensor takes torch's composition whatever the switch says)
        route(force)
        ours.zero_grad()
        theirs.zero_grad()
        xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        (ya, va), (yb, vb) = ours(xa), theirs(xb)
        (ya.sum() + va[1].pow(2).sum() + va[2].pow(2).sum()).backward()
        (yb.sum() + vb[1].pow(2).sum() + vb[2].pow(2).sum()).backward()
        assert torch.equal(ya, yb) and all(torch.equal(a, b) for a, b in zip(va, vb)) and torch.equal(xa.grad, xb.grad)
        for (n, a), b in zip(ours.named_parameters(), theirs.parameters()):
            assert torch.equal(a.grad, b.grad), n
        for (n, a), b in zip(ours.named_buffers(), theirs.buffers()):
            assert torch.equal(a, b), n


def test_the_drop_in_falls_back_to_torchs_composition(route):
    route(True)
    m = enc.InPlaceABN(3)
    x = torch.randn(2, 3, 2, 3, 4)
    res = torch.randn(2, 3, 2, 3, 4)
    F = torch.nn.functional
    want = res + F.leaky_relu(F.batch_norm(x, None, None, m.bn.weight, m.bn.bias, True, 0.1, 1e-5), 0.01)
    assert torch.equal(m(x.clone(), residual=res), want)
    assert int(m.bn.num_batches_tracked) == 1
    assert not m._fused(x) and not m._fused(x.double())
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        m(torch.zeros(1, 3, 1, 1, 1))


def test_the_routing_rule_matches_the_committed_measurement():
    """profiles/encoder_bench.json (scripts/bench_encoder.py on an MI355X): the rule fuses a shape ONLY where the fused side's third
    quartile lay below torch's first quartile in all four (pass, form) pairs -- and it does fuse the stem's two largest sites."""
    import json
    with open(os.path.join(ROOT, "profiles", "encoder_bench.json")) as f:
        bench = json.load(f)
    assert len(bench["shapes"]) == 7 and sorted(s for v in bench["shapes"].values() for s in v["sites"]) == sorted(
        ["conv0", "conv1", "conv2", "conv3", "conv4", "conv5", "conv6", "conv7", "conv9", "conv11"])
    fused = []
    for key, v in bench["shapes"].items():
        won = all(v[p][f]["fused"]["q3_us"] < v[p][f]["torch"]["q1_us"] for p in ("forward", "forward_backward")
                  for f in ("eager", "graph"))
        assert won == v["fused_wins"] == bench["routing_as_measured"][key], key
        if enc.fused_site(v["side"] ** 3, v["C"]):
            assert won, key
            fused += v["sites"]
        assert bench["routing_in_the_package"][key] == enc.fused_site(v["side"] ** 3, v["C"]), key
    assert sorted(fused) == ["conv0", "conv11"]
    assert enc.FORCE is None


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
def run(t, case_or_slope, training=True, slices=0, x=None, hooks=None):
    """{quantity: CPU tensor} of one forward (+ backward) of the op on a fixture-shaped dict `t`; fresh running buffers (0, 1) unless
    `t` holds running_mean0 / running_var0."""
    slope = ac.slope_of(case_or_slope) if isinstance(case_or_slope, str) else case_or_slope
    d = dev()
    x = (t["x"].to(d) if x is None else x).detach().requires_grad_(training)   # (a leaf of this run alone; strides and offset kept)
    w, b = (t[k].to(d).clone().requires_grad_(training) for k in ("weight", "bias"))
    res = t["residual"].to(d).clone().requires_grad_(training) if "residual" in t else None
    C = w.numel()
    rm = t["running_mean0"].to(d).clone() if "running_mean0" in t else torch.zeros(C, device=d)
    rv = t["running_var0"].to(d).clone() if "running_var0" in t else torch.ones(C, device=d)
    nbt = torch.zeros((), dtype=torch.int64, device=d)
    y = enc._batch_norm_act(x, w, b, rm, rv, nbt, training, ac.MOMENTUM, ac.EPS, slope, res, slices=slices)
    out = {"y": y.detach().cpu(), "running_mean": rm.cpu(), "running_var": rv.cpu(), "nbt": int(nbt)}
    if training:
        g = t["g"].to(d)
        if hooks is not None:
            res.register_hook(lambda grad: hooks.append(grad))
        y.backward(g)
        out.update(dx=x.grad.cpu(), dweight=w.grad.cpu(), dbias=b.grad.cpu(), dres=None if res is None else res.grad.cpu(), g=g)
    return out


def check(tag, got, truth, ref_err, z64=None, kink_share=0.0):
    """got within the rule of truth ({quantity: float64 CPU tensor}), quantity by quantity; every figure printed first."""
    fails = []
    for q in ac.QUANTITIES:
        if q not in truth:
            continue
        diff = (got[q].double() - truth[q]).abs()
        if q == "dx" and z64 is not None:
            near = ac.near_kink(z64)
            share = near.double().mean().item()
            assert share <= kink_share, (tag, "elements near the kink", share)
            diff = diff[~near]
        e, bnd = diff.max().item(), ac.bound(ref_err[q], truth[q])
        print(f"{tag} {q}: err {e:.3e}, bound {bnd:.3e} (yardstick {ref_err[q]:.2e} of max|truth| {truth[q].abs().max().item():.3e})")
        if not e <= bnd:
            fails.append((q, e, bnd))
    assert not fails, (tag, fails)


@gpu
@pytest.mark.parametrize("case", list(ac.CASES))
def test_every_fixture_forward_backward_and_running_buffers(case):
    f = ac.load_fixture(case)
    training = ac.CASES[case].get("training", True)
    got = run(f, case, training=training)
    truth = {q: f[q + "64"] for q in ac.QUANTITIES if q + "64" in f}
    z64 = _restated(f, case, torch.float64)[1]
    if case == "dead_channel":   # every element of the dead channel is AT the kink, with dx = 0 whatever the branch: compared
        z64 = z64.clone()
        z64[:, ac.CASES[case]["dead"]] = 1.0
    check(case, got, truth, f["ref_err"], z64)
    if training:
        assert got["nbt"] == 1, "num_batches_tracked advanced by one"
        if "residual" in f:
            assert ac.same_bits(got["dres"], f["g"]), "the skip tensor's gradient is the incoming gradient"
    else:
        assert got["nbt"] == 0 and ac.same_bits(got["running_mean"], f["running_mean0"]) and ac.same_bits(got["running_var"], f["running_var0"])


@gpu
def test_one_value_per_channel_raises_torchs_message_and_eval_has_no_backward():
    d = dev()
    C = 3
    w, b, rm, rv = torch.ones(C, device=d), torch.zeros(C, device=d), torch.zeros(C, device=d), torch.ones(C, device=d)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        enc.batch_norm_act(torch.zeros(1, C, 1, 1, 1, device=d), w, b, rm, rv, training=True)
    y = enc.batch_norm_act(torch.full((1, C, 1, 1, 1), 2.0, device=d), w, b, rm, rv, training=False)   # (fine in eval mode)
    assert torch.allclose(y.cpu(), torch.full((1, C, 1, 1, 1), 2.0 / (1 + 1e-5) ** 0.5))
    with pytest.raises(ValueError, match="momentum"):
        enc.batch_norm_act(torch.zeros(2, C, 2, 2, 2, device=d), w, b, rm, rv, training=True, momentum=None)
    x = torch.zeros(2, C, 2, 2, 2, device=d, requires_grad=True)
    with pytest.raises(RuntimeError, match="no backward in eval mode"):
        enc.batch_norm_act(x, w, b, rm, rv, training=False).sum().backward()


_FULL_CACHE = {}


def full_inputs(name):
    """Inputs on the CPU, the float64 restatement's results (run on the device) and the float32 one's errors: computed once, shared."""
    if name not in _FULL_CACHE:
        shape, with_res = FULL[name]
        C = shape[1]
        g = torch.Generator().manual_seed(4000 + list(FULL).index(name))
        t = {"x": torch.randn(*shape, generator=g) * 0.7 + 0.2, "g": torch.randn(*shape, generator=g),
             "weight": 1.0 + 0.5 * torch.randn(C, generator=g), "bias": 0.3 * torch.randn(C, generator=g)}
        if with_res:
            t["residual"] = torch.randn(*shape, generator=g)
        res = {}
        for dtype in (torch.float64, torch.float32):
            out, z = _restated(t, "tiny", dtype, device=dev())
            res[dtype] = {q: v.double().cpu() for q, v in out.items()}
            if dtype == torch.float64:
                z64 = z.cpu()
            del out, z
        t64, t32 = res[torch.float64], res[torch.float32]
        err = {q: (t32[q] - t64[q]).abs().max().item() / t64[q].abs().max().item() for q in t64}
        _FULL_CACHE[name] = dict(t=t, truth=t64, ref_err=err, z64=z64)
        torch.cuda.empty_cache()
    return _FULL_CACHE[name]


@gpu
@pytest.mark.parametrize("name", list(FULL))
def test_full_size_against_float64(name):
    c = full_inputs(name)
    got = run(c["t"], 0.01)
    check(name, got, c["truth"], c["ref_err"], c["z64"], KINK_SHARE)
    assert got["nbt"] == 1


@gpu
def test_the_same_bits_across_two_runs_and_across_slice_counts():
    """long_odd has 64 sub-slices per row, odd has one: `slices` decides which workgroup reduces which, never what is summed."""
    for t, tag in ((full_inputs("long_odd")["t"], "long_odd"), (ac.load_fixture("odd"), "odd"), (ac.load_fixture("offset"), "offset")):
        first = run(t, 0.01)
        for slices in (0, 1, 2, 7, 64):
            again = run(t, 0.01, slices=slices)
            for q in ac.QUANTITIES:
                assert ac.same_bits(first[q], again[q]), (tag, slices, q)


@gpu
def test_the_residual_gradient_is_the_incoming_tensor_itself():
    f = ac.load_fixture("tiny")
    seen = []
    got = run(f, "tiny", hooks=seen)
    assert len(seen) == 1 and seen[0].data_ptr() == got["g"].data_ptr() and seen[0].shape == got["g"].shape, "uncopied"


@gpu
def test_non_contiguous_and_offset_views_give_the_contiguous_result():
    f = ac.load_fixture("odd")
    want = run(f, "odd")
    x = f["x"].to(dev())
    view = x.permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3)  # channels last in memory
    assert not view.is_contiguous() and torch.equal(view, x)
    flat = torch.empty(x.numel() + 1, device=dev())
    shifted = flat[1:].view(x.shape)   # contiguous, 4 bytes off a 16-byte boundary
    shifted.copy_(x)
    assert shifted.is_contiguous() and shifted.data_ptr() % 16 == 4
    for tag, v in (("channels last", view), ("4-byte offset", shifted)):
        got = run(f, "odd", x=v)
        for q in ac.QUANTITIES:
            assert ac.same_bits(got[q], want[q]), (tag, q)


@gpu
def test_nothing_of_the_volumes_size_is_held_beside_x():
    c = full_inputs("site0")
    d = dev()
    t = {k: v.to(d) for k, v in c["t"].items()}
    x = t["x"].requires_grad_(True)
    w, b = t["weight"].requires_grad_(True), t["bias"].requires_grad_(True)
    rm, rv = torch.zeros(8, device=d), torch.ones(8, device=d)
    volume = x.numel() * 4

    def forward():
        return enc.batch_norm_act(x, w, b, rm, rv, training=True, residual=t["residual"])

    forward()  # (the cached workspace exists from here on)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    y = forward()
    torch.cuda.synchronize()
    fwd_peak = torch.cuda.max_memory_allocated() - base
    y.backward(t["g"])
    torch.cuda.synchronize()
    total = torch.cuda.max_memory_allocated() - base
    print(f"volume {volume} bytes: forward peak +{fwd_peak}; forward + backward peak +{total}")
    assert fwd_peak <= volume + (1 << 20), "y and nothing else"
    assert total <= 2 * volume + (1 << 20), "y and dx"


@gpu
def test_the_drop_in_stem_fused_against_torchs_path(route):
    """[1,10,12,12,12]: the same module with every site fused and with none; the truth is the module in float64 on the CPU."""
    d = dev()
    torch.manual_seed(21)
    m = enc.MultiLayer3DEncoderShallow().to(d)
    state = {k: v.clone() for k, v in m.state_dict().items()}
    gen = torch.Generator().manual_seed(22)
    x = torch.randn(1, 10, 12, 12, 12, generator=gen).to(d)
    g_out, g_v1, g_v2 = (torch.randn(*s, generator=gen).to(d) for s in ((1, 64, 12, 12, 12), (1, 32, 3, 3, 3), (1, 16, 6, 6, 6)))

    def once(force, dtype, where):
        route(force)
        m.load_state_dict(state)
        m.to(where, dtype).train().zero_grad()
        out, voxels = m(x.to(where, dtype))
        to = dict(device=where, dtype=dtype)
        ((out * g_out.to(**to)).sum() + (voxels[1] * g_v1.to(**to)).sum() + (voxels[2] * g_v2.to(**to)).sum()).backward()
        r = {"out": out.detach(), "voxel1": voxels[1].detach(), "voxel2": voxels[2].detach()}
        r.update({"grad " + n: p.grad for n, p in m.named_parameters()})
        r.update({n: b.clone() for n, b in m.named_buffers() if b.dtype.is_floating_point})
        counts = [int(b) for n, b in m.named_buffers() if n.endswith("num_batches_tracked")]
        r = {k: v.detach().double().cpu().clone() for k, v in r.items()}   # (copies: m.to() below converts the gradients in place)
        m.to(d, torch.float32)
        return r, counts

    truth, _ = once(False, torch.float64, "cpu")
    torchs, n_torch = once(False, torch.float32, d)
    fused, n_fused = once(True, torch.float32, d)
    assert n_torch == n_fused == [1] * 10
    fails = []
    for k, want in truth.items():
        mag = want.abs().max().item()
        yard = (torchs[k] - want).abs().max().item() / mag
        e, bnd = (fused[k] - want).abs().max().item(), max(ac.FACTOR * yard, ac.FACTOR * ac.FLOOR) * mag
        print(f"stem {k}: err {e:.3e}, bound {bnd:.3e} (torch's fp32 path {yard:.2e} of {mag:.3e})")
        if not e <= bnd:
            fails.append((k, e, bnd))
    assert not fails, fails
    assert any((fused[k] != torchs[k]).any() for k in fused), "the forced route changed nothing: the fused path did not run"


@gpu
def test_forward_and_backward_captured_into_a_hip_graph():
    """In a child process: stream capture is process-wide state (tests/tools/abn_graph_capture_check.py)."""
    run_graph_tool("abn_graph_capture_check.py")
