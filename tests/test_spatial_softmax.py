"""The fused SpatialSoftmax3D + global max-pool (manigaussian_amd/spatial_softmax.py, csrc/mgs_spatial_softmax.hip) against
ManiGaussian's own SpatialSoftmax3D (helpers/network_utils.py:927-963) and nn.AdaptiveMaxPool3d(1).

The yardstick is the reference's own fp32 rounding error: a fixture (tests/golden/spatial_softmax/, tests/spatial_softmax_cases.py)
holds the reference's float64 result -- the truth -- and how far the reference's float32 run lies from it.
  maxpool    equals max(x) bit for bit;
  keypoints  |ours - kp64| <= max(16 x ref_abs_err, 16 x 2^-23): absolute, coordinates live in [-1, 1] and may be 0;
  dx         |ours - dx64| <= 16 x ref_err x max|dx64|.
On the GPU machine the reference does not exist: the full-size tests take the same formula in plain torch ops
(spatial_softmax_cases.restatement, pinned against the fixtures here) in float64 as the truth and in float32 as the yardstick.
"""
import os

import numpy as np
import pytest
import torch

from child import run_graph_tool
from numerics import dev
import spatial_softmax_cases as sc

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = sc.TEMPERATURE
FULL = {"d0_rows": ((1, 8, 100, 100, 100), 0.3, 0.5),      # the production row length, many slices
        "ss1": ((1, 128, 20, 20, 20), 0.3, 0.5),           # the production ss1
        "long_odd": ((2, 3, 101, 99, 103), 0.3, 0.5)}      # long, odd, misaligned, non-cube


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not sc.have_reference(), reason="no copy of the reference on this machine")
def test_fixtures_match_the_reference():
    """The generator's computation, re-run.  Inputs and integers bit for bit; the float64 truth to 1e-12 of its magnitude (the
    order of a CPU's sums may follow its thread count); the yardsticks, maxima of float32 rounding errors, within a factor of 2."""
    for case in sc.CASES:
        f, now = sc.load_fixture(case), sc.reference_case(case)
        yard = dict(zip(("kp", "dx", "dx_k"), [float(now["ref_abs_err"])] + now["ref_err"].tolist()))
        for n, e in yard.items():
            c = f["ref_err"][n]
            assert (e == 0 and c == 0) or 0.5 * c <= e <= 2 * c, (case, n, e, c)
            assert e <= sc.REF_ERR_CEILING, (case, n, e)
        for k, v in now.items():
            if k in ("ref_err", "ref_abs_err"):
                continue
            if v.dtype == np.float64:
                t = torch.from_numpy(v)
                assert (t - f[k]).abs().max().item() <= 1e-12 * max(t.abs().max().item(), 1e-300), (case, k)
            else:
                assert np.array_equal(v, f[k].numpy()), (case, k)
        assert (set(now) - {"ref_abs_err"}) | {"dx64_k"} == set(f), case


def test_fixtures_are_small():
    for case in sc.CASES:
        assert os.path.getsize(sc.fixture_path(case)) <= 1_000_000, case
        with np.load(sc.fixture_path(case), allow_pickle=False) as z:
            assert all(z[k].dtype.kind in "fi" for k in z.files), case
            assert float(z["ref_abs_err"]) <= sc.REF_ERR_CEILING and float(z["ref_err"].max()) <= sc.REF_ERR_CEILING, case


def test_the_float64_restatement_reproduces_every_fixture():
    """Pins restatement(), the GPU tests' stand-in for the reference, and first_argmax() (the max-pool's tie rule)."""
    for case in sc.CASES:
        f = sc.load_fixture(case)
        B, C, D, H, W = f["x"].shape
        assert torch.equal(sc.first_argmax(f["x"]), f["argmax"]), case
        for name, with_max in (("dx64", True), ("dx64_k", False)):
            x = f["x"].double().requires_grad_(True)
            kp, mx = sc.restatement(x, D, H, W, T, torch.float64)
            loss = (kp * f["g_k"].double()).sum()
            if with_max:
                # (torch.max routes a tied maximum's gradient elsewhere than the pooling layer does: the first index, by hand)
                flat = x.reshape(B * C, -1)
                loss = loss + (flat[torch.arange(B * C), f["argmax"]] * f["g_m"].double().reshape(-1)).sum()
            loss.backward()
            for got, want, what in ((kp.detach(), f["kp64"], "kp64"), (mx.detach(), f["max64"], "max64"), (x.grad, f[name], name)):
                mag = want.abs().max().item()
                assert (got - want).abs().max().item() <= 1e-12 * mag, (case, what)
    assert int((sc.load_fixture("ties")["x"][0, 0] == sc.load_fixture("ties")["x"][0, 0].max()).sum()) > 100, "ties has no ties"


def test_the_modules_buffers_are_the_references_tables():
    from manigaussian_amd import SpatialSoftmax3D
    f = sc.load_fixture("noncube")
    _, C, D, H, W = f["x"].shape
    m = SpatialSoftmax3D(D, H, W, C)
    assert m.temperature == 0.01 and (m.depth, m.height, m.width, m.channel) == (D, H, W, C)
    assert sorted(m.state_dict()) == ["pos_x", "pos_y", "pos_z"]
    for n, t in zip(("pos_x", "pos_y", "pos_z"), sc.position_tables(D, H, W)):
        assert sc.same_bits(getattr(m, n), f[n]), n
        assert sc.same_bits(t, f[n]), n
    # the index arithmetic the kernels use (mgsplat.h): i = (a D + b) W + c, pos_x = lin_D[b], pos_y = lin_H[a], pos_z = lin_W[c]
    i = torch.arange(D * H * W)
    lin = [torch.from_numpy(np.linspace(-1., 1., n)).float() for n in (D, H, W)]
    assert torch.equal(lin[0][(i // W) % D], f["pos_x"]) and torch.equal(lin[1][i // (D * W)], f["pos_y"])
    assert torch.equal(lin[2][i % W], f["pos_z"])
    assert torch.equal(SpatialSoftmax3D(1, 1, 1, 2).pos_x, torch.tensor([-1.0]))


def _fwd(L, fake, **kw):
    a = dict(rows=6, C=3, D=5, H=7, W=9, t=0.01, feature=fake, kp=fake, kp_stride=12, mp=fake, mp_stride=12, stats=fake, ws=fake,
             ws_bytes=L.mgs_spatial_softmax_workspace_bytes(6, 315), slices=0)
    a.update(kw)
    return L.mgs_spatial_softmax_forward(a["rows"], a["C"], a["D"], a["H"], a["W"], a["t"], a["feature"], a["kp"], a["kp_stride"],
                                         a["mp"], a["mp_stride"], a["stats"], a["ws"], a["ws_bytes"], a["slices"], None)


def _bwd(L, fake, **kw):
    a = dict(rows=6, C=3, D=5, H=7, W=9, t=0.01, feature=fake, stats=fake, gk=fake, gk_stride=9, gm=fake, gm_stride=3, gx=fake,
             slices=0)
    a.update(kw)
    return L.mgs_spatial_softmax_backward(a["rows"], a["C"], a["D"], a["H"], a["W"], a["t"], a["feature"], a["stats"], a["gk"],
                                          a["gk_stride"], a["gm"], a["gm_stride"], a["gx"], a["slices"], None)


def test_the_library_refuses_bad_arguments_before_any_launch():
    from manigaussian_amd import _lib
    L = _lib.lib()
    fake = 0x10000
    INV = _lib.MGS_ERR_INVALID_ARG
    both = ((dict(rows=0), "rows = 0"), (dict(D=0), "D = 0"), (dict(H=-1), "H = -1"), (dict(W=0), "W = 0"), (dict(C=0), "C = 0"),
            (dict(rows=7), "no multiple"), (dict(D=1 << 11, H=1 << 10, W=1 << 10), "2^31 - 1"), (dict(rows=3 << 25, C=3), "rows ="),
            (dict(t=0.0), "temperature"), (dict(t=-0.01), "temperature"), (dict(t=float("inf")), "temperature"),
            (dict(t=float("nan")), "temperature"), (dict(t=1e-45), "temperature"), (dict(slices=-1), "slices"),
            (dict(slices=65), "slices"), (dict(feature=None), "NULL"), (dict(stats=None), "NULL"),
            (dict(feature=fake + 4), "16-byte aligned"))
    for kw, word in both:
        for call in (_fwd, _bwd):
            assert call(L, fake, **kw) == INV, (call.__name__, kw)
            assert word in _lib.last_error(), (call.__name__, kw, _lib.last_error())
    for kw, word in ((dict(kp=None), "NULL"), (dict(ws=None), "NULL"), (dict(ws=fake + 8), "16-byte aligned"),
                     (dict(kp_stride=8), "row strides"), (dict(mp_stride=2), "row strides")):
        assert _fwd(L, fake, **kw) == INV and word in _lib.last_error(), (kw, _lib.last_error())
    for kw, word in ((dict(gx=None), "NULL"), (dict(gx=fake + 4), "16-byte aligned"), (dict(gk_stride=8), "row strides"),
                     (dict(gm_stride=2), "row strides")):
        assert _bwd(L, fake, **kw) == INV and word in _lib.last_error(), (kw, _lib.last_error())
    need = L.mgs_spatial_softmax_workspace_bytes(6, 315)
    assert _fwd(L, fake, ws_bytes=need - 1) == _lib.MGS_ERR_WORKSPACE and "needed" in _lib.last_error()


def test_the_workspace_size_is_monotone_and_aligned():
    from manigaussian_amd import _lib
    W = _lib.lib().mgs_spatial_softmax_workspace_bytes
    n = 100 ** 3
    assert W(128, n) % 256 == 0 and 128 * 32 <= W(128, n) <= 1 << 19, "records per slice, never anything of the row's length"
    sizes = [W(r, n) for r in (1, 2, 8, 64, 128, 129, 1024)]
    assert all(a < b or (a == b and a > 0) for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0 and sizes[-1] > sizes[0]
    assert all(s % 256 == 0 for s in sizes)
    assert W(8, 1) <= W(8, 8000) <= W(8, n) <= W(8, 2 ** 31 - 1), "not decreasing in N"
    assert W(0, n) == 0 and W(8, 0) == 0 and W(8, 2 ** 31) == 0 and W(-1, n) == 0


def test_the_module_refuses_cpu_tensors_wrong_shapes_and_other_dtypes():
    from manigaussian_amd import SpatialSoftmax3D, spatial_softmax3d
    m = SpatialSoftmax3D(5, 7, 9, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(torch.zeros(2, 3, 5, 7, 9))
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.forward_with_max(torch.zeros(2, 3, 5, 7, 9))
    for dtype in (torch.float64, torch.float16, torch.bfloat16):
        with pytest.raises(RuntimeError, match=str(dtype).replace(".", r"\.")):
            m(torch.zeros(2, 3, 5, 7, 9, dtype=dtype))
    with pytest.raises(RuntimeError, match="no CPU path"):
        spatial_softmax3d(torch.zeros(1, 1, 2, 2, 2), with_max=True)
    for bad in ((2, 3, 7, 5, 9), (2, 4, 5, 7, 9), (3, 5, 7, 9), (2, 3, 5, 7 * 9)):
        with pytest.raises(ValueError) as e:
            m(torch.zeros(*bad))
        assert str(bad) in str(e.value) and "[B, 3, 5, 7, 9]" in str(e.value), str(e.value)


def test_a_reference_shaped_state_dict_loads_strict():
    from manigaussian_amd import SpatialSoftmax3D
    f = sc.load_fixture("noncube")
    m = SpatialSoftmax3D(5, 7, 9, 3)
    for n in ("pos_x", "pos_y", "pos_z"):
        getattr(m, n).zero_()
    m.load_state_dict({n: f[n] for n in ("pos_x", "pos_y", "pos_z")}, strict=True)
    assert all(torch.equal(getattr(m, n), f[n]) for n in ("pos_x", "pos_y", "pos_z"))
    if sc.have_reference():
        ref = sc.load_reference().SpatialSoftmax3D(5, 7, 9, 3)
        ref.load_state_dict(m.state_dict(), strict=True)  # ... and the other way round
        m.load_state_dict(ref.state_dict(), strict=True)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
def run(x, g_k, g_m, slices=0, module=None):
    """(keypoints, maxpool, dx) on the CPU: through the module (forward_with_max, or forward alone when g_m is None) or, with a
    forced split, through the private function underneath."""
    x = x.detach().to(dev()).clone().requires_grad_(True)  # (a leaf of this run alone, also when x already lives on the device)
    if module is not None:
        kp, mx = module.forward_with_max(x) if g_m is not None else (module(x), None)
    else:
        from manigaussian_amd.spatial_softmax import _spatial_softmax3d
        kp, mx = _spatial_softmax3d(x, T, slices=slices)
    loss = (kp * g_k.to(dev())).sum()
    if g_m is not None:
        loss = loss + (mx * g_m.to(dev())).sum()
    loss.backward()
    return kp.detach().cpu(), None if mx is None else mx.detach().cpu(), x.grad.cpu()


def check_against_fixture(case, kp, mx, dx, which, tag):
    f, b = sc.load_fixture(case), sc.bounds(case)
    e_kp = (kp.double() - f["kp64"]).abs().max().item()
    e_dx = (dx.double() - f["dx64" if which == "dx" else "dx64_k"]).abs().max().item()
    print(f"{case} {tag}: keypoints err {e_kp:.3e} (bound {b['kp']:.3e}), {which} err {e_dx:.3e} (bound {b[which]:.3e})")
    assert e_kp <= b["kp"], (case, tag, e_kp, b["kp"])
    assert e_dx <= b[which], (case, tag, which, e_dx, b[which])
    if mx is not None:
        assert sc.same_bits(mx, f["x"].amax(dim=(2, 3, 4))), (case, tag, "maxpool")
        assert torch.equal(mx.double(), f["max64"]), (case, tag, "max64")


@gpu
@pytest.mark.parametrize("case", list(sc.CASES))
def test_every_fixture_forward_and_backward(case):
    from manigaussian_amd import SpatialSoftmax3D
    f = sc.load_fixture(case)
    B, C, D, H, W = f["x"].shape
    m = SpatialSoftmax3D(D, H, W, C).to(dev())
    kp, mx, dx = run(f["x"], f["g_k"], f["g_m"], module=m)
    assert kp.shape == (B, 3 * C) and mx.shape == (B, C) and dx.shape == f["x"].shape
    check_against_fixture(case, kp, mx, dx, "dx", "forward_with_max")
    kp_only, _, dx_k = run(f["x"], f["g_k"], None, module=m)
    check_against_fixture(case, kp_only, None, dx_k, "dx_k", "forward")
    assert sc.same_bits(kp_only, kp)
    # the pair is the two halves of one [B, 4C] buffer: the Perceiver's [ss | maxp]
    x = f["x"].to(dev())
    a, b = m.forward_with_max(x)
    assert a._base is not None and a._base is b._base and a._base.shape == (B, 4 * C)
    assert sc.same_bits(torch.cat([a, b], dim=1), a._base)


@gpu
@pytest.mark.parametrize("case", ["cube20", "ties"])
def test_slice_seams(case):
    """The row split forced to 1, 2, 3 and 7 slices: max, the tie rule and the argmax-routed gradient do not depend on it."""
    f = sc.load_fixture(case)
    rows = f["argmax"].numel()
    for slices in (1, 2, 3, 7):
        kp, mx, dx = run(f["x"], f["g_k"], f["g_m"], slices=slices)
        check_against_fixture(case, kp, mx, dx, "dx", f"{slices} slices")
        _, _, dx_k = run(f["x"], f["g_k"], None, slices=slices)
        check_against_fixture(case, kp, None, dx_k, "dx_k", f"{slices} slices")
        routed = (dx != dx_k).reshape(rows, -1)
        assert torch.equal(routed.sum(1), torch.ones(rows, dtype=torch.long)), (case, slices, routed.sum(1))
        assert torch.equal(torch.argmax(routed.to(torch.uint8), dim=1), f["argmax"]), (case, slices)
        at = (torch.arange(rows), f["argmax"])
        want = dx_k.reshape(rows, -1)[at].double() + f["g_m"].reshape(-1).double()  # (one rounding, wherever the kernel adds)
        assert ((dx.reshape(rows, -1)[at].double() - want).abs() <= 2.0 ** -23 * want.abs()).all(), (case, slices)


_FULL_CACHE = {}


def full_inputs(name):
    """x, g_k, g_m on the device, the float64 restatement's (kp, max, dx) and the float32 one's errors: computed once, shared."""
    if name not in _FULL_CACHE:
        shape, scale, shift = FULL[name]
        B, C, D, H, W = shape
        g = torch.Generator().manual_seed(3000 + list(FULL).index(name))
        x = (torch.randn(*shape, generator=g) * scale + shift).to(dev())
        g_k, g_m = torch.randn(B, 3 * C, generator=g).to(dev()), torch.randn(B, C, generator=g).to(dev())
        arg = sc.first_argmax(x)
        res = {}
        for dtype in (torch.float64, torch.float32):
            xx = x.detach().clone().requires_grad_(True)
            kp, mx = sc.restatement(xx, D, H, W, T, dtype)
            picked = xx.reshape(B * C, -1)[torch.arange(B * C, device=dev()), arg].to(dtype)  # the pooling layer's tie rule
            ((kp * g_k.to(dtype)).sum() + (picked * g_m.to(dtype).reshape(-1)).sum()).backward()
            res[dtype] = (kp.detach().double(), mx.detach().double(), xx.grad.double())
            del xx, kp, mx, picked
        t, s = res[torch.float64], res[torch.float32]
        _FULL_CACHE[name] = dict(x=x, g_k=g_k, g_m=g_m, kp64=t[0], max64=t[1], dx64=t[2],
                                 kp_err32=(s[0] - t[0]).abs().max().item(), dx_err32=(s[2] - t[2]).abs().max().item())
    return _FULL_CACHE[name]


@gpu
@pytest.mark.parametrize("name", list(FULL))
def test_full_size_against_float64(name):
    from manigaussian_amd import SpatialSoftmax3D
    c = full_inputs(name)
    B, C, D, H, W = FULL[name][0]
    m = SpatialSoftmax3D(D, H, W, C).to(dev())
    x = c["x"].detach().clone().requires_grad_(True)
    kp, mx = m.forward_with_max(x)
    ((kp * c["g_k"]).sum() + (mx * c["g_m"]).sum()).backward()
    e_kp = (kp.detach().double() - c["kp64"]).abs().max().item()
    e_dx = (x.grad.double() - c["dx64"]).abs().max().item()
    b_kp, b_dx = sc.kp_bound(c["kp_err32"]), sc.FACTOR * c["dx_err32"]
    print(f"{name}: keypoints err {e_kp:.3e}, the fp32 torch sequence {c['kp_err32']:.3e}, bound {b_kp:.3e}; "
          f"dx err {e_dx:.3e}, the fp32 torch sequence {c['dx_err32']:.3e}, bound {b_dx:.3e}, max|dx| {c['dx64'].abs().max().item():.3e}")
    assert torch.equal(mx.detach().double(), c["max64"]), name
    assert e_kp <= b_kp, (name, e_kp, b_kp)
    assert e_dx <= b_dx, (name, e_dx, b_dx)


@gpu
@pytest.mark.parametrize("case", ["odd31", "ties"])
def test_two_runs_are_bit_identical(case):
    f = sc.load_fixture(case)
    a, b = run(f["x"], f["g_k"], f["g_m"]), run(f["x"], f["g_k"], f["g_m"])
    for p, q in zip(a, b):
        assert sc.same_bits(p, q), case
    c = full_inputs("long_odd")
    a, b = run(c["x"], c["g_k"], c["g_m"]), run(c["x"], c["g_k"], c["g_m"])
    for p, q in zip(a, b):
        assert sc.same_bits(p, q), "long_odd"


@gpu
def test_a_non_contiguous_input_equals_its_contiguous_copy():
    f = sc.load_fixture("noncube")
    x = f["x"].to(dev())
    view = x.permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3)  # channels last in memory
    assert not view.is_contiguous() and torch.equal(view, x)
    a, b = run(x, f["g_k"], f["g_m"]), run(view, f["g_k"], f["g_m"])
    for p, q in zip(a, b):
        assert sc.same_bits(p, q)
    check_against_fixture("noncube", *b, "dx", "channels last")


@gpu
def test_nothing_of_the_volumes_size_is_held():
    from manigaussian_amd import spatial_softmax3d
    c = full_inputs("d0_rows")
    x = c["x"].detach().clone().requires_grad_(True)
    volume = x.numel() * 4

    def forward():
        return spatial_softmax3d(x, T, with_max=True)

    forward()  # (the cached workspace exists from here on)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    kp, mx = forward()
    torch.cuda.synchronize()
    fwd_peak, fwd_held = torch.cuda.max_memory_allocated() - base, torch.cuda.memory_allocated() - base
    ((kp * c["g_k"]).sum() + (mx * c["g_m"]).sum()).backward()
    torch.cuda.synchronize()
    total = torch.cuda.max_memory_allocated() - base
    print(f"volume {volume} bytes: forward peak +{fwd_peak}, held +{fwd_held}; forward + backward peak +{total}")
    assert fwd_peak <= 1 << 20, fwd_peak
    assert total <= volume + (1 << 20), (total, volume)


@gpu
def test_forward_and_backward_captured_into_a_hip_graph():
    """In a child process: stream capture is process-wide state (tests/tools/spatial_softmax_graph_capture_check.py)."""
    run_graph_tool("spatial_softmax_graph_capture_check.py")
