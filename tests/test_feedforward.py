"""The fused layer norm and bias-GEGLU (manigaussian_amd/feedforward.py, csrc/mgs_feedforward.hip) and the PreNorm / GEGLU /
FeedForward drop-ins, against torch's own composition and ManiGaussian's own classes (agents/manigaussian_bc/
perceiver_lang_io.py:56-99).

The yardstick is the reference's own fp32 rounding error (tests/feedforward_cases.py): the truth is torch's composition in
float64, ref_err the same composition's float32 deviation from it over max|truth|, and ours must satisfy
  |ours - truth| <= 16 x max(ref_err, 2^-23) x max|truth|
for the output and every gradient.  Torch's own ref_err is below 4e-7 at every case but the one whose inputs are shifted by 30
(about 1e-6); a logic error is of order 1e-1.  Cases whose relative yardstick is degenerate (D = 1, a constant row, a zero gate)
are checked by value.  At the production shapes the truth is float64 on the GPU and the yardstick torch's float32 run there.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attention_cases as ac
from child import run_graph_tool
import feedforward_cases as fc
from numerics import dev, spy

gpu = pytest.mark.gpu
FUSED_ENTRIES = ("mgs_layernorm_forward", "mgs_layernorm_backward", "mgs_bias_geglu_forward", "mgs_bias_geglu_backward")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LN_NAMES = {"d0": "dx", "d1": "dweight", "d2": "dbias"}
GG_NAMES = {"d0": "dh", "d1": "dbias"}


def check(tag, got, want, ref_err):
    err, allowed = fc.rel_err(got, want), fc.bound(ref_err)
    print(f"{tag}: err {err:.3e}, ref_err {ref_err:.3e}, bound {allowed:.3e}")
    assert tuple(got.shape) == tuple(want.shape), (tag, got.shape, want.shape)
    assert err <= allowed, (tag, err, allowed)


def check_results(tag, got, t, names):
    assert set(got) == set(t["r64"]), (tag, sorted(got))
    for k, want in t["r64"].items():
        check(f"{tag} {names.get(k, k)}", got[k], want, t["ref_err"][k])


def check_module(name, errors, tag):
    for k, (err, ref_err) in errors.items():
        allowed = fc.bound(ref_err)
        print(f"{name} {tag} {k}: err {err:.3e}, ref_err {ref_err:.3e}, bound {allowed:.3e}")
        assert err <= allowed, (name, tag, k, err, allowed)


# ---- CPU -----------------------------------------------------------------------------------------------------------------------
def test_the_cases_yardsticks_stay_under_the_ceiling():
    for kind, cases in (("ln", fc.LN_CASES), ("geglu", fc.GEGLU_CASES)):
        for case in cases:
            e = fc.truth(kind, case)["ref_err"]
            print(kind, case, {k: f"{v:.2e}" for k, v in e.items()})
            assert max(e.values()) <= fc.REF_ERR_CEILING, (kind, case, e)
    assert set(fc.truth("ln", "frozen")["r64"]) == {"out", "d0"}
    x, _, _, g = fc.ln_inputs("strided")
    assert x.stride() == (160, 1) and not x.is_contiguous()
    assert fc.ln_inputs("expanded_g")[3].stride() == (0, 1)
    h, b, _ = fc.geglu_inputs("saturated")
    assert (h[:, 130:] + b[130:]).min().item() <= -40 and (h[:, 130:] + b[130:]).max().item() >= 40
    for r in fc.truth("geglu", "saturated")["r64"].values():
        assert torch.isfinite(r).all()


@pytest.mark.skipif(not fc.have_reference(), reason="no copy of the reference on this machine")
def test_module_fixtures_match_the_reference():
    """The generator's computation, re-run.  Inputs and parameters bit for bit; the float64 truth to 1e-12 of its magnitude; the
    yardsticks, maxima of float32 rounding errors, within a factor of 4."""
    for name in fc.MODULES:
        f, now = fc.load_module_fixture(name), fc.reference_module_case(name)
        assert set(now) == set(f), name
        for k, v in now.items():
            if k.startswith("ref_err."):
                e, c = float(v), f[k]
                assert (e == 0 and c == 0) or 0.25 * c <= e <= 4 * c, (name, k, e, c)
                assert e <= fc.REF_ERR_CEILING, (name, k, e)
            elif v.dtype == np.float64:
                assert fc.rel_err(torch.from_numpy(v), f[k]) <= 1e-12, (name, k)
            else:
                assert np.array_equal(v, f[k].numpy()), (name, k)


def test_module_fixtures_are_small():
    for name in fc.MODULES:
        assert os.path.getsize(fc.module_fixture_path(name)) <= 1_000_000, name
        with np.load(fc.module_fixture_path(name), allow_pickle=False) as z:
            assert all(z[k].dtype.kind in "fi" for k in z.files), name
            assert max(float(z[k]) for k in z.files if k.startswith("ref_err.")) <= fc.REF_ERR_CEILING, name
            assert sorted(k[2:] for k in z.files if k.startswith("p.")) == fc.STATE_KEYS[name], name
            assert {"x", "g", "out64", "dx64", "ref_err.out", "ref_err.dx"} <= set(z.files), name


@pytest.mark.parametrize("name", list(fc.MODULES))
def test_the_drop_ins_reproduce_every_fixture_on_the_cpu(name):
    import manigaussian_amd
    f = fc.load_module_fixture(name)
    m = fc.fixture_module(manigaussian_amd, name)
    assert sorted(m.state_dict()) == fc.STATE_KEYS[name]
    out, dx, dp, dc = fc.run_module(m, f["x"], f["g"], torch.float32, context=f.get("context"))
    assert out.shape == f["out64"].shape
    check_module(name, fc.module_errors(f, out, dx, dp, dc), "cpu")


def test_the_context_fixture_sees_the_normed_context():
    """What the fixture pins: a PreNorm that hands the raw context on misses its truth by far more than the bound."""
    import manigaussian_amd
    f = fc.load_module_fixture("prenorm_context")
    m = fc.fixture_module(manigaussian_amd, "prenorm_context")
    raw = m.fn(F.layer_norm(f["x"], (16,), m.norm.weight, m.norm.bias), context=f["context"])
    assert fc.rel_err(raw.detach(), f["out64"]) > 1e-2


class _Recorder(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.seen = None

    def forward(self, x, **kwargs):
        self.seen = (x, kwargs)
        return x


def test_the_drop_ins_keep_the_references_interface():
    from manigaussian_amd import GEGLU, FeedForward, PreNorm
    ff = FeedForward(8)
    assert isinstance(ff.net, torch.nn.Sequential) and len(ff.net) == 3 and isinstance(ff.net[1], GEGLU)
    assert ff.net[0].weight.shape == (64, 8) and ff.net[2].weight.shape == (8, 32)
    assert sorted(ff.state_dict()) == ["net.0.bias", "net.0.weight", "net.2.bias", "net.2.weight"]
    assert FeedForward(6, mult=1).net[0].weight.shape == (12, 6)
    assert list(GEGLU().parameters()) == []
    p = PreNorm(8, ff)
    assert p.fn is ff and isinstance(p.norm, torch.nn.LayerNorm) and p.norm.eps == 1e-5 and p.norm_context is None
    assert sorted(p.state_dict()) == ["fn.net.0.bias", "fn.net.0.weight", "fn.net.2.bias", "fn.net.2.weight", "norm.bias", "norm.weight"]
    rec = _Recorder()
    pc = PreNorm(8, rec, context_dim=4)
    assert sorted(pc.state_dict()) == ["norm.bias", "norm.weight", "norm_context.bias", "norm_context.weight"]
    gen = torch.Generator().manual_seed(3)
    x, context = torch.randn(2, 3, 8, generator=gen), torch.randn(2, 5, 4, generator=gen)
    out = pc(x, context=context, mask=None)
    assert torch.equal(out, F.layer_norm(x, (8,))) and set(rec.seen[1]) == {"context", "mask"}
    assert torch.equal(rec.seen[1]["context"], F.layer_norm(context, (4,))) and rec.seen[1]["mask"] is None
    pc.get_attention_matrix(x, context=context)
    assert rec.seen[1]["return_attention_weights"] is True and torch.equal(rec.seen[1]["context"], F.layer_norm(context, (4,)))
    PreNorm(8, rec).get_attention_matrix(x)
    assert rec.seen[1] == {"return_attention_weights": True}
    with pytest.raises(KeyError):
        pc(x)


def test_the_same_seed_gives_torchs_own_layers_parameters_in_the_references_order():
    from manigaussian_amd import FeedForward, PreNorm
    torch.manual_seed(77)
    ours = PreNorm(12, FeedForward(12, mult=2), context_dim=5)
    torch.manual_seed(77)
    first, last = torch.nn.Linear(12, 48), torch.nn.Linear(24, 12)   # the reference builds the feed-forward before the norms
    for k, v in (("fn.net.0.weight", first.weight), ("fn.net.0.bias", first.bias), ("fn.net.2.weight", last.weight),
                 ("fn.net.2.bias", last.bias)):
        assert fc.same_bits(ours.state_dict()[k], v.detach()), k
    assert torch.equal(ours.norm.weight, torch.ones(12)) and torch.equal(ours.norm_context.bias, torch.zeros(5))


@pytest.mark.skipif(not fc.have_reference(), reason="no copy of the reference on this machine")
@pytest.mark.parametrize("name", list(fc.MODULES))
def test_a_reference_state_dict_loads_strict_both_ways_and_the_inits_agree(name):
    import manigaussian_amd
    ref = ac.load_reference()
    with torch.random.fork_rng():
        torch.manual_seed(77)
        theirs = fc.new_module(ref, name)
        torch.manual_seed(77)
        ours = fc.new_module(manigaussian_amd, name)
    assert sorted(theirs.state_dict()) == sorted(ours.state_dict()) == fc.STATE_KEYS[name]
    for k, v in theirs.state_dict().items():
        assert fc.same_bits(v, ours.state_dict()[k]), (name, k, "the same seed gives the reference's initial parameters")
    mine = fc.fixture_module(manigaussian_amd, name)
    theirs.load_state_dict(mine.state_dict(), strict=True)
    ours.load_state_dict(theirs.state_dict(), strict=True)
    f = fc.load_module_fixture(name)
    assert all(torch.equal(ours.state_dict()[k], f["p." + k]) for k in fc.STATE_KEYS[name])


def test_what_the_kernels_do_not_take_falls_through_to_torch_bit_for_bit():
    from manigaussian_amd import bias_geglu, layer_norm
    gen = torch.Generator().manual_seed(5)
    for x in (torch.randn(3, 7, 10, generator=gen, dtype=torch.float64), torch.randn(4, 1025, generator=gen),
              torch.randn(3, 10, generator=gen)):
        D = x.shape[-1]
        w, b = torch.randn(D, generator=gen, dtype=x.dtype), torch.randn(D, generator=gen, dtype=x.dtype)
        assert torch.equal(layer_norm(x, w, b, 1e-3), F.layer_norm(x, (D,), w, b, 1e-3))
        assert torch.equal(layer_norm(x, None, None), F.layer_norm(x, (D,)))
    for h in (torch.randn(3, 7, 10, generator=gen, dtype=torch.float64), torch.randn(5, 6, generator=gen)):
        b = torch.randn(h.shape[-1], generator=gen, dtype=h.dtype)
        assert torch.equal(bias_geglu(h, b), fc.geglu_compose(h, b))
        assert torch.equal(bias_geglu(h), fc.geglu_compose(h, None))
    # ... differentiably
    h = torch.randn(5, 6, generator=gen, requires_grad=True)
    bias_geglu(h).sum().backward()
    assert h.grad is not None and h.grad.shape == (5, 6)


def test_rows_are_read_in_place_when_their_stride_is_uniform():
    from manigaussian_amd.feedforward import _by_rows
    base = torch.zeros(4, 9, 160)
    for t, stride in ((base, 160), (base[:, :, :128], 160), (base[0], 160), (base[:, 0], 9 * 160), (base[:, :1], 9 * 160),
                      (torch.zeros(1, 128).expand(9, 128), 0)):
        got, s = _by_rows(t, t.shape[-1], zero_ok=True)
        assert got is t and s == stride, (t.shape, t.stride(), s)
    assert _by_rows(torch.zeros(1, 128).expand(9, 128), 128)[0].is_contiguous(), "an input row is not shared"
    for t in (base[:, :5], base.transpose(0, 1), base[..., ::2], base.transpose(1, 2)):
        got, s = _by_rows(t, t.shape[-1])
        assert got.is_contiguous() and s == t.shape[-1] and torch.equal(got, t), (t.shape, t.stride())


def test_the_library_refuses_bad_arguments_before_any_launch():
    """With fake pointers: a call that got as far as a launch would not come back with MGS_ERR_INVALID_ARG."""
    from manigaussian_amd import _lib
    L = _lib.lib()
    fake, INV, big = 0x10000, _lib.MGS_ERR_INVALID_ARG, 1 << 40

    def ln_fwd(rows=4, D=8, x=fake, xs=None, w=fake, b=fake, y=fake, stats=fake):
        return L.mgs_layernorm_forward(rows, D, x, D if xs is None else xs, w, b, 1e-5, y, stats, None)

    def ln_bwd(rows=4, D=8, x=fake, xs=None, w=fake, stats=fake, g=fake, gs=None, dx=fake, dw=fake, db=fake, ws=fake, wsb=big, split=0):
        return L.mgs_layernorm_backward(rows, D, x, D if xs is None else xs, w, stats, g, D if gs is None else gs, dx, dw, db, ws,
                                        wsb, split, None)

    def gg_fwd(rows=4, M=8, h=fake, hs=None, b=fake, out=fake):
        return L.mgs_bias_geglu_forward(rows, M, h, 2 * M if hs is None else hs, b, out, None)

    def gg_bwd(rows=4, M=8, h=fake, hs=None, b=fake, g=fake, gs=None, dh=fake, db=fake, ws=fake, wsb=big, split=0):
        return L.mgs_bias_geglu_backward(rows, M, h, 2 * M if hs is None else hs, b, g, M if gs is None else gs, dh, db, ws, wsb,
                                         split, None)

    for call in (ln_fwd, ln_bwd):
        for kw, word in ((dict(D=1025), "D = 1025"), (dict(D=0), "D = 0"), (dict(rows=0), "rows = 0"), (dict(rows=-1), "rows = -1"),
                         (dict(rows=1 << 21, D=1024), "2^31 - 1"), (dict(xs=7), "row stride"), (dict(x=None), "NULL"),
                         (dict(w=None), "NULL"), (dict(stats=None), "NULL"), (dict(x=fake + 2), "aligned")):
            assert call(**kw) == INV, (call.__name__, kw)
            assert word in _lib.last_error(), (call.__name__, kw, _lib.last_error())
    assert ln_fwd(b=None) == INV and ln_fwd(y=None) == INV and ln_fwd(y=fake + 4) == INV and "16-byte" in _lib.last_error()
    for call in (gg_fwd, gg_bwd):
        for kw, word in ((dict(M=0), "M = 0"), (dict(rows=0), "rows = 0"), (dict(rows=1 << 20, M=1 << 10), "2^31 - 1"),
                         (dict(rows=1, M=1 << 30), "2^31 - 1"), (dict(hs=15), "row stride"), (dict(h=None), "NULL"),
                         (dict(h=fake + 1), "aligned")):
            assert call(**kw) == INV, (call.__name__, kw)
            assert word in _lib.last_error(), (call.__name__, kw, _lib.last_error())
    assert gg_fwd(out=None) == INV and gg_fwd(out=fake + 8) == INV
    for call, need in ((ln_bwd, L.mgs_feedforward_workspace_bytes(4, 8)), (gg_bwd, L.mgs_feedforward_workspace_bytes(4, 8))):
        assert need > 0
        for kw, word in ((dict(g=None), "NULL"), (dict(gs=3), "row stride"), (dict(split=65), "row_split"), (dict(split=-1), "row_split"),
                         (dict(ws=None), "workspace"), (dict(ws=fake + 4), "workspace")):
            assert call(**kw) == INV, (call.__name__, kw)
            assert word in _lib.last_error(), (call.__name__, kw, _lib.last_error())
        assert call(wsb=need - 1) == _lib.MGS_ERR_WORKSPACE and "needed" in _lib.last_error()
        assert call(wsb=0) == _lib.MGS_ERR_WORKSPACE
    assert ln_bwd(dx=None) == INV and gg_bwd(dh=None) == INV and gg_bwd(dh=fake + 4) == INV


def test_the_workspace_size_covers_sixty_four_slabs_of_two_sums():
    from manigaussian_amd import _lib
    L = _lib.lib()
    for rows, cols in ((1, 1), (2048, 512), (8077, 128), (2048, 2048), (3, 1 << 20)):
        n = L.mgs_feedforward_workspace_bytes(rows, cols)
        assert 64 * 2 * cols * 4 <= n <= 64 * 2 * cols * 4 + 512 and n % 256 == 0, (rows, cols, n)
    assert L.mgs_feedforward_workspace_bytes(0, 8) == 0 and L.mgs_feedforward_workspace_bytes(8, 0) == 0
    assert L.mgs_feedforward_workspace_bytes(2048, 512) == L.mgs_feedforward_workspace_bytes(7, 512), "independent of the split"


def test_the_drop_ins_routing_follows_the_recorded_medians():
    """profiles/feedforward_bench.json is the record: an op is routed through its kernel only if ours is below torch's median,
    forward and forward + backward, at every use of it -- the bias-GEGLU also inside the whole block as it would then be routed."""
    import json
    from manigaussian_amd import feedforward
    with open(os.path.join(ROOT, "profiles", "feedforward_bench.json")) as f:
        rec = json.load(f)
    uses = rec["uses"]
    assert rec["build_id"] and set(uses) == {"ln_latents", "ln_sequence", "geglu_hidden", "block"}
    for e in uses.values():
        for side in (k for k in e if k in ("ours", "ours_geglu_only", "torch")):
            for what in ("forward_s", "forward_backward_s"):
                assert e[side][what]["runs"] >= 20 and e[side][what]["min"] <= e[side][what]["median"] <= e[side][what]["max"]

    def below(use, side="ours"):
        e = uses[use]
        return all(e[side][w]["median"] < e["torch"][w]["median"] for w in ("forward_s", "forward_backward_s"))

    ln = below("ln_latents") and below("ln_sequence")
    geglu = below("geglu_hidden") and below("block", "ours" if ln else "ours_geglu_only")
    assert feedforward.ROUTE == {"layer_norm": ln, "bias_geglu": geglu}, (feedforward.ROUTE, ln, geglu)


# ---- GPU -----------------------------------------------------------------------------------------------------------------------
def ours_ln(row_split=0):
    from manigaussian_amd import layer_norm
    return lambda x, w, b: layer_norm(x, w, b, fc.EPS, row_split=row_split)


def ours_geglu(row_split=0):
    from manigaussian_amd import bias_geglu
    return lambda h, b: bias_geglu(h, b, row_split=row_split)


def run_case(kind, case, row_split=0):
    t = fc.truth(kind, case)
    fn = ours_ln(row_split) if kind == "ln" else ours_geglu(row_split)
    return t, fc.run_op(fn, t["inputs"], t["g"], None, dev(), frozen=t["frozen"])


@gpu
@pytest.mark.parametrize("case", list(fc.LN_CASES))
def test_layer_norm_cases_forward_and_gradients(case):
    t, got = run_case("ln", case)
    assert got["out"].is_contiguous() and got["d0"].is_contiguous()
    check_results(f"layer_norm {case}", got, t, LN_NAMES)


@gpu
@pytest.mark.parametrize("case", list(fc.GEGLU_CASES))
def test_bias_geglu_cases_forward_and_gradients(case):
    t, got = run_case("geglu", case)
    assert got["out"].is_contiguous() and got["d0"].is_contiguous()
    check_results(f"bias_geglu {case}", got, t, GG_NAMES)
    if case == "saturated":
        h, b = (x.to(dev()) for x in t["inputs"])
        M = h.shape[1] // 2
        gate = h[:, M:] + b[M:]
        assert all(torch.isfinite(v).all() for v in got.values())
        low = gate <= -40
        assert low.any() and (got["d0"][:, M:][low] == 0).all(), "gelu'(t <= -40) is exactly 0"
        assert (got["out"][low] == 0).all()


@gpu
def test_views_are_read_in_place_and_equal_their_copies(monkeypatch):
    from manigaussian_amd import _lib
    seen = spy(_lib.lib(), FUSED_ENTRIES, monkeypatch)
    for kind, case, fn in (("ln", "strided", ours_ln()), ("geglu", "strided", ours_geglu()), ("ln", "expanded_g", ours_ln())):
        t = fc.truth(kind, case)
        seen.clear()
        a = fc.run_op(fn, t["inputs"], t["g"], None, dev())
        strides = {n: [x for x in v[0][2:8] if isinstance(x, int) and x < 4096] for n, v in seen.items()}
        if case == "strided":
            wide = (fc.LN_CASES if kind == "ln" else fc.GEGLU_CASES)[case]["wide"]
            assert all(wide in s for s in strides.values()), (kind, strides)   # the view's own row stride reached the library
        else:
            assert seen["mgs_layernorm_backward"][0][7] == 0, "the expanded gradient's row stride"
        b = fc.run_op(fn, [None if x is None else x.contiguous() for x in t["inputs"]], t["g"].contiguous(), None, dev())
        assert set(a) == set(b) and all(fc.same_bits(a[k], b[k]) for k in a), (kind, case)
    # a gradient expanded in both dimensions (sum().backward()) and a transposed input are copied, not misread
    from manigaussian_amd import layer_norm
    t = fc.truth("ln", "r65_d130")
    x, w, b = (v.to(dev()) for v in t["inputs"])
    xt = x.t().contiguous().t().requires_grad_(True)
    xc = x.clone().requires_grad_(True)
    layer_norm(xt, w, b).sum().backward()
    layer_norm(xc, w, b).backward(torch.ones(65, 130, device=dev()))
    assert fc.same_bits(xt.grad.contiguous(), xc.grad)


@gpu
def test_frozen_parameters_get_dx_alone_without_partial_sums(monkeypatch):
    from manigaussian_amd import _lib, bias_geglu
    calls = spy(_lib.lib(), ["mgs_layernorm_backward"], monkeypatch)["mgs_layernorm_backward"]
    t, got = run_case("ln", "frozen")
    assert set(got) == {"out", "d0"} and len(calls) == 1
    dw, db, ws, ws_bytes = calls[0][9:13]
    assert dw is None and db is None and ws is None and ws_bytes == 0, "NULL sums: the library issues the row launch alone"
    check_results("layer_norm frozen", got, t, LN_NAMES)
    # ... and one frozen parameter: the other's sum alone
    x, w, b = (v.to(dev()) for v in t["inputs"])
    calls.clear()
    free = fc.run_op(ours_ln(), [x, w, b], t["g"], None, dev(), frozen=(1,))
    assert set(free) == {"out", "d0", "d2"} and calls[0][9] is None and calls[0][10] is not None
    full = fc.run_op(ours_ln(), [x, w, b], t["g"], None, dev())
    assert fc.same_bits(free["d0"], full["d0"]) and fc.same_bits(free["d2"], full["d2"]) and fc.same_bits(free["d0"], got["d0"])
    # the GEGLU without a bias gradient
    gcalls = spy(_lib.lib(), ["mgs_bias_geglu_backward"], monkeypatch)["mgs_bias_geglu_backward"]
    tg = fc.truth("geglu", "r65_m130")
    a = fc.run_op(ours_geglu(), tg["inputs"], tg["g"], None, dev(), frozen=(1,))
    assert set(a) == {"out", "d0"} and gcalls[0][8] is None and gcalls[0][9] is None
    check("bias_geglu frozen dh", a["d0"], tg["r64"]["d0"], tg["ref_err"]["d0"])


@gpu
def test_layer_norm_exact_cases():
    from manigaussian_amd import layer_norm
    gen = torch.Generator().manual_seed(11)
    # D = 1: every row is its own mean
    x, w, b, g = (torch.randn(s, generator=gen).to(dev()) for s in ((37, 1), (1,), (1,), (37, 1)))
    r = fc.run_op(lambda *a: layer_norm(*a), [x, w, b], g, None, dev())
    assert fc.same_bits(r["out"], b.expand(37, 1).contiguous()), "out == bias bit for bit"
    assert (r["d0"] == 0).all() and (r["d1"] == 0).all()
    want = g.double().sum(0)
    check("D = 1 dbias", r["d2"], want, fc.rel_err(g.sum(0), want))
    # one row of a constant: the centred values are exactly zero
    x = torch.full((1, 128), 3.25, device=dev())
    w, b, g = (torch.randn(s, generator=gen).to(dev()) for s in ((128,), (128,), (1, 128)))
    r = fc.run_op(lambda *a: layer_norm(*a), [x, w, b], g, None, dev())
    assert fc.same_bits(r["out"], b.reshape(1, 128)), "out == bias bit for bit"
    gw = (g.double() * w.double())
    want = (gw - gw.mean()) / np.sqrt(1e-5)
    gw32 = g * w
    check("constant row dx", r["d0"], want, fc.rel_err((gw32 - gw32.mean()) * torch.rsqrt(torch.tensor(1e-5, device=dev())), want))


@gpu
def test_bias_geglu_with_a_zero_gate_is_exactly_zero():
    gen = torch.Generator().manual_seed(12)
    h = torch.randn(21, 2 * 37, generator=gen)
    h[:, 37:] = 0
    g = torch.randn(21, 37, generator=gen)
    for bias in (None, torch.cat([torch.randn(37, generator=gen), torch.zeros(37)])):
        r = fc.run_op(ours_geglu(), [h, bias], g, None, dev())
        assert (r["out"] == 0).all() and (r["d0"][:, :37] == 0).all()
        a = h[:, :37] if bias is None else h[:, :37] + bias[:37]
        want = g.double() * a.double() * 0.5    # gelu'(0) = Phi(0) = 1 / 2
        check("zero gate dh", r["d0"][:, 37:], want, 0.0)


@gpu
@pytest.mark.parametrize("kind,case", list(zip(("ln", "geglu"), fc.SPLIT_CASES)))
def test_the_row_split_changes_no_bit_of_dx_and_keeps_the_sums_within_the_bound(kind, case):
    names = LN_NAMES if kind == "ln" else GG_NAMES
    runs = {}
    for split in fc.SPLITS:
        t, runs[split] = run_case(kind, case, split)
        _, again = run_case(kind, case, split)
        assert all(fc.same_bits(runs[split][k], again[k]) for k in again), (kind, split, "two runs with one split")
        check_results(f"{kind} {case} row_split {split}", runs[split], t, names)
    for split in fc.SPLITS[1:]:
        for k in ("out", "d0"):
            assert fc.same_bits(runs[split][k], runs[fc.SPLITS[0]][k]), (kind, k, split)
    _, auto = run_case(kind, case, 0)
    assert fc.same_bits(auto["d0"], runs[1]["d0"])


def route(monkeypatch, kernels, watch=False):
    """The drop-ins' routing for this test: both ops through the kernels, or both through torch.  watch: returns the spy's record of the
    library's entries."""
    from manigaussian_amd import _lib, feedforward
    monkeypatch.setitem(feedforward.ROUTE, "layer_norm", kernels)
    monkeypatch.setitem(feedforward.ROUTE, "bias_geglu", kernels)
    return spy(_lib.lib(), FUSED_ENTRIES, monkeypatch) if watch else None


@gpu
@pytest.mark.parametrize("kernels", [True, False], ids=["kernels", "torch"])
@pytest.mark.parametrize("name", list(fc.MODULES))
def test_module_fixtures_on_the_device(name, kernels, monkeypatch):
    """Whatever the shipped routing: once with both ops through the kernels, once with both left to torch."""
    import manigaussian_amd
    calls = route(monkeypatch, kernels, watch=True)
    f = fc.load_module_fixture(name)
    m = fc.fixture_module(manigaussian_amd, name)
    got = fc.run_module(m, f["x"], f["g"], torch.float32, dev(), context=f.get("context"))
    check_module(name, fc.module_errors(f, *got), "device, kernels" if kernels else "device, torch")
    want = {"prenorm_ff": {"mgs_layernorm_forward": 1, "mgs_layernorm_backward": 1, "mgs_bias_geglu_forward": 1, "mgs_bias_geglu_backward": 1},
            "ff_odd": {"mgs_bias_geglu_forward": 1, "mgs_bias_geglu_backward": 1},
            "prenorm_context": {"mgs_layernorm_forward": 2, "mgs_layernorm_backward": 2}}[name]
    assert {k: len(v) for k, v in calls.items()} == (want if kernels else {}), (name, kernels, calls)


@gpu
def test_prenorm_around_the_fused_attention_against_float64_on_the_device(monkeypatch):
    import manigaussian_amd
    route(monkeypatch, True)
    torch.manual_seed(31)
    plain = manigaussian_amd.PreNorm(16, fc.PlainAttention(16, 8, 1, 64), context_dim=8)
    ours = manigaussian_amd.PreNorm(16, manigaussian_amd.Attention(16, context_dim=8, heads=1, dim_head=64), context_dim=8)
    gen = torch.Generator().manual_seed(32)
    with torch.no_grad():
        for k, v in sorted(plain.state_dict().items()):
            if k.startswith("norm"):
                v.copy_(torch.randn(v.shape, generator=gen) * 0.3 + (1.0 if k.endswith("weight") else 0.0))
    ours.load_state_dict(plain.state_dict(), strict=True)
    x, context, g = (torch.randn(s, generator=gen) for s in ((2, 7, 16), (2, 5, 8), (2, 7, 16)))
    import copy
    r64 = fc.run_module(copy.deepcopy(plain), x, g, torch.float64, dev(), context=context)   # (float64: torch's composition)
    r32 = fc.run_module(copy.deepcopy(plain), x, g, torch.float32, dev(), context=context)
    got = fc.run_module(ours, x, g, torch.float32, dev(), context=context)

    def flat(r):
        return {"out": r[0], "dx": r[1], "dcontext": r[3], **{"dp." + k: v for k, v in r[2].items()}}

    a, b, c = flat(got), flat(r32), flat(r64)
    for k in c:
        check(f"prenorm(attention) {k}", a[k], c[k], fc.rel_err(b[k], c[k]))


PRODUCTION = {"latents": ("ln", 2048, 512), "sequence": ("ln", 8077, 128), "hidden": ("geglu", 2048, 2048)}


@gpu
@pytest.mark.parametrize("name", list(PRODUCTION))
def test_production_shapes_against_float64_on_the_device(name):
    kind, rows, width = PRODUCTION[name]
    gen = torch.Generator(device=dev()).manual_seed(9000 + list(PRODUCTION).index(name))
    if kind == "ln":
        inputs = [torch.randn(s, device=dev(), generator=gen) for s in ((rows, width), (width,), (width,))]
        fn, theirs, names = ours_ln(), fc.ln_compose, LN_NAMES
    else:
        inputs = [torch.randn(s, device=dev(), generator=gen) for s in ((rows, 2 * width), (2 * width,))]
        fn, theirs, names = ours_geglu(), fc.geglu_compose, GG_NAMES
    g = torch.randn(rows, width, device=dev(), generator=gen)
    got = fc.run_op(fn, inputs, g, None, dev())
    again = fc.run_op(fn, inputs, g, None, dev())
    assert all(torch.equal(got[k], again[k]) for k in got), "two runs are bit-identical"
    r32 = fc.run_op(theirs, inputs, g, torch.float32, dev())
    r64 = fc.run_op(theirs, inputs, g, torch.float64, dev())
    for k, want in r64.items():
        check(f"{name} {names.get(k, k)}", got[k], want, fc.rel_err(r32[k], want))


@gpu
def test_the_library_refuses_on_the_device_and_launches_nothing():
    """Through the raw C ABI with real tensors: D = 1025 and a short workspace return their errors and leave the outputs alone."""
    from manigaussian_amd import _lib, _ops
    L = _lib.lib()
    x = torch.randn(4, 1025, device=dev())
    w = torch.ones(1025, device=dev())
    y = torch.full((4, 1025), 7.0, device=dev())
    stats = torch.full((4, 2), 7.0, device=dev())
    s = _ops.stream(dev())
    assert L.mgs_layernorm_forward(4, 1025, x.data_ptr(), 1025, w.data_ptr(), w.data_ptr(), 1e-5, y.data_ptr(), stats.data_ptr(), s) \
        == _lib.MGS_ERR_INVALID_ARG
    assert "D = 1025" in _lib.last_error()
    dx, dw = torch.full((4, 512), 7.0, device=dev()), torch.full((512,), 7.0, device=dev())
    ws = torch.zeros(1024, dtype=torch.uint8, device=dev())
    rc = L.mgs_layernorm_backward(4, 512, x.data_ptr(), 1025, w.data_ptr(), stats.data_ptr(), x.data_ptr(), 1025, dx.data_ptr(),
                                  dw.data_ptr(), dw.data_ptr(), ws.data_ptr(), ws.numel(), 0, s)
    assert rc == _lib.MGS_ERR_WORKSPACE and "needed" in _lib.last_error()
    dh, db = torch.full((4, 1024), 7.0, device=dev()), torch.full((1024,), 7.0, device=dev())
    rc = L.mgs_bias_geglu_backward(4, 512, x.data_ptr(), 1025, None, x.data_ptr(), 1025, dh.data_ptr(), db.data_ptr(), ws.data_ptr(),
                                   ws.numel(), 0, s)
    assert rc == _lib.MGS_ERR_WORKSPACE
    torch.cuda.synchronize()
    for t in (y, stats, dx, dw, dh, db):
        assert (t == 7.0).all(), "nothing was launched"
    with pytest.raises(RuntimeError, match=r"^layernorm_forward: .*\(code -1\)$"):
        _ops.call("mgs_layernorm_forward", dev(), 4, 1025, x.data_ptr(), 1025, w.data_ptr(), w.data_ptr(), 1e-5, y.data_ptr(),
                  stats.data_ptr())


@gpu
def test_forward_and_backward_captured_into_a_hip_graph():
    """In a child process: stream capture is process-wide state (tests/tools/feedforward_graph_capture_check.py)."""
    run_graph_tool("feedforward_graph_capture_check.py")
