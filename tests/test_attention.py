"""The fused attention (manigaussian_amd/attention.py, csrc/mgs_attention.hip) against ManiGaussian's own Attention class
(agents/manigaussian_bc/perceiver_lang_io.py:102-145).

The yardstick is the reference's own fp32 rounding error: a fixture (tests/golden/attention/, tests/attention_cases.py) holds
the reference module's float64 result -- the truth -- and, per tensor, how far the reference's float32 run lies from it
(ref_err).  Ours must lie within 16 x ref_err x max|truth| of the truth, for the output and every gradient.  The factor covers
another summation order (key tiles with rescaling against whole rows) and another exp; the smallest logic error (one dropped key
of 338) is two orders above it.  A truth that is identically zero (one_key: softmax of one element has no gradient towards
q) is bounded by 1e-5 of the largest magnitude among the case's other gradients.

With MGS_ATTENTION_PARITY_OUT=<file> the GPU tests append every measured error and its ratio to ref_err to that JSON file
(profiles/attention_parity.json is meant to be such a run; none has been recorded on an MI355X yet).
"""
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import attention_cases as ac
from child import run_graph_tool
from numerics import dev

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROPOUT_CASES = [c for c in ac.CASES if ac.CASES[c]["p"] > 0]
WIDE_SHAPE = (16, 8, 70, 130)  # B, H, Nq, Nk of wide_ragged: four waves per workgroup; one batch item of it: one wave
FULL = {"encoder_cross": (1, 2048, 8077), "latent_self": (8, 2048, 2048), "decoder_cross": (1, 8077, 2048)}  # H, Nq, Nk


def record(name, rows):
    path = os.environ.get("MGS_ATTENTION_PARITY_OUT")
    if not path:
        return
    data = {}
    if os.path.exists(path):
        with open(path) as f:
            data = json.load(f)
    from manigaussian_amd import _lib
    data["build_id"] = _lib.build_id()
    data[name] = rows
    with open(path, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not ac.have_reference(), reason="no copy of the reference on this machine")
def test_fixtures_match_the_reference():
    """The generator's computation, re-run.  Inputs bit for bit; the float64 truth to 1e-12 of its magnitude (the order of a CPU's
    sums may follow its thread count); ref_err, a maximum of float32 rounding errors, within a factor of two."""
    for case in ac.CASES:
        f, now = ac.load_fixture(case), ac.reference_case(case)
        for k, v in now.items():
            if k == "ref_err":
                for n, e in zip(ac.grad_names(case), v.tolist()):
                    c = f["ref_err"][n]
                    assert (e == 0 and c == 0) or 0.5 * c <= e <= 2 * c, (case, n, e, c)
            elif k.endswith("64"):
                t = torch.from_numpy(v)
                assert (t - f[k]).abs().max().item() <= 1e-12 * max(t.abs().max().item(), 1e-300), (case, k)
            else:
                assert np.array_equal(v, f[k].numpy()), (case, k)
        assert set(now) == set(f), case


def test_fixtures_are_small():
    for case in ac.CASES:
        assert os.path.getsize(ac.fixture_path(case)) <= 1_000_000, case
        with np.load(ac.fixture_path(case), allow_pickle=False) as z:
            assert all(z[k].dtype.kind in "fb" for k in z.files), case


def test_the_numpy_dropout_function_keeps_the_right_share():
    c = ac.CASES["dropout_p10"]
    BH, Nq, Nk, p = c["B"] * c["H"], c["Nq"], c["Nk"], c["p"]
    seed, offset = c["rng"]
    keep = ac.keep_mask(seed, offset, BH, Nq, Nk, p)
    n = keep.size
    assert n == 104_000
    sigma = math.sqrt(p * (1 - p) / n)
    assert abs(keep.mean() - (1 - p)) <= 5 * sigma, keep.mean()
    for s in range(BH):
        assert abs(keep[s].mean() - (1 - p)) <= 5 * math.sqrt(p * (1 - p) / keep[s].size), (s, keep[s].mean())
    other = ac.keep_mask(seed, offset + 1, BH, Nq, Nk, p)
    agree, q = (keep == other).mean(), (1 - p) ** 2 + p ** 2
    assert abs(agree - q) <= 5 * math.sqrt(q * (1 - q) / n), agree
    # a pure function: the element's decision does not depend on the extent of the array it is computed in
    assert np.array_equal(ac.keep_mask(seed, offset, BH, 7, 13, p), keep[:, :7, :13])


def _args(**kw):
    from manigaussian_amd import _lib
    fake = 0x10000
    H = kw.get("H", 2)
    a = _lib.MgsAttentionArgs()
    a.B, a.H, a.Nq, a.Nk, a.D, a.dropout_p = 1, H, 100, 200, 64, 0.0
    a.q = a.k = a.v = fake
    a.q_stride_n = a.out_stride_n = a.dout_stride_n = a.dq_stride_n = 64 * H
    a.k_stride_n = a.v_stride_n = a.dkv_stride_n = 128 * H
    a.q_stride_b = a.out_stride_b = a.dout_stride_b = a.dq_stride_b = 64 * H * 100
    a.k_stride_b = a.v_stride_b = a.dkv_stride_b = 128 * H * 200
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_the_library_refuses_bad_arguments_before_any_launch():
    from manigaussian_amd import _lib
    L = _lib.lib()
    fake = 0x10000
    INV = _lib.MGS_ERR_INVALID_ARG
    ws = L.mgs_attention_workspace_bytes(1, 2, 100, 200)
    for kw, word in ((dict(D=32), "head dimension 32"), (dict(Nk=0), "Nk = 0"), (dict(Nq=0), "Nq = 0"),
                     (dict(dropout_p=1.0), "outside [0, 1)"), (dict(dropout_p=-0.1), "outside [0, 1)"),
                     (dict(dropout_p=0.5), "rng_state"), (dict(q_stride_n=64), "row strides"), (dict(k_stride_n=127), "row strides"),
                     (dict(v_stride_n=130), "row strides"), (dict(q=fake + 4), "16-byte aligned"), (dict(v=fake + 8), "16-byte aligned"),
                     (dict(k=None), "NULL"), (dict(mask=fake, mask_stride_b=100), "mask stride")):
        a = _args(**kw)
        assert L.mgs_attention_forward(ctypes.byref(a), fake, fake, None) == INV, kw
        assert word in _lib.last_error(), (kw, _lib.last_error())
        assert L.mgs_attention_backward(ctypes.byref(a), fake, fake, fake, fake, fake, fake, ws, None) == INV, kw
        assert word in _lib.last_error(), (kw, _lib.last_error())
    a = _args()
    assert L.mgs_attention_forward(ctypes.byref(a), fake + 4, fake, None) == INV and "16-byte aligned" in _lib.last_error()
    assert L.mgs_attention_forward(ctypes.byref(_args(out_stride_n=64)), fake, fake, None) == INV
    assert L.mgs_attention_backward(ctypes.byref(a), fake, fake, fake, fake + 4, fake, fake, ws, None) == INV
    assert L.mgs_attention_backward(ctypes.byref(_args(dkv_stride_n=128)), fake, fake, fake, fake, fake, fake, ws, None) == INV
    assert "dkv" in _lib.last_error()
    assert L.mgs_attention_backward(ctypes.byref(a), fake, fake, fake, fake, fake, fake, ws - 1, None) == _lib.MGS_ERR_WORKSPACE
    assert "needed" in _lib.last_error()
    assert L.mgs_attention_dropout_mask(ctypes.byref(_args(dropout_p=0.5)), fake, None) == INV
    # B H Nq Nk is no limit: sizes whose score matrix would hold 2^44 elements pass the checks (refused here for the stride only)
    big = _args(B=4, Nq=1 << 21, Nk=1 << 21, q_stride_n=64)
    assert L.mgs_attention_forward(ctypes.byref(big), fake, fake, None) == INV and "row strides" in _lib.last_error()


def test_the_library_refuses_more_than_65535_batch_heads():
    """B H is the grid's y extent.  65536 is refused by every entry point; 65535 passes that check (and is refused by the next
    one, for the dropout without a state, before any launch)."""
    from manigaussian_amd import _lib
    L = _lib.lib()
    fake = 0x10000
    INV = _lib.MGS_ERR_INVALID_ARG

    def calls(a):
        ws = 1 << 40
        yield "forward", L.mgs_attention_forward(ctypes.byref(a), fake, fake, None)
        yield "backward", L.mgs_attention_backward(ctypes.byref(a), fake, fake, fake, fake, fake, fake, ws, None)
        yield "dropout_mask", L.mgs_attention_dropout_mask(ctypes.byref(a), fake, None)

    def args(B, H, **kw):
        return _args(H=H, B=B, **kw)

    for B, H in ((65536, 1), (1, 65536), (256, 256)):
        for p in (0.0, 0.5):
            a = args(B, H, dropout_p=p)
            for name, rc in calls(a):
                assert rc == INV and "B H <= 65535" in _lib.last_error(), (B, H, p, name, rc, _lib.last_error())
    for B, H in ((65535, 1), (1, 65535), (255, 257)):
        a = args(B, H, dropout_p=0.5)
        for name, rc in calls(a):
            assert rc == INV and "rng_state" in _lib.last_error() and "65535" not in _lib.last_error(), \
                (B, H, name, rc, _lib.last_error())


def _kernel_constants():
    with open(os.path.join(ROOT, "manigaussian_amd", "csrc", "mgs_attention.hip")) as f:
        src = f.read()
    found = dict(re.findall(r"^constexpr int (ATT_\w+) = (\d+);", src, flags=re.M))
    return {k: int(found[k]) for k in ("ATT_CUS", "ATT_T", "ATT_WQ")}


def launch_form(B, H, rows):
    """mgs_attention.hip's wide(): four waves per workgroup once B H ceil(rows / (4 ATT_WQ)) reaches ATT_CUS workgroups; rows
    is Nq for the forward and dQ, Nk for dK/dV."""
    k = _kernel_constants()
    per_wg = 4 * k["ATT_WQ"]
    return "wide" if B * H * ((rows + per_wg - 1) // per_wg) >= k["ATT_CUS"] else "narrow"


def test_the_wide_cases_reach_the_four_wave_form():
    """The premise of the cases appended for the 256-thread form, pinned: a change of the launch rule fails here instead of
    quietly turning them into one-wave runs."""
    k = _kernel_constants()
    assert k["ATT_T"] == 4 * k["ATT_WQ"] == 64, "the cases' tile edges (64, 128) and ragged ends assume 64-row tiles"
    assert set(ac.LAUNCH_FORMS) == set(list(ac.CASES)[10:])
    for case, (fwd, dkv) in ac.LAUNCH_FORMS.items():
        c = ac.CASES[case]
        assert launch_form(c["B"], c["H"], c["Nq"]) == fwd, (case, "forward and dQ")
        assert launch_form(c["B"], c["H"], c["Nk"]) == dkv, (case, "dK/dV")
    assert all(launch_form(c["B"], c["H"], max(c["Nq"], c["Nk"])) == "narrow" for c in list(ac.CASES.values())[:10])
    # wide_ragged's last workgroups: 6 live queries and 2 live keys in wave 0, none in waves 1 to 3
    c = ac.CASES["wide_ragged"]
    assert c["Nq"] % 64 == 6 and c["Nk"] % 64 == 2
    # test_four_wave_and_one_wave_launches_give_the_same_bits: the batch is wide in both directions, one item of it is not
    B, H, Nq, Nk = WIDE_SHAPE
    assert launch_form(B, H, Nq) == launch_form(B, H, Nk) == "wide"
    assert launch_form(1, H, Nq) == launch_form(1, H, Nk) == "narrow"
    # the masks are what the cases' names say: whole 64-key tiles
    m = ac.case_mask("first_tiles_masked")
    assert not m[0, :64].any() and m[0, 64:].all() and not m[1, :128].any() and m[1, 128:].all()
    m = ac.case_mask("last_tiles_masked")
    assert m[0, :64].all() and not m[0, 64:].any() and m[1].nonzero().flatten().tolist() == [129]
    m = ac.case_mask("all_masked_dropout")
    assert m[0].sum() == 120 and not m[1].any()
    m = ac.case_mask("wide_masked_dropout")
    assert not m[0, :64].any() and m[0, 64:].all() and m[1, :64].all() and not m[1, 64:].any() and not m[2].any()
    assert m[3].tolist() == [j % 3 != 0 for j in range(130)] and torch.equal(m[:4], m[12:])


def test_the_workspace_size_is_monotone_and_aligned():
    from manigaussian_amd import _lib
    W = _lib.lib().mgs_attention_workspace_bytes
    base = W(1, 8, 2048, 2048)
    assert base >= 4 * 8 * 2048 and base % 256 == 0
    assert base < 1 << 20, "the backward's scratch is B H Nq floats, not a score matrix"
    for lo, hi in (((1, 8, 2048, 2048), (2, 8, 2048, 2048)), ((1, 1, 2048, 8077), (1, 8, 2048, 8077)),
                   ((1, 1, 2048, 2048), (1, 1, 8077, 2048))):
        assert 0 < W(*lo) < W(*hi) and W(*hi) % 256 == 0, (lo, hi)
    assert W(1, 1, 2048, 2048) <= W(1, 1, 2048, 8077)
    assert W(0, 1, 1, 1) == 0 and W(1, 0, 1, 1) == 0 and W(1, 1, 0, 1) == 0 and W(1, 1, 1, 0) == 0


def test_attention_refuses_cpu_tensors_and_other_head_sizes_and_loads_a_reference_state_dict():
    from manigaussian_amd import Attention, fused_attention
    with pytest.raises(ValueError, match="dim_head = 32"):
        Attention(16, heads=2, dim_head=32)
    m = Attention(16, context_dim=24, heads=2, dim_head=64, dropout=0.1)
    assert sorted(m.state_dict()) == sorted(ac.PARAMS), "rng_state must not be part of the state"
    _, _, _, _, params = ac.make_inputs("cross_enc")
    ref_shaped = Attention(24, context_dim=40, heads=1)
    ref_shaped.load_state_dict(params, strict=True)
    assert all(torch.equal(ref_shaped.state_dict()[k], v) for k, v in params.items())
    if ac.have_reference():
        ref = ac.load_reference().Attention(24, context_dim=40, heads=1)
        ref.load_state_dict(ref_shaped.state_dict(), strict=True)  # ... and the other way round
        ref_shaped.load_state_dict(ref.state_dict(), strict=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(torch.zeros(1, 5, 16), context=torch.zeros(1, 7, 24))
    with pytest.raises(RuntimeError, match="no CPU path"):
        fused_attention(torch.zeros(1, 5, 128), torch.zeros(1, 7, 128), torch.zeros(1, 7, 128), 2)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
def build_module(case, dropout=None):
    from manigaussian_amd import Attention
    c = ac.CASES[case]
    f = ac.load_fixture(case)
    m = Attention(c["qd"], context_dim=c["cd"], heads=c["H"], dim_head=64, dropout=c["p"] if dropout is None else dropout)
    m.load_state_dict({n: f[n] for n in ac.PARAMS}, strict=True)
    m = m.to(dev()).train()
    if c["p"] > 0:
        m.manual_seed(*c["rng"])
    return m


def run_case(case, m=None):
    """{tensor name: fp32 tensor on the CPU} of forward + backward of `case` through Attention."""
    c = ac.CASES[case]
    f = ac.load_fixture(case)
    m = build_module(case) if m is None else m
    m.zero_grad(set_to_none=True)
    if c["p"] > 0:
        m.manual_seed(*c["rng"])
    x = f["x"].to(dev()).requires_grad_(True)
    context = f["context"].to(dev()).requires_grad_(True) if "context" in f else None
    mask = f["mask"].to(dev()) if "mask" in f else None
    out = m(x, context=context, mask=mask)
    out.backward(f["grad"].to(dev()))
    res = {"out": out.detach().cpu(), "dx": x.grad.cpu()}
    if context is not None:
        res["dcontext"] = context.grad.cpu()
    for n, p in m.named_parameters():
        res["d" + n] = p.grad.cpu()
    return res


@gpu
@pytest.mark.parametrize("case", list(ac.CASES))
def test_every_fixture_forward_and_backward(case):
    f = ac.load_fixture(case)
    got = run_case(case)
    rows, bad = {}, []
    for n, (bound, mag, ref_err) in ac.bounds(case).items():
        err = (got[n].double() - f[n + "64"]).abs().max().item()
        rows[n] = dict(err=err, bound=bound, max_truth=mag, ref_err=ref_err,
                       ratio_to_ref_err=(err / (ref_err * mag) if ref_err * mag > 0 else None))
        print(f"{case} {n}: err {err:.3e} bound {bound:.3e} ({rows[n]['ratio_to_ref_err']} x ref_err)")
        if not err <= bound:
            bad.append((n, err, bound))
    record("fixture/" + case, rows)
    assert not bad, (case, bad)
    # the reference's edge case: a row whose keys are all masked attends uniformly; without dropout it is the mean of v
    dead = [] if "mask" not in f else [b for b in range(f["mask"].size(0)) if not f["mask"][b].any()]
    assert dead == {"masked": [1], "wide_masked_dropout": [2, 6, 10, 14], "all_masked_dropout": [1]}.get(case, [])
    if dead:
        m = build_module(case).eval()  # (eval: no dropout)
        with torch.no_grad():
            out = m(f["x"].to(dev()), context=f["context"].to(dev()), mask=f["mask"].to(dev())).cpu()
            v = m.to_kv(f["context"].to(dev())).chunk(2, dim=-1)[1]
            exp = m.to_out(v.mean(1, keepdim=True)).expand(-1, ac.CASES[case]["Nq"], -1).cpu()
        for b in dead:
            d, lim = (out[b] - exp[b]).abs().max().item(), 1e-6 * exp[b].abs().max().item() + 1e-7
            print(f"{case} item {b}, all keys masked: |out - to_out(mean v)| {d:.3e}, allowed {lim:.3e}")
            assert d <= lim, (case, b, d, lim)


@gpu
@pytest.mark.parametrize("shape", DROPOUT_CASES + ["tiles"])
def test_the_kernels_keep_mask_is_the_numpy_function(shape):
    from manigaussian_amd.attention import dropout_keep_mask
    if shape == "tiles":
        B, H, Nq, Nk, p, rng = 1, 3, 150, 333, 0.25, (0xFEDCBA9876543210, 0xABCDEF0123456789)
    else:
        c = ac.CASES[shape]
        B, H, Nq, Nk, p, rng = c["B"], c["H"], c["Nq"], c["Nk"], c["p"], c["rng"]
    from manigaussian_amd.attention import _as_int64
    state = torch.tensor([_as_int64(rng[0]), _as_int64(rng[1])], dtype=torch.int64, device=dev())
    got = dropout_keep_mask(B, H, Nq, Nk, p, state).cpu().numpy().astype(bool)
    exp = ac.keep_mask(rng[0], rng[1], B * H, Nq, Nk, p)
    assert got.shape == exp.shape and int((got != exp).sum()) == 0


def _qkv(B, H, Nq, Nk, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, Nq, H * 64, generator=g)
    kv = torch.randn(B, Nk, 2 * H * 64, generator=g)
    return q.to(dev()), kv.to(dev()), torch.randn(B, Nq, H * 64, generator=g).to(dev())


@gpu
@pytest.mark.parametrize("p", [0.0, 0.2])
def test_strided_inputs_equal_contiguous_copies_bit_for_bit(p):
    from manigaussian_amd import fused_attention
    B, H, Nq, Nk = 2, 2, 70, 150
    q, kv, g = _qkv(B, H, Nq, Nk, 3)
    state = torch.tensor([11, 5], dtype=torch.int64, device=dev()) if p else None
    wide = torch.zeros(B, Nq, H * 64 + 64, device=dev())
    wide[..., 32:32 + H * 64] = q

    def run(q_, k_, v_):
        q_, k_, v_ = (t.detach().requires_grad_(True) for t in (q_, k_, v_))
        out = fused_attention(q_, k_, v_, H, dropout_p=p, rng_state=state)
        out.backward(g)
        return out.detach(), q_.grad, k_.grad, v_.grad

    k, v = kv.chunk(2, dim=-1)
    assert not k.is_contiguous() and not v.is_contiguous()
    base = run(q, k.contiguous(), v.contiguous())
    for other in (run(q, k, v), run(wide[..., 32:32 + H * 64], k, v)):
        for a, b in zip(base, other):
            assert ac.same_bits(a.cpu(), b.cpu())
    # the packed form of the module: one gradient for the to_kv output, the halves of which are the ones above
    from manigaussian_amd.attention import fused_attention_kv
    q_, kv_ = q.detach().requires_grad_(True), kv.detach().requires_grad_(True)
    out = fused_attention_kv(q_, kv_, H, dropout_p=p, rng_state=state)
    out.backward(g)
    assert kv_.grad.is_contiguous() and ac.same_bits(out.detach().cpu(), base[0].cpu())
    assert ac.same_bits(kv_.grad.cpu(), torch.cat([base[2], base[3]], dim=-1).cpu())


def _run_qkv(q_, k_, v_, H, g, p=0.0, state=None, mask=None, backward=None):
    """out and the gradients of q, k, v, which are taken as they are laid out (detach keeps strides and offset)."""
    from manigaussian_amd import fused_attention
    q_, k_, v_ = (t.detach().requires_grad_(True) for t in (q_, k_, v_))
    out = fused_attention(q_, k_, v_, H, mask=mask, dropout_p=p, rng_state=state)
    if backward is None:
        out.backward(g)
    else:
        backward(out)
    return out.detach(), q_.grad, k_.grad, v_.grad


def _assert_same(base, other, what):
    for n, a, b in zip(("out", "dq", "dk", "dv"), base, other):
        assert a.shape == b.shape and ac.same_bits(a.cpu(), b.cpu()), (what, n)


def _odd_layouts(t):
    """t [B,N,W] in layouts the library does not read in place: base not 16-byte aligned; row stride no multiple of 4 floats."""
    B, N, W = t.shape
    off = torch.zeros(B, N, W + 4, device=t.device)
    off[..., 1:1 + W] = t
    odd = torch.zeros(B, N, W + 2, device=t.device)
    odd[..., :W] = t
    views = {"misaligned": off[..., 1:1 + W], "odd_row_stride": odd[..., :W]}
    assert views["misaligned"].data_ptr() % 16 == 4 and views["odd_row_stride"].stride(1) % 4 == 2
    assert all(torch.equal(v, t) and v.stride(2) == 1 for v in views.values())
    return views


@gpu
@pytest.mark.parametrize("p", [0.0, 0.2])
def test_layouts_the_library_refuses_are_copied_and_equal_contiguous_copies_bit_for_bit(p):
    """fused_attention / fused_attention_kv take any layout with a unit last stride; where mgs_attention_forward / _backward
    would refuse it (base not 16-byte aligned, row stride no multiple of 4 or shorter than the row) the wrapper copies."""
    from manigaussian_amd.attention import fused_attention_kv
    B, H, Nq, Nk = 2, 2, 70, 150
    HD = H * 64
    q, kv, g = _qkv(B, H, Nq, Nk, 3)
    state = torch.tensor([11, 5], dtype=torch.int64, device=dev()) if p else None
    k, v = (t.contiguous() for t in kv.chunk(2, dim=-1))
    base = _run_qkv(q, k, v, H, g, p, state)
    for name, view in _odd_layouts(q).items():
        _assert_same(base, _run_qkv(view, k, v, H, g, p, state), "q " + name)
    for (name, kview), vview in zip(_odd_layouts(k).items(), _odd_layouts(v).values()):
        _assert_same(base, _run_qkv(q, kview, vview, H, g, p, state), "k and v " + name)
        _assert_same(base, _run_qkv(q, kview, v, H, g, p, state), "k " + name)
        _assert_same(base, _run_qkv(q, k, vview, H, g, p, state), "v " + name)
    # q expanded over the batch (batch stride 0) and over the rows (row stride 0); the gradient has q's shape
    for name, src in (("batch", q[:1]), ("rows", q[:, :1])):
        view = src.expand(B, Nq, HD)
        assert view.stride(0 if name == "batch" else 1) == 0
        _assert_same(_run_qkv(view.contiguous(), k, v, H, g, p, state), _run_qkv(view, k, v, H, g, p, state),
                     "q expanded over the " + name)
    # upstream gradients of row stride 0: what out.sum(1).backward(g2) sends, strides (HD, 0, 1), and (0, 0, 1)
    g2 = g[:, 0].contiguous()
    seen = []

    def summed(out):
        out.register_hook(lambda d: seen.append(d.stride()))
        out.sum(1).backward(g2)

    _assert_same(_run_qkv(q, k, v, H, g2[:, None].expand(B, Nq, HD).contiguous(), p, state),
                 _run_qkv(q, k, v, H, None, p, state, backward=summed), "d_out from sum(1)")
    assert seen == [(HD, 0, 1)], seen
    g1 = g[0, 0].contiguous()
    _assert_same(_run_qkv(q, k, v, H, g1.expand(B, Nq, HD).contiguous(), p, state),
                 _run_qkv(q, k, v, H, g1.expand(B, Nq, HD), p, state), "d_out of strides (0, 0, 1)")
    # the packed form with kv as a misaligned slice of a wider buffer
    for name, view in _odd_layouts(kv).items():
        q_, kv_ = q.detach().requires_grad_(True), view.detach().requires_grad_(True)
        out = fused_attention_kv(q_, kv_, H, dropout_p=p, rng_state=state)
        out.backward(g)
        assert kv_.grad.shape == kv.shape
        _assert_same(base, (out.detach(), q_.grad, kv_.grad[..., :HD], kv_.grad[..., HD:]), "kv " + name)


@gpu
def test_layouts_the_library_accepts_are_not_copied(monkeypatch):
    """The aligned column slice and the chunk halves of test_strided_inputs_..., the packed kv, a batch-expanded q and a
    contiguous gradient reach the library where they lie: the wrapper's copy is never taken, forward or backward."""
    from manigaussian_amd import attention
    B, H, Nq, Nk = 2, 2, 70, 150
    HD = H * 64
    q, kv, g = _qkv(B, H, Nq, Nk, 3)
    wide = torch.zeros(B, Nq, HD + 64, device=dev())
    wide[..., 32:32 + HD] = q
    k, v = kv.chunk(2, dim=-1)
    base = _run_qkv(q, k.contiguous(), v.contiguous(), H, g)
    copies = []
    real = attention._copy

    def probe(t):
        copies.append((tuple(t.shape), t.stride()))
        return real(t)

    monkeypatch.setattr(attention, "_copy", probe)
    _assert_same(base, _run_qkv(wide[..., 32:32 + HD], k, v, H, g), "aligned slice, chunk halves")
    _assert_same(_run_qkv(q[:1].expand(B, Nq, HD).contiguous(), k, v, H, g), _run_qkv(q[:1].expand(B, Nq, HD), k, v, H, g),
                 "q expanded over the batch")
    q_, kv_ = q.detach().requires_grad_(True), kv.detach().requires_grad_(True)
    out = attention.fused_attention_kv(q_, kv_, H)
    out.backward(g)
    _assert_same(base, (out.detach(), q_.grad, kv_.grad[..., :HD], kv_.grad[..., HD:]), "packed kv")
    assert copies == [], copies
    _run_qkv(wide[..., 1:1 + HD], k, v, H, g)
    assert copies == [((B, Nq, HD), (Nq * (HD + 64), HD + 64, 1))], "(the probe sees a copy when there is one)"


def _wide_mask():
    B, H, Nq, Nk = WIDE_SHAPE
    return ac.mask_pattern("b_mod_4", B, Nk).to(dev())


@gpu
@pytest.mark.parametrize("masked", [False, True])
def test_four_wave_and_one_wave_launches_give_the_same_bits(masked):
    """"a wave's arithmetic does not depend on its workgroup".  The batch of 16 is launched with four waves per
    workgroup (256 and 384 workgroups), one item of it with one wave (test_the_wide_cases_reach_the_four_wave_form); p = 0,
    because the dropout's counter holds b H + h."""
    from manigaussian_amd.attention import fused_attention_kv
    B, H, Nq, Nk = WIDE_SHAPE
    q, kv, g = _qkv(B, H, Nq, Nk, 29)
    mask = _wide_mask() if masked else None

    def run(sl):
        q_, kv_ = q[sl].detach().requires_grad_(True), kv[sl].detach().requires_grad_(True)
        out = fused_attention_kv(q_, kv_, H, mask=None if mask is None else mask[sl])
        out.backward(g[sl])
        return out.detach().cpu(), q_.grad.cpu(), kv_.grad.cpu()

    whole = run(slice(None))
    for t in whole:
        assert bool(torch.isfinite(t).all())
    for b in (0, 5, 10, 15):
        for n, w, o in zip(("out", "dq", "dkv"), whole, run(slice(b, b + 1))):
            assert ac.same_bits(w[b:b + 1], o), (b, n)


@gpu
def test_every_form_of_the_mask_gives_the_same_bits():
    """_check's paths: a mask of another type (non-zero: live), of shape [B,1,Nk], and a non-contiguous column slice."""
    from manigaussian_amd.attention import fused_attention_kv
    c, f = ac.CASES["masked"], ac.load_fixture("masked")
    B, H, Nq, Nk = c["B"], c["H"], c["Nq"], c["Nk"]
    q, kv, g = _qkv(B, H, Nq, Nk, 31)
    mask = f["mask"].to(dev())
    assert mask.dtype == torch.bool and mask.shape == (B, Nk)

    def run(m):
        q_, kv_ = q.detach().requires_grad_(True), kv.detach().requires_grad_(True)
        out = fused_attention_kv(q_, kv_, H, mask=m)
        out.backward(g)
        return out.detach().cpu(), q_.grad.cpu(), kv_.grad.cpu()

    base = run(mask)
    assert not ac.same_bits(base[0], run(None)[0]), "the mask must matter"
    wider = torch.ones(B, Nk + 7, dtype=torch.bool, device=dev())
    wider[:, 3:3 + Nk] = mask
    sliced = wider[:, 3:3 + Nk]
    assert not sliced.is_contiguous()
    forms = {"uint8": mask.to(torch.uint8), "int64": mask.to(torch.int64) * 3, "float32": mask.to(torch.float32),
             "bool [B,1,Nk]": mask[:, None, :], "column slice": sliced, "uint8 [B,1,Nk] column slice": sliced[:, None, :].to(torch.uint8)}
    for name, m in forms.items():
        for n, a, b in zip(("out", "dq", "dkv"), base, run(m)):
            assert ac.same_bits(a, b), (name, n)


@gpu
@pytest.mark.parametrize("case", ["self_h8", "dropout_p10"])
def test_two_runs_are_bit_identical(case):
    m = build_module(case)
    a, b = run_case(case, m), run_case(case, m)
    for n in a:
        assert ac.same_bits(a[n], b[n]), (case, n)


@gpu
def test_eval_mode_ignores_dropout():
    f = ac.load_fixture("dropout_p10")
    x, context = f["x"].to(dev()), f["context"].to(dev())
    with_p, without = build_module("dropout_p10", dropout=0.1).eval(), build_module("dropout_p10", dropout=0.0).eval()
    before = with_p.rng_state.clone()
    a, b = with_p(x, context=context), without(x, context=context)
    assert ac.same_bits(a.detach().cpu(), b.detach().cpu())
    assert torch.equal(before, with_p.rng_state), "eval() must not draw"
    assert not ac.same_bits(with_p.train()(x, context=context).detach().cpu(), b.detach().cpu())
    assert int(with_p.rng_state[1] - before[1]) == 1, "a training forward advances the offset by one"


@gpu
def test_return_attention_weights_is_the_softmax_matrix():
    c, f = ac.CASES["masked"], ac.load_fixture("masked")
    m = build_module("masked")
    w = m(f["x"].to(dev()), context=f["context"].to(dev()), mask=f["mask"].to(dev()), return_attention_weights=True)
    assert w.shape == (c["B"] * c["H"], c["Nq"], c["Nk"])
    assert (w.sum(-1) - 1).abs().max().item() < 1e-5
    assert w[:c["H"], :, 10:40].abs().max().item() == 0 and (w[c["H"]:] - 1 / c["Nk"]).abs().max().item() < 1e-7


def torch_sequence(q, kv, g, H, dtype, max_bytes=1 << 30):
    """The reference's operations written with torch calls, in `dtype`, query rows in chunks so that no score matrix above
    max_bytes exists -> out, dq, dkv (in dtype, on the device)."""
    q = q.detach().to(dtype).requires_grad_(True)
    kv = kv.detach().to(dtype).requires_grad_(True)
    B, Nq, Nk = q.size(0), q.size(1), kv.size(1)
    rows = max(1, min(Nq, max_bytes // (B * H * Nk * torch.empty(0, dtype=dtype).element_size())))
    outs = []
    for s in range(0, Nq, rows):
        k, v = (t.reshape(B, Nk, H, 64).transpose(1, 2) for t in kv.chunk(2, dim=-1))
        qc = q[:, s:s + rows].reshape(B, -1, H, 64).transpose(1, 2)
        attn = (torch.einsum("bhid,bhjd->bhij", qc, k) * 64 ** -0.5).softmax(dim=-1)
        o = torch.einsum("bhij,bhjd->bhid", attn, v).transpose(1, 2).reshape(B, -1, H * 64)
        o.backward(g[:, s:s + rows].to(dtype))
        outs.append(o.detach())
    return torch.cat(outs, dim=1), q.grad, kv.grad


@gpu
@pytest.mark.parametrize("name", list(FULL))
def test_full_size_against_float64(name):
    from manigaussian_amd.attention import fused_attention_kv
    H, Nq, Nk = FULL[name]
    q, kv, g = _qkv(1, H, Nq, Nk, 17)
    truth = torch_sequence(q, kv, g, H, torch.float64)
    seq = torch_sequence(q, kv, g, H, torch.float32)
    q_, kv_ = q.detach().requires_grad_(True), kv.detach().requires_grad_(True)
    out = fused_attention_kv(q_, kv_, H)
    out.backward(g)
    ours = (out.detach(), q_.grad, kv_.grad)
    HD = H * 64
    rows, bad = {}, []
    for n, t, s, o in zip(("out", "dq", "dkv"), truth, seq, ours):
        parts = (("dk", slice(0, HD)), ("dv", slice(HD, 2 * HD))) if n == "dkv" else ((n, slice(None)),)
        for pn, sl in parts:
            ref_err = (s[..., sl].double() - t[..., sl]).abs().max().item()
            err = (o[..., sl].double() - t[..., sl]).abs().max().item()
            rows[pn] = dict(err=err, torch_fp32_err=ref_err, ratio=err / ref_err, max_truth=t[..., sl].abs().max().item())
            print(f"{name} {pn}: err {err:.3e}, the fp32 torch sequence {ref_err:.3e}")
            if not err <= ac.FACTOR * ref_err:
                bad.append((pn, err, ref_err))
    record("full/" + name, rows)
    assert not bad, (name, bad)


@gpu
def test_forward_and_backward_never_hold_a_score_matrix():
    from manigaussian_amd.attention import fused_attention_kv
    H, Nq, Nk = FULL["latent_self"]
    q, kv, g = _qkv(1, H, Nq, Nk, 5)

    def step():
        q_, kv_ = q.detach().requires_grad_(True), kv.detach().requires_grad_(True)
        fused_attention_kv(q_, kv_, H).backward(g)

    step()  # (the cached workspace of the backward exists from here on)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    step()
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    print(f"forward + backward of the latent self-attention: {extra / 1e6:.1f} MB beyond its inputs")
    record("memory/latent_self", dict(extra_bytes=extra, score_matrix_bytes=H * Nq * Nk * 4))
    assert extra < H * Nq * Nk * 4, extra


@gpu
def test_forward_and_backward_captured_into_a_hip_graph():
    """In a child process: stream capture is process-wide state (tests/tools/attention_graph_capture_check.py)."""
    run_graph_tool("attention_graph_capture_check.py")
