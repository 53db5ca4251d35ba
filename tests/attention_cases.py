"""Cases, fixtures and restatements shared by tests/test_attention.py, tests/golden/make_golden_attention.py and
tests/tools/attention_graph_capture_check.py -- TEST INFRASTRUCTURE.

A fixture (tests/golden/attention/<case>.npz, arrays only) holds what ManiGaussian's own Attention class
(agents/manigaussian_bc/perceiver_lang_io.py:102-145, executed unmodified on a CPU) was given and gave:
  x, context (absent: self-attention), mask (absent: none), the four parameters and the upstream gradient, float32;
  the float64 module's output and gradients (out64, dx64, dcontext64, dto_q.weight64, ...): the truth;
  ref_err: per tensor, the float32 module's own largest deviation from the truth over the truth's largest magnitude -- the
  yardstick of the tolerance (16 x ref_err x max|truth|), in the order of grad_names(case).
The dropout cases replace the reference module's `dropout` SUBMODULE INSTANCE by one that multiplies by keep / (1 - p), keep
being keep_mask() below: the numpy statement of the library's dropout function (DESIGN.md "Attention").
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

from numerics import same_bits  # noqa: F401  (re-exported: the tests and the tools reach them through this module)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden", "attention")
REF_FILE = os.path.join(os.environ.get("MGS_REFERENCE_ROOT", "/root/reference"), "agents", "manigaussian_bc",
                        "perceiver_lang_io.py")
DIM_HEAD = 64
PARAMS = ("to_q.weight", "to_kv.weight", "to_out.weight", "to_out.bias")
FACTOR = 16.0          # tolerance = FACTOR x ref_err x max|truth|
ZERO_BOUND = 1e-5      # a truth that is identically zero: this times the largest magnitude among the case's other gradients

# name: B, H, Nq, Nk, query_dim, context_dim (None: self-attention, context = x), input scale, dropout p, mask, (seed, offset)
CASES = {
    "self_h8":            dict(B=2, H=8, Nq=200, Nk=200, qd=16, cd=None, scale=1.0, p=0.0, mask=None),
    "cross_enc":          dict(B=1, H=1, Nq=130, Nk=338, qd=24, cd=40, scale=1.0, p=0.0, mask=None),
    "cross_dec":          dict(B=1, H=1, Nq=338, Nk=96, qd=40, cd=24, scale=1.0, p=0.0, mask=None),
    "one_key":            dict(B=1, H=2, Nq=5, Nk=1, qd=16, cd=16, scale=1.0, p=0.0, mask=None),
    "one_query":          dict(B=1, H=2, Nq=1, Nk=70, qd=16, cd=16, scale=1.0, p=0.0, mask=None),
    "exact_tiles":        dict(B=1, H=2, Nq=256, Nk=512, qd=16, cd=16, scale=1.0, p=0.0, mask=None),
    "large_logits":       dict(B=2, H=8, Nq=200, Nk=200, qd=16, cd=None, scale=6.0, p=0.0, mask=None),
    "masked":             dict(B=2, H=2, Nq=9, Nk=70, qd=16, cd=16, scale=1.0, p=0.0, mask="b0_10_39_b1_all"),
    "dropout_p10":        dict(B=2, H=2, Nq=130, Nk=200, qd=16, cd=16, scale=1.0, p=0.1, mask=None,
                               rng=(0x1234567887654321, 0x100000003)),
    "dropout_p50_masked": dict(B=1, H=2, Nq=70, Nk=130, qd=16, cd=16, scale=1.0, p=0.5, mask="some",
                               rng=(20240229, 7)),
    # (appended: make_inputs seeds by position.)  The first four reach the four-wave launch form (launch_form below; width 8
    # keeps their files under the size limit), the last three the key tiles that are masked as a whole.
    "wide_ragged":         dict(B=16, H=8, Nq=70, Nk=130, qd=8, cd=8, scale=1.0, p=0.0, mask=None),
    "wide_fwd_narrow_dkv": dict(B=16, H=8, Nq=70, Nk=40, qd=8, cd=8, scale=1.0, p=0.0, mask=None),
    "narrow_fwd_wide_dkv": dict(B=16, H=8, Nq=40, Nk=70, qd=8, cd=8, scale=1.0, p=0.0, mask=None),
    "wide_masked_dropout": dict(B=16, H=8, Nq=70, Nk=130, qd=8, cd=8, scale=1.0, p=0.25, mask="b_mod_4",
                                rng=(0x0F1E2D3C4B5A6978, 0x200000005)),
    "first_tiles_masked":  dict(B=2, H=2, Nq=20, Nk=130, qd=16, cd=16, scale=1.0, p=0.0, mask="b0_0_63_b1_0_127"),
    "last_tiles_masked":   dict(B=2, H=2, Nq=20, Nk=130, qd=16, cd=16, scale=1.0, p=0.0, mask="b0_64_on_b1_all_but_129"),
    "all_masked_dropout":  dict(B=2, H=2, Nq=20, Nk=130, qd=16, cd=16, scale=1.0, p=0.5, mask="b0_60_69_b1_all",
                                rng=(0xC0FFEE, 0x1FFFFFFFF)),
}

# The launch form each appended case is there to reach: (forward and dQ, dK/dV), "wide" = four waves per workgroup.
# tests/test_attention.py restates the library's launch rule from the constants of mgs_attention.hip and asserts this table.
LAUNCH_FORMS = {
    "wide_ragged": ("wide", "wide"), "wide_fwd_narrow_dkv": ("wide", "narrow"), "narrow_fwd_wide_dkv": ("narrow", "wide"),
    "wide_masked_dropout": ("wide", "wide"), "first_tiles_masked": ("narrow", "narrow"),
    "last_tiles_masked": ("narrow", "narrow"), "all_masked_dropout": ("narrow", "narrow"),
}


# ---- the dropout function, in numpy ------------------------------------------------------------------------------------------
def _philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw 2011) on uint32 arrays; the key is bumped after every round."""
    M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    W0, W1 = 0x9E3779B9, 0xBB67AE85
    lo32 = np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in (c0, c1, c2, c3))
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & lo32, p1 >> np.uint64(32), p1 & lo32
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def keep_threshold(p):
    return int(np.floor(float(np.float32(p)) * 4294967296.0))


def keep_mask(seed, offset, BH, Nq, Nk, p):
    """bool [BH, Nq, Nk]: element (b H + h, i, j) is kept iff word (j & 3) of Philox4x32-10 with counter
    (j >> 2, i, b H + h, offset & 0xffffffff) and key (seed & 0xffffffff, (seed >> 32) ^ (offset >> 32)) is
    >= floor(float32(p) * 2^32)."""
    seed, offset = int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset) & 0xFFFFFFFFFFFFFFFF
    J4 = (Nk + 3) // 4
    bh = np.arange(BH, dtype=np.uint64)[:, None, None]
    i = np.arange(Nq, dtype=np.uint64)[None, :, None]
    j4 = np.arange(J4, dtype=np.uint64)[None, None, :]
    shape = (BH, Nq, J4)
    w = _philox4x32_10(np.broadcast_to(j4, shape), np.broadcast_to(i, shape), np.broadcast_to(bh, shape),
                       np.full(shape, offset & 0xFFFFFFFF, dtype=np.uint64), seed & 0xFFFFFFFF,
                       ((seed >> 32) ^ (offset >> 32)) & 0xFFFFFFFF)
    words = np.stack(w, axis=-1).reshape(BH, Nq, 4 * J4)[:, :, :Nk]
    return words >= np.uint64(keep_threshold(p))


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def mask_pattern(name, B, Nk):
    """bool [B, Nk], False: masked."""
    m = torch.ones(B, Nk, dtype=torch.bool)
    if name == "b0_10_39_b1_all":
        m[0, 10:40] = False
        m[1, :] = False
    elif name == "some":  # every third key and a run across a tile boundary
        m[:, ::3] = False
        m[:, 60:70] = False
    elif name == "b_mod_4":  # the first key tile; every tile but the first; everything; every third key
        m[0::4, :64] = False
        m[1::4, 64:] = False
        m[2::4, :] = False
        m[3::4, ::3] = False
    elif name == "b0_0_63_b1_0_127":  # one and two whole tiles masked, live keys after them
        m[0, :64] = False
        m[1, :128] = False
    elif name == "b0_64_on_b1_all_but_129":  # live keys first, then whole masked tiles; one live key at the ragged end
        m[0, 64:] = False
        m[1, :129] = False
    elif name == "b0_60_69_b1_all":
        m[0, 60:70] = False
        m[1, :] = False
    else:
        raise KeyError(name)
    return m


def case_mask(case):
    c = CASES[case]
    return None if c["mask"] is None else mask_pattern(c["mask"], c["B"], c["Nk"])


def make_inputs(case):
    """x, context (None: self-attention), mask (None or bool [B,Nk]), upstream gradient, parameters {name: tensor}: fp32 on the CPU,
    from a generator seeded by the case's position (the committed fixtures are these numbers)."""
    c = CASES[case]
    g = torch.Generator().manual_seed(1000 + list(CASES).index(case))
    inner = c["H"] * DIM_HEAD
    cd = c["qd"] if c["cd"] is None else c["cd"]
    x = torch.randn(c["B"], c["Nq"], c["qd"], generator=g) * c["scale"]
    context = None if c["cd"] is None else torch.randn(c["B"], c["Nk"], cd, generator=g) * c["scale"]
    grad = torch.randn(c["B"], c["Nq"], c["qd"], generator=g)

    def uniform(shape, fan_in):
        return (torch.rand(*shape, generator=g) * 2 - 1) / fan_in ** 0.5

    params = {"to_q.weight": uniform((inner, c["qd"]), c["qd"]), "to_kv.weight": uniform((2 * inner, cd), cd),
              "to_out.weight": uniform((c["qd"], inner), inner), "to_out.bias": uniform((c["qd"],), inner)}
    return x, context, case_mask(case), grad, params


def grad_names(case):
    names = ["out", "dx"] + ([] if CASES[case]["cd"] is None else ["dcontext"]) + ["d" + n for n in PARAMS]
    return names


# ---- the reference -----------------------------------------------------------------------------------------------------------
def have_reference() -> bool:
    return os.path.isfile(REF_FILE)


_REF = []


def load_reference():
    """perceiver_lang_io.py, unmodified.  What this container lacks of its imports -- termcolor and the five class names of
    helpers.network_utils -- are empty stand-ins that class Attention never touches; they are removed again after the load."""
    if _REF:
        return _REF[0]
    names = ("termcolor", "helpers", "helpers.network_utils")
    before = {n: sys.modules.get(n) for n in names}
    tc = types.ModuleType("termcolor")
    tc.colored, tc.cprint = (lambda s, *a, **k: s), (lambda *a, **k: None)
    hp = types.ModuleType("helpers")
    hp.__path__ = []
    nu = types.ModuleType("helpers.network_utils")
    for n in ("DenseBlock", "SpatialSoftmax3D", "Conv3DBlock", "Conv3DUpsampleBlock", "MultiLayer3DEncoderShallow"):
        setattr(nu, n, type(n, (), {}))
    hp.network_utils = nu
    sys.modules.update({"termcolor": tc, "helpers": hp, "helpers.network_utils": nu})
    try:
        spec = importlib.util.spec_from_file_location("_mgs_reference_perceiver_lang_io", REF_FILE)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for n, m in before.items():
            if m is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = m
    _REF.append(mod)
    return mod


class FixedDropout(torch.nn.Module):
    """Stands where the reference module keeps its nn.Dropout: multiplies by keep / (1 - p)."""

    def __init__(self, keep, p):
        super().__init__()
        self.keep, self.p = keep, p

    def forward(self, attn):
        return attn * (self.keep.to(attn.dtype) / (1.0 - self.p))


def _run(module, x, context, mask, grad, dtype):
    module = module.to(dtype)
    x = x.detach().to(dtype).clone().requires_grad_(True)
    context = None if context is None else context.detach().to(dtype).clone().requires_grad_(True)
    out = module(x, context=context, mask=mask)
    out.backward(grad.to(dtype))
    res = {"out": out.detach(), "dx": x.grad}
    if context is not None:
        res["dcontext"] = context.grad
    for n, prm in module.named_parameters():
        res["d" + n] = prm.grad
    return res


def reference_case(case):
    """{array name: numpy array}: the fixture of `case`, computed from the reference."""
    c = CASES[case]
    ref = load_reference()
    x, context, mask, grad, params = make_inputs(case)
    res = {}
    for dtype in (torch.float32, torch.float64):
        m = ref.Attention(c["qd"], context_dim=c["cd"], heads=c["H"], dim_head=DIM_HEAD, dropout=c["p"])
        m.load_state_dict(params, strict=True)
        m.train()
        if c["p"] > 0:
            keep = keep_mask(*c["rng"], c["B"] * c["H"], c["Nq"], c["Nk"], c["p"])
            m.dropout = FixedDropout(torch.from_numpy(keep), float(np.float32(c["p"])))
        res[dtype] = _run(m, x, context, mask, grad, dtype)
    names = grad_names(case)
    assert sorted(names) == sorted(res[torch.float64]), (names, sorted(res[torch.float64]))
    out = {"x": x.numpy(), "grad": grad.numpy()}
    if context is not None:
        out["context"] = context.numpy()
    if mask is not None:
        out["mask"] = mask.numpy()
    for n, t in params.items():
        out[n] = t.numpy()
    err = []
    for n in names:
        t64, t32 = res[torch.float64][n], res[torch.float32][n].double()
        out[n + "64"] = t64.numpy()
        mag = t64.abs().max().item()
        err.append((t32 - t64).abs().max().item() / mag if mag > 0 else 0.0)
    out["ref_err"] = np.asarray(err, dtype=np.float64)
    return out


def fixture_path(case):
    return os.path.join(GOLDEN_DIR, case + ".npz")


_FIXTURES = {}


def load_fixture(case):
    """The committed fixture as {name: tensor}, loaded once and shared (do not modify); ref_err as {tensor name: float}."""
    if case not in _FIXTURES:
        with np.load(fixture_path(case)) as z:
            f = {k: torch.from_numpy(z[k]) for k in z.files if k != "ref_err"}
            f["ref_err"] = dict(zip(grad_names(case), z["ref_err"].tolist()))
        _FIXTURES[case] = f
    return _FIXTURES[case]


def bounds(case, f=None):
    """{tensor name: (largest allowed |ours - truth|, max|truth|, ref_err)} from the fixture alone."""
    f = load_fixture(case) if f is None else f
    names = grad_names(case)
    mags = {n: f[n + "64"].abs().max().item() for n in names}
    other = max(mags[n] for n in names if n != "out")
    res = {}
    for n in names:
        if mags[n] > 0:
            res[n] = (FACTOR * f["ref_err"][n] * mags[n], mags[n], f["ref_err"][n])
        else:
            res[n] = (ZERO_BOUND * other, 0.0, 0.0)
    return res
