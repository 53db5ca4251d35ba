"""Cases, float64 truths, fixtures and bounds shared by tests/test_feedforward.py, tests/golden/make_golden_feedforward.py and
tests/tools/feedforward_graph_capture_check.py -- TEST INFRASTRUCTURE.

The ops:  layer_norm(x, w, b, eps) = F.layer_norm over the last dimension;  bias_geglu(h, b): a, gates = (h + b).chunk(2, -1),
a * F.gelu(gates).  The truth of a case is torch's composition in float64 on the CPU; ref_err is the relative max error of the
same composition in float32 against it; ours must lie within FACTOR x max(ref_err, 2^-23) x max|truth|, for the output and every
gradient (the yardstick of tests/volume_cases.py).

A module fixture (tests/golden/feedforward/<name>.npz, arrays only) holds what ManiGaussian's own PreNorm / FeedForward
(agents/manigaussian_bc/perceiver_lang_io.py:56-99, executed unmodified on a CPU) were given and gave:
  x, g (and context): the input, the upstream gradient (and the context), float32;  p.<key>: the parameters by state_dict key;
  out64, dx64 (dcontext64), dp64.<key>: the float64 module's output and the float64 gradients of sum(out g);
  ref_err.out, ref_err.dx (ref_err.dcontext), ref_err.dp.<key>: the float32 module's largest deviation from each over max|truth|.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

import attention_cases as ac
from numerics import rel_err, same_bits  # noqa: F401  (re-exported: the tests and the tools reach them through this module)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden", "feedforward")
FACTOR = 16.0              # tolerance = FACTOR x the reference's own float32 error ...
FLOOR = 2.0 ** -23         # ... which counts as at least one ulp of the truth's magnitude
REF_ERR_CEILING = 1e-5     # a case whose yardstick is looser than this is refused
EPS = 1e-5

# name: rows, D; offset: added to every input; view: x is columns 0..D-1 of a [rows, wide] tensor; expand: the upstream gradient is
# one row expanded over all (row stride 0); frozen: weight and bias take no gradient
LN_CASES = {
    "r3_d5":      dict(rows=3, D=5),
    "r1_d128":    dict(rows=1, D=128),
    "r65_d130":   dict(rows=65, D=130),      # D no multiple of 4: every other row starts off a 16-byte boundary
    "r257_d512":  dict(rows=257, D=512),     # several slabs and a ragged last one
    "r5_d1024":   dict(rows=5, D=1024),      # the limit: four groups per lane
    "r300_d128":  dict(rows=300, D=128),
    "offset30":   dict(rows=65, D=512, offset=30.0),   # a one-pass variance loses ~5e-5 here, 1.2e-5 is allowed
    "strided":    dict(rows=9, D=128, wide=160),
    "expanded_g": dict(rows=33, D=96, expand=True),
    "frozen":     dict(rows=19, D=200, frozen=True),
}
# name: rows, M; gate_scale: the gate half of h is multiplied by it; bias: False = None; wide: h is columns 0..2M-1 of [rows, wide]
GEGLU_CASES = {
    "r1_m1":     dict(rows=1, M=1),
    "r3_m3":     dict(rows=3, M=3),          # the gate half starts off a 16-byte boundary
    "r5_m2048":  dict(rows=5, M=2048),
    "r257_m6":   dict(rows=257, M=6),
    "r65_m130":  dict(rows=65, M=130),
    "saturated": dict(rows=65, M=130, gate_scale=40.0),
    "no_bias":   dict(rows=17, M=36, bias=False),
    "strided":   dict(rows=9, M=20, wide=56),
}
SPLITS = (1, 2, 3, 64)
SPLIT_CASES = ("r257_d512", "r257_m6")


def bound(ref_err):
    return FACTOR * max(ref_err, FLOOR)


# ---- the two ops ------------------------------------------------------------------------------------------------------------------
def ln_inputs(case):
    """x [rows, D] (a view where the case says so), weight, bias, g (expanded where the case says so), fp32, CPU."""
    c = LN_CASES[case]
    gen = torch.Generator().manual_seed(7000 + list(LN_CASES).index(case))
    rows, D = c["rows"], c["D"]
    x = torch.randn(rows, c.get("wide", D), generator=gen) + c.get("offset", 0.0)
    w, b = torch.randn(D, generator=gen), torch.randn(D, generator=gen)
    g = torch.randn(1 if c.get("expand") else rows, D, generator=gen)
    return x[:, :D], w, b, (g.expand(rows, D) if c.get("expand") else g)


def geglu_inputs(case):
    """h [rows, 2M] (a view where the case says so), bias [2M] or None, g [rows, M], fp32, CPU."""
    c = GEGLU_CASES[case]
    gen = torch.Generator().manual_seed(7500 + list(GEGLU_CASES).index(case))
    rows, M = c["rows"], c["M"]
    h = torch.randn(rows, c.get("wide", 2 * M), generator=gen)
    h[:, M:2 * M] *= c.get("gate_scale", 1.0)
    b = torch.randn(2 * M, generator=gen) if c.get("bias", True) else None
    return h[:, :2 * M], b, torch.randn(rows, M, generator=gen)


def ln_compose(x, w, b, eps=EPS):
    return F.layer_norm(x, x.shape[-1:], w, b, eps)


def geglu_compose(h, b):
    if b is not None:
        h = h + b
    a, gates = h.chunk(2, dim=-1)
    return a * F.gelu(gates)


def to_device(t, device):
    """t on the device with its shape, strides and storage offset (a view of a copy of its base)."""
    if t is None or t._base is None:
        return t if t is None else t.to(device)
    return t._base.to(device).as_strided(t.shape, t.stride(), t.storage_offset())


def run_op(fn, inputs, g, dtype=None, device="cpu", frozen=()):
    """fn(*leaves) and the gradients of sum(out g): {"out": .., "d0": .., "d1": ..} by input position (None inputs and the
    positions in `frozen` take no gradient).  dtype None: the tensors as they are (views stay views)."""
    leaves = []
    for k, t in enumerate(inputs):
        if t is not None:
            t = to_device(t, device).detach() if dtype is None else t.detach().to(device=device, dtype=dtype)
            t = t.requires_grad_(k not in frozen)
        leaves.append(t)
    out = fn(*leaves)
    gg = to_device(g, device) if dtype is None else g.to(device=device, dtype=dtype)
    wanted = [(k, t) for k, t in enumerate(leaves) if t is not None and t.requires_grad]
    grads = torch.autograd.grad(out, [t for _, t in wanted], gg)
    res = {"out": out.detach()}
    res.update({f"d{k}": v for (k, _), v in zip(wanted, grads)})
    return res


_TRUTH = {}


def truth(kind, case):
    """The case's CPU truth, computed once and shared (do not modify): inputs, g, the float64 results and the float32
    composition's ref_err per result."""
    key = (kind, case)
    if key not in _TRUTH:
        if kind == "ln":
            *inputs, g = ln_inputs(case)
            fn, frozen = ln_compose, ((1, 2) if LN_CASES[case].get("frozen") else ())
        else:
            *inputs, g = geglu_inputs(case)
            fn, frozen = geglu_compose, ()
        r64 = run_op(fn, inputs, g, torch.float64, frozen=frozen)
        r32 = run_op(fn, inputs, g, torch.float32, frozen=frozen)
        errs = {k: rel_err(r32[k], r64[k]) for k in r64}
        _TRUTH[key] = dict(inputs=inputs, g=g, frozen=frozen, r64=r64, ref_err=errs)
    return _TRUTH[key]


# ---- the module fixtures ----------------------------------------------------------------------------------------------------------
class Probe(nn.Module):
    """Stands where a PreNorm keeps its Attention: a linear on x plus the mean over the sequence of a linear on the context, so
    that the output and the gradients show whether the context was normed and handed on."""

    def __init__(self, dim, context_dim):
        super().__init__()
        self.on_x = nn.Linear(dim, dim)
        self.on_context = nn.Linear(context_dim, dim)

    def forward(self, x, context=None):
        return self.on_x(x) + self.on_context(context).mean(dim=1, keepdim=True)


class PlainAttention(nn.Module):
    """perceiver_lang_io.py:102's Attention without mask and dropout in plain torch calls, any dtype: the float64 side of the
    test that wraps manigaussian_amd.Attention."""

    def __init__(self, query_dim, context_dim, heads, dim_head):
        super().__init__()
        self.heads, self.scale = heads, dim_head ** -0.5
        self.to_q = nn.Linear(query_dim, heads * dim_head, bias=False)
        self.to_kv = nn.Linear(context_dim, 2 * heads * dim_head, bias=False)
        self.to_out = nn.Linear(heads * dim_head, query_dim)

    def forward(self, x, context=None):
        B, H = x.shape[0], self.heads
        q = self.to_q(x)
        k, v = self.to_kv(x if context is None else context).chunk(2, dim=-1)
        q, k, v = (t.reshape(B, t.shape[1], H, -1).transpose(1, 2) for t in (q, k, v))
        attn = (q @ k.transpose(-1, -2) * self.scale).softmax(dim=-1)
        return self.to_out((attn @ v).transpose(1, 2).reshape(B, q.shape[2], -1))


# name: (x shape, context shape or None)
MODULES = {"prenorm_ff": ((2, 7, 12), None), "ff_odd": ((3, 5, 6), None), "prenorm_context": ((2, 7, 16), (2, 5, 8))}
STATE_KEYS = {
    "prenorm_ff": ["fn.net.0.bias", "fn.net.0.weight", "fn.net.2.bias", "fn.net.2.weight", "norm.bias", "norm.weight"],
    "ff_odd": ["net.0.bias", "net.0.weight", "net.2.bias", "net.2.weight"],
    "prenorm_context": ["fn.on_context.bias", "fn.on_context.weight", "fn.on_x.bias", "fn.on_x.weight", "norm.bias", "norm.weight",
                        "norm_context.bias", "norm_context.weight"],
}


def new_module(namespace, name):
    """The module of fixture `name` from `namespace` (the reference's file or manigaussian_amd), freshly initialised."""
    if name == "prenorm_ff":
        return namespace.PreNorm(12, namespace.FeedForward(12))
    if name == "ff_odd":
        return namespace.FeedForward(6, mult=1)   # M = 6: the gate half starts off a 16-byte boundary
    return namespace.PreNorm(16, Probe(16, 8), context_dim=8)


def build_module(namespace, name, seed):
    """... with the layer norms' parameters drawn too (nn.LayerNorm starts at weight 1, bias 0: a gain of one and a zero bias
    would leave their paths untested)."""
    torch.manual_seed(seed)
    m = new_module(namespace, name)
    gen = torch.Generator().manual_seed(seed + 500)
    with torch.no_grad():
        for k, v in sorted(m.state_dict().items()):
            if k.startswith("norm"):
                v.copy_(torch.randn(v.shape, generator=gen) * 0.3 + (1.0 if k.endswith("weight") else 0.0))
    return m


def module_inputs(name):
    """x, context (or None), g(shape) and the parameter seed."""
    seed = 8000 + list(MODULES).index(name)
    gen = torch.Generator().manual_seed(seed)
    xs, cs = MODULES[name]
    x = torch.randn(*xs, generator=gen)
    context = None if cs is None else torch.randn(*cs, generator=gen)
    return x, context, (lambda shape: torch.randn(*shape, generator=gen)), seed


def run_module(m, x, g, dtype, device="cpu", context=None):
    """(out, dx, {key: dparam}, dcontext or None) of module m (moved to dtype / device), as float64 CPU tensors."""
    m = m.to(device=device, dtype=dtype)
    m.zero_grad(set_to_none=True)
    xx = x.detach().to(device=device, dtype=dtype).clone().requires_grad_(True)
    cc = None if context is None else context.detach().to(device=device, dtype=dtype).clone().requires_grad_(True)
    out = m(xx) if cc is None else m(xx, context=cc)
    out.backward(g.to(device=device, dtype=dtype))
    dp = {k: v.grad.detach().double().cpu() for k, v in m.named_parameters()}
    return out.detach().double().cpu(), xx.grad.double().cpu(), dp, (None if cc is None else cc.grad.double().cpu())


def have_reference():
    return ac.have_reference()


def reference_module_case(name):
    """{array name: numpy array}: the fixture of `name`, computed from the reference's classes."""
    ref = ac.load_reference()
    x, context, draw, seed = module_inputs(name)
    m = build_module(ref, name, seed)
    params = {k: v.detach().clone() for k, v in m.state_dict().items()}
    with torch.no_grad():
        g = draw((m(x) if context is None else m(x, context=context)).shape)
    out32, dx32, dp32, dc32 = run_module(m, x, g, torch.float32, context=context)
    out64, dx64, dp64, dc64 = run_module(m, x, g, torch.float64, context=context)
    arrays = {"x": x.numpy(), "g": g.numpy(), "out64": out64.numpy(), "dx64": dx64.numpy(),
              "ref_err.out": np.float64(rel_err(out32, out64)), "ref_err.dx": np.float64(rel_err(dx32, dx64))}
    if context is not None:
        arrays.update({"context": context.numpy(), "dcontext64": dc64.numpy(), "ref_err.dcontext": np.float64(rel_err(dc32, dc64))})
    for k, v in params.items():
        arrays["p." + k] = v.numpy()
        arrays["dp64." + k] = dp64[k].numpy()
        arrays["ref_err.dp." + k] = np.float64(rel_err(dp32[k], dp64[k]))
    worst = max(float(v) for k, v in arrays.items() if k.startswith("ref_err."))
    assert worst <= REF_ERR_CEILING, (name, worst)
    assert sorted(params) == STATE_KEYS[name], (name, sorted(params))
    return arrays


def module_fixture_path(name):
    return os.path.join(GOLDEN_DIR, name + ".npz")


_MODULE_FIXTURES = {}


def load_module_fixture(name):
    """The committed fixture as {array name: tensor (float for ref_err.*)}, loaded once and shared (do not modify)."""
    if name not in _MODULE_FIXTURES:
        with np.load(module_fixture_path(name), allow_pickle=False) as z:
            _MODULE_FIXTURES[name] = {k: (float(z[k]) if k.startswith("ref_err.") else torch.from_numpy(z[k])) for k in z.files}
    return _MODULE_FIXTURES[name]


def fixture_module(namespace, name):
    """The module of fixture `name` from `namespace`, carrying the fixture's parameters (loaded with strict=True)."""
    f = load_module_fixture(name)
    m = new_module(namespace, name)
    m.load_state_dict({k[2:]: v for k, v in f.items() if k.startswith("p.")}, strict=True)
    return m


def module_errors(f, out, dx, dp, dcontext=None):
    """{tensor name: (relative error against the fixture's truth, the fixture's ref_err)}."""
    res = {"out": (rel_err(out, f["out64"]), f["ref_err.out"]), "dx": (rel_err(dx, f["dx64"]), f["ref_err.dx"])}
    if dcontext is not None:
        res["dcontext"] = (rel_err(dcontext, f["dcontext64"]), f["ref_err.dcontext"])
    for k, v in dp.items():
        res["dp." + k] = (rel_err(v, f["dp64." + k]), f["ref_err.dp." + k])
    return res
