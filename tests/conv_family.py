"""The harness of the Conv3d families' tests (tests/test_conv3d.py, test_pointwise.py, test_narrow_conv.py, test_dense_conv.py,
test_patch_conv.py, and test_poisoned_memory.py, which walks all five) and of their graph tool (tests/tools/conv_graph_capture_check.py) -- TEST INFRASTRUCTURE, not a test file.

A family is a Family record in FAMILIES: its cases module, its C entry points, how a case's extra arguments reach its op, and what
its backward is handed beside dx, dw and db.  Over that record this file holds once what every family's tests do: one forward +
backward on the device, the comparison with the float64 truth, the same bits across runs and splits, only the requested gradients,
views, the library calls counted, the graph tool's arguments, the routing criterion, the bad-argument builder and the ABI check.
"""
import ctypes
import importlib
import os
import re

import torch

import conv3d_cases
import dense_conv_cases
import narrow_conv_cases
import patch_conv_cases
import pointwise_cases
from child import run_graph_tool
from conv_cases import FACTOR, FLOOR
from manigaussian_amd import _lib
from numerics import dev, same_bits, spy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mgsplat.h")
ABI = 17
ALL_NEEDS = ((True, False, False), (False, True, True), (False, False, True), (True, True, False), (False, False, False))


class Family:
    """name: of the tool's argument; cases: the cases module; prefix + (workspace_bytes, forward, backward...): the C entry points;
    call(case, x, w, b, split): the op on a case's extra arguments, split None: the public op; watched: the backward's parameters
    (include/mgsplat.h's names) whose being given count_calls records; also_given(need): what the parameters of `watched` after dx,
    dw, db are expected to be for need = (x, w, b); expected(case, need): the library calls of one forward + backward, where a
    family's are not forward + backward; needs: the combinations test_only_the_requested_gradients walks."""

    def __init__(self, name, cases, prefix, call, graph_cases, splits=(1, 2, 7, 64), entries=("forward", "backward"),
                 watched=("dx", "dw", "db"), also_given=lambda need: (), expected=None, needs=ALL_NEEDS):
        self.name, self.cases, self.prefix, self.call, self.graph_cases, self.splits = name, cases, prefix, call, graph_cases, splits
        self.entries, self.watched, self.also_given, self.needs = entries, watched, also_given, needs
        self.names = tuple(prefix + e for e in ("workspace_bytes",) + entries)
        if expected is not None:
            self.expected = expected

    def expected(self, case, need):
        need = tuple(need[:2]) + (need[2] and self.cases.has_bias(case),)
        return [("forward",)] + ([("backward",) + need + tuple(self.also_given(need))] if any(need) else [])


def _module(name):
    return importlib.import_module("manigaussian_amd." + name)   # (the package's attribute `conv3d` is the function)


def _pointwise(case, x, w, b, split=None):
    m = _module("pointwise")
    return m.pointwise_conv3d(x, w, b) if split is None else m._pointwise_conv3d(x, w, b, split)


def _narrow(case, x, w, b, split=None):
    m, mode = _module("narrow"), narrow_conv_cases.mode_of(case)
    return m.narrow_conv3d(x, w, b, mode) if split is None else m._narrow_conv3d(x, w, b, mode, split)


def _dense(case, x, w, b, split=None):
    m, slope = _module("dense"), dense_conv_cases.slope_of(case)
    return m.dense_conv3d(x, w, b, slope) if split is None else m._dense_conv3d(x, w, b, slope, split)


def _direct(case, x, w, b, split=None):
    m, cc = _module("conv3d"), conv3d_cases
    if cc.is_transposed(case):
        last = cc.TRANSPOSED[case]["shape"][4]   # output_padding
        return m.conv_transpose3d(x, w, last) if split is None else m._conv_transpose3d(x, w, last, split)
    last = cc.CASES[case]["shape"][4]   # stride
    return m.conv3d(x, w, last) if split is None else m._conv3d(x, w, last, split)


def _direct_expected(case, need):
    """No bias, and an entry point per gradient; the transposed convolution's forward is backward_data and the other way round."""
    first, data = ("backward_data", "forward") if conv3d_cases.is_transposed(case) else ("forward", "backward_data")
    return [(first,)] + [(name,) for name, asked in ((data, need[0]), ("backward_weight", need[1])) if asked]


FAMILIES = {f.name: f for f in (
    Family("conv3d", conv3d_cases, "mgs_conv3d_", _direct, ("stem_in", "up_op1"),
           entries=("forward", "backward_data", "backward_weight"), watched=(), expected=_direct_expected,
           needs=((True, False), (False, True))),
    Family("pointwise", pointwise_cases, "mgs_pointwise_", _pointwise, ("stem_out_batch", "in_pre")),
    # the workspace is passed where dw or db is asked for
    Family("narrow", narrow_conv_cases, "mgs_narrow_conv3d_", _narrow, ("odd", "head"), splits=(1, 3, 64),
           watched=("dx", "dw", "db", "workspace"), also_given=lambda need: (need[1] or need[2],)),
    # the padded gradient is allocated where dx is asked for
    Family("dense", dense_conv_cases, "mgs_dense_conv3d_", _dense, ("odd_k3", "up0_last_head"), splits=(1, 3, 64),
           watched=("dx", "dw", "db", "g_scratch"), also_given=lambda need: (need[0],)),
    # the workspace is passed where dw or db is asked for
    Family("patch", patch_conv_cases, "mgs_patch_conv3d_", patch_conv_cases.call, ("odd", "site_small"), splits=(1, 3, 64),
           watched=("dx", "dw", "db", "workspace"), also_given=lambda need: (need[1] or need[2],)),
)}


# ---- the header and the ctypes table --------------------------------------------------------------------------------------------
def header():
    """include/mgsplat.h without its comments (which name entry points and hold commas and semicolons of their own)."""
    with open(HEADER) as f:
        return re.sub(r"/\*.*?\*/|//[^\n]*", " ", f.read(), flags=re.S)


def ctypes_table():
    """{name: (restype, argtypes)} as bound on the library object."""
    L = _lib.lib()
    return {n: (getattr(L, n).restype, list(getattr(L, n).argtypes)) for n in _lib.exported_symbols()}


def declared(hdr):
    return set(re.findall(r"\b(mgs_[a-z0-9_]+)\s*\(", hdr)) - {"mgs_stream_t"}


def parameters(name, hdr=None):
    """The parameter names of an entry point's declaration in include/mgsplat.h, in order."""
    params = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", header() if hdr is None else hdr, re.S).group(1)
    if params.strip() in ("", "void"):
        return []
    return [re.findall(r"[A-Za-z_]\w*", p)[-1] for p in params.split(",")]


def returns_size_t(name, hdr):
    return re.search(r"\bsize_t\s+" + name + r"\s*\(", hdr) is not None


def check_abi(names=(), table=None):
    """The ABI version; header and ctypes table declare the same names, `names` among them; every entry point has as many argtypes
    as its declaration has parameters; every size query the header declares as size_t returns c_size_t."""
    L, hdr = _lib.lib(), header()
    table = ctypes_table() if table is None else table
    assert _lib.ABI_VERSION == ABI and L.mgs_abi_version() == ABI
    assert "#define MGS_ABI_VERSION %d" % ABI in re.sub(r"[ \t]+", " ", hdr)
    names_declared = declared(hdr)
    assert names_declared and set(table) == names_declared, "ctypes table and header disagree"
    for name in names:
        assert name in names_declared and hasattr(L, name), name
    for name, (restype, argtypes) in sorted(table.items()):
        assert hasattr(L, name), f"{name} declared in mgsplat.h but not exported by libmgsplat.so"
        assert len(parameters(name, hdr)) == len(argtypes), name
        if name.endswith("_bytes") and returns_size_t(name, hdr):
            assert restype is ctypes.c_size_t, name


# ---- the bad-argument tests' calls ----------------------------------------------------------------------------------------------
FAKE = 0x10000


def fake_args(entry, query, shape, defaults, names, query_shape=None):
    """f(**kw): the library's `entry` on the shape names' and `names`' defaults (every pointer the fake address: a launch would
    fault) with kw laid over them and a null stream; ws_bytes None: what `query` says for the shape (its first parameters:
    query_shape), at least 256."""
    def f(**kw):
        a = dict(defaults, ws_bytes=None, split=0)
        a.update(kw)
        if a["ws_bytes"] is None:
            a["ws_bytes"] = max(getattr(_lib.lib(), query)(*(a[k] for k in (query_shape or shape))), 256)
        return getattr(_lib.lib(), entry)(*([a[k] for k in tuple(shape) + tuple(names)] + [None]))
    f.__name__ = entry
    return f


def check_refusals(fwd, bwd, shapes, required, pointers):
    """A bias-carrying family's forward and backward (fake_args' calls) refuse, each with its word in the message: every (kw, word)
    of shapes; a NULL among `required` = (the forward's, the backward's pointers that are never optional); any of `pointers`
    misaligned; a backward without w, without x, or with none of dx, dw, db; a split outside 0..64."""
    INV = _lib.MGS_ERR_INVALID_ARG
    for kw, word in shapes:
        for call in (fwd, bwd):
            assert call(**kw) == INV, (call.__name__, kw)
            assert word in _lib.last_error(), (call.__name__, kw, _lib.last_error())
    for call, names in zip((fwd, bwd), required):
        for p in names:
            assert call(**{p: None}) == INV and "NULL" in _lib.last_error(), (call.__name__, p, _lib.last_error())
    for call, names in zip((fwd, bwd), pointers):
        for p in names:
            assert call(**{p: FAKE + 8}) == INV and "aligned" in _lib.last_error(), (call.__name__, p, _lib.last_error())
    for kw in (dict(w=None), dict(x=None), dict(dx=None, dw=None, db=None)):
        assert bwd(**kw) == INV and "NULL" in _lib.last_error(), kw
    for split in (-1, 65):
        assert bwd(split=split) == INV and "split" in _lib.last_error()


# ---- the routing tests ----------------------------------------------------------------------------------------------------------
class _SaidToBeOnDevice(torch.Tensor):
    """A CPU tensor that answers is_cuda with True: without a GPU the route's other questions can still be asked (its .device stays
    the host's, which is where the modules' weights then are too)."""
    is_cuda = property(lambda self: True)


def on_device(t):
    return t.as_subclass(_SaidToBeOnDevice)


def op_wins(entry, benchmark_may_be_missing=False):
    """The criterion of encoder.fused_site(): in all four (pass, form) pairs the op's third quartile lies below the first quartile of
    torch's faster setting of cudnn.benchmark.  benchmark_may_be_missing: a torch_benchmark child that did not finish is recorded
    as such and not compared."""
    for p in ("forward", "forward_backward"):
        for f in ("eager", "graph"):
            sides = entry[p][f]
            torchs = ("torch", "torch_benchmark")
            if benchmark_may_be_missing:
                torchs = [s for s in torchs if s in sides and "median_us" in sides[s]]
            t = min((sides[s] for s in torchs), key=lambda s: s["median_us"])   # (a KeyError where a side has to be there and is not)
            if not sides["op"]["q3_us"] < t["q1_us"]:
                return False
    return True


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
def run(family, case, split=0, need=(True, True, True), **given):
    """{y, dx, dw, db}: CPU tensors of one forward + backward of the op on the case's inputs (or on x / w / b / g given, on the
    device)."""
    t, d = family.cases.reference(case), dev()
    need = tuple(need) + (True,) * (3 - len(need))

    def leaf(k, wanted):
        v = given.get(k)
        if v is None and t.get(k) is None:
            return None
        return (t[k].to(d) if v is None else v).detach().requires_grad_(wanted)
    x, w, b = leaf("x", need[0]), leaf("w", need[1]), leaf("b", need[2])
    g = t["g"].to(d) if given.get("g") is None else given["g"]
    y = family.call(case, x, w, b, split)
    assert y.is_contiguous()
    if y.requires_grad:
        y.backward(g)
    torch.cuda.synchronize()

    def grad(v):
        if v is None or v.grad is None:
            return None
        # (autograd lays the .grad of a non-contiguous leaf out like the leaf: what the op returned is seen where the leaf is contiguous)
        assert v.grad.is_contiguous() or not v.is_contiguous()
        return v.grad.cpu()
    return {"y": y.detach().cpu(), "dx": grad(x), "dw": grad(w), "db": grad(b)}


def compare(cases, case, got):
    """|got - truth| <= bound for every quantity of the case, with its shape and dtype; prints every figure before it asserts."""
    r = cases.reference(case)
    fails = []
    for q in cases.quantities(case):
        truth, yard = r[q + "64"], r["ref_err"][q]
        assert yard <= cases.REF_ERR_CEILING, (case, q, yard)
        assert got[q].shape == truth.shape and got[q].dtype == torch.float32, (case, q, got[q].shape)
        e, bnd = (got[q].double() - truth).abs().max().item(), cases.bound(yard, truth)
        print(f"{case} {q}: err {e:.3e}, bound {bnd:.3e} (yardstick {yard:.2e} of {truth.abs().max().item():.3e})")
        if not e <= bnd:
            fails.append((q, e, bnd))
    assert not fails, (case, fails)


def compare_modules(label, yardstick, truth, torchs, routed):
    """A module with a site routed against the same module not routed, {name: float64 CPU tensor} each: truth is the module in
    float64 on the CPU, torchs its own fp32 path on the GPU -- the yardstick, named in the printed line -- and routed the op's."""
    fails = []
    for k, want in truth.items():
        mag = want.abs().max().item()
        yard = (torchs[k] - want).abs().max().item() / mag
        e, bnd = (routed[k] - want).abs().max().item(), max(FACTOR * yard, FACTOR * FLOOR) * mag
        print(f"{label} {k}: err {e:.3e}, bound {bnd:.3e} ({yardstick} {yard:.2e} of {mag:.3e})")
        if not e <= bnd:
            fails.append((k, e, bnd))
    assert not fails, fails


def check_case(family, case):
    got = run(family, case)
    compare(family.cases, case, got)
    if "db" not in family.cases.quantities(case):
        assert got["db"] is None


def check_same_bits(family, case):
    """The same bits from a second run and from every forced split."""
    want = run(family, case)
    again = run(family, case)
    for q in family.cases.quantities(case):
        assert same_bits(again[q], want[q]), (case, q, "second run")
    for split in family.splits:
        got = run(family, case, split=split)
        for q in family.cases.quantities(case):
            assert same_bits(got[q], want[q]), (case, q, split)


def backward_positions(family):
    """{entry point: the positions of family.watched in its parameter list}, by the parameters' names in include/mgsplat.h."""
    hdr, at = header(), {}
    for entry in family.entries[1:]:
        names = parameters(family.prefix + entry, hdr)
        at[family.prefix + entry] = tuple(names.index(p) for p in family.watched)
    return at


def count_calls(monkeypatch, family):
    """Replaces the family's entry points on the library object by wrappers that record (name,) per call, and for a backward (name,
    family.watched given ...)."""
    calls, at = [], backward_positions(family)
    spy(_lib.lib(), family.names[1:], monkeypatch,
        on_call=lambda name, a: calls.append((name[len(family.prefix):],) + tuple(bool(a[i]) for i in at.get(name, ()))))
    return calls


def check_requested_gradients(family, case, monkeypatch):
    """Every combination of family.needs: the library is called for what is asked for and handed nothing else, what is not asked for
    is None, and what is has the bits it has when everything is asked for."""
    calls = count_calls(monkeypatch, family)
    want = run(family, case)
    assert calls == family.expected(case, (True, True, True)), calls
    for need in family.needs:
        del calls[:]
        got = run(family, case, need=need)
        assert calls == family.expected(case, tuple(need) + (False,) * (3 - len(need))), (need, calls)
        assert same_bits(got["y"], want["y"]), need
        for q, asked in zip(("dx", "dw", "db"), need):
            if q in family.cases.quantities(case):
                assert (same_bits(got[q], want[q]) if asked else got[q] is None), (need, q)
    del calls[:]
    r, d = family.cases.reference(case), dev()
    with torch.no_grad():
        y = family.call(case, *(None if r.get(k) is None else r[k].to(d) for k in ("x", "w", "b")))
    assert calls == family.expected(case, (False, False, False)) and same_bits(y.cpu(), want["y"])


def channels_last(t):
    v = t.to(dev()).permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3)
    assert not v.is_contiguous() and torch.equal(v, t.to(dev()))
    return v


def strided(t):   # (a [Cout,Cin,1,1,1] weight and a [Cout] bias have no channels-last form: every other element of a longer vector)
    v = torch.empty(2 * t.numel(), device=dev())[::2].view(t.shape)
    v.copy_(t)
    assert not v.is_contiguous() and torch.equal(v, t.to(dev()))
    return v


def shifted(t):
    flat = torch.empty(t.numel() + 1, device=dev())
    v = flat[1:].view(t.shape)   # contiguous, 4 bytes off a 16-byte boundary
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def check_views(family, case):
    """Each of x, w, b and g in turn non-contiguous, and 4 bytes off a 16-byte boundary: the contiguous call's bits."""
    r = family.cases.reference(case)
    want = run(family, case)
    for tag, f in (("channels last", channels_last), ("4-byte offset", shifted)):
        for which in ("x", "w", "b", "g"):
            if r.get(which) is None:
                continue
            no_form = r[which].dim() != 5 or r[which][0, 0].numel() == 1
            got = run(family, case, **{which: strided(r[which]) if (no_form and f is channels_last) else f(r[which])})
            for q in family.cases.quantities(case):
                assert same_bits(got[q], want[q]), (tag, which, q)


def graph_capture(*tool_args):
    """The graph tool in a child process: stream capture is process-wide state."""
    run_graph_tool("conv_graph_capture_check.py", *tool_args)
