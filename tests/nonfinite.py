"""One NaN or infinity in one operand, and what the reference makes of it -- TEST INFRASTRUCTURE of tests/test_nonfinite.py and
tests/golden/make_golden_nonfinite.py.  CPU only, torch only.

Every element of every result and gradient has a class: finite, NaN, +inf or -inf (classes()).  A case is one op on its usual small
inputs with ONE element of ONE operand replaced by a non-finite value (taint()).  The reference -- the op's existing float64 truth:
torch's own composition or the restatement its test file already uses -- is run four times on the CPU:

  r64, r32   the tainted inputs in float64 and in float32.  Their classes must agree at every element of every result: a case in
             which the reference does not speak clearly is REFUSED (Refused, an AssertionError), not excused;
  clean64    the untainted inputs in float64;
  big64      the taint replaced by +2^100, and by -2^100, in float64.  An element that is non-finite in r64 and has clean64's bits
             in both never depended on the tainted element's value (one sign alone can hide behind a ReLU or a clamp that the
             untainted element had already saturated): its non-finite class rests on the taint times an exact zero (a padded zero of im2col, an interpolation weight that is exactly 0, a dropped attention
             weight).  Such an element is FREE: either class is accepted there.  Free elements are capped per op: none at all for
             an op without padding, interpolation or dropout, else at most one eighth of the reference's non-finite elements of any
             result.

compare() then holds the code under test to r64's class at every element that is not free, and, where that class is finite, to the
op's existing bound: FACTOR x max(yardstick, 2^-23) x max|truth| with both maxima and the yardstick (r32 against r64) taken over the
finite elements only.  It prints the 4 x 4 confusion count of every result before it asserts.
"""
import math

import torch

from volume_cases import FACTOR, FLOOR

FINITE, NAN, POS_INF, NEG_INF = 0, 1, 2, 3
NAMES = ("finite", "nan", "+inf", "-inf")
VALUES = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}
BIG = 2.0 ** 100
FREE_SHARE = 1.0 / 8.0


class Refused(AssertionError):
    """The reference does not speak clearly on this case (or the case breaks its cap of free elements)."""


def taint(t, index, value):
    """A contiguous copy of t with the element at flat `index` (negative: from the end) replaced by `value`."""
    out = t.detach().clone().contiguous()
    out.view(-1)[index] = value
    return out


def classes(t):
    """uint8, t's shape: 0 finite, 1 NaN, 2 +inf, 3 -inf."""
    t = t.detach()
    c = torch.zeros(t.shape, dtype=torch.uint8, device=t.device)
    c[torch.isnan(t)] = NAN
    c[t == float("inf")] = POS_INF
    c[t == float("-inf")] = NEG_INF
    return c


def confusion(got_classes, want_classes):
    """[4, 4] counts: row = the reference's class, column = ours."""
    return torch.bincount(want_classes.reshape(-1).long() * 4 + got_classes.reshape(-1).long(), minlength=16).view(4, 4)


def _same_bits(a, b):
    return (a.contiguous().view(torch.int64) == b.contiguous().view(torch.int64)) if a.dtype == torch.float64 else (a == b)


class Admission:
    """What admit() found: r64, r32 {name: tensor or None}, want {name: uint8 classes}, free {name: bool}, the tag."""

    def __init__(self, tag, r64, r32, want, free):
        self.tag, self.r64, self.r32, self.want, self.free = tag, r64, r32, want, free

    def nonfinite(self):
        return sum(int((c != FINITE).sum()) for c in self.want.values())


_CLEAN = {}


def _fresh(inputs):
    """Copies: a reference that marks its float32 inputs as leaves must not mark the case's own tensors."""
    return {k: (v.detach().clone() if isinstance(v, torch.Tensor) else v) for k, v in inputs.items()}


def admit(tag, ref, inputs, operand, index, value, free_share=0.0, clean_key=None, alt=None, cap_refuses=True):
    """ref(inputs, dtype) -> {name: tensor or None} on the CPU; inputs {operand: float32 tensor or anything else}; the taint is
    `value` at flat `index` of inputs[operand].  free_share: 0.0 for an op without padding, interpolation or dropout, else
    FREE_SHARE.  clean_key: the untainted float64 run is computed once per key and shared.  alt: the same operation written in
    other torch ops, where the reference is (or stands for) ONE fused torch op that is free to associate its terms as it likes
    (inf - inf in one order is +-inf in another).  The elements on whose class the two formulations disagree in float64 are UNCLEAR:
    there is no class to hold anyone to, and they alone are exempt, like free elements; every other element of every result is
    compared as usual.  cap_refuses=False: a case over its cap of free elements is not refused but compared at every element
    that is not free (for cases whose masks and dropout put the cap out of reach of every position; Admission.over_cap says so).
    Raises Refused."""
    assert value != value or math.isinf(value), value
    tainted = dict(inputs)
    tainted[operand] = taint(inputs[operand], index, value)
    r64, r32 = ref(_fresh(tainted), torch.float64), ref(_fresh(tainted), torch.float32)
    assert set(r64) == set(r32)
    want = {}
    for k in r64:
        if r64[k] is None:
            assert r32[k] is None, (tag, k)
            continue
        c64, c32 = classes(r64[k]), classes(r32[k])
        if not torch.equal(c64, c32):
            where = (c64 != c32).reshape(-1).nonzero().reshape(-1)[:6].tolist()
            raise Refused(f"{tag}: the reference's float32 and float64 runs disagree on the class of {int((c64 != c32).sum())} elements "
                          f"of {k} (float64 rows, float32 columns {confusion(c32, c64).tolist()}), first at {where}")
        want[k] = c64
    unclear = {k: torch.zeros(c.shape, dtype=torch.bool) for k, c in want.items()}
    if alt is not None:
        a64 = alt(_fresh(tainted), torch.float64)
        unclear = {k: c64 != classes(a64[k]) for k, c64 in want.items()}
    if clean_key is None or clean_key not in _CLEAN:
        clean = ref(_fresh(inputs), torch.float64)
        if clean_key is not None:
            _CLEAN[clean_key] = clean
    else:
        clean = _CLEAN[clean_key]
    big64 = []
    for sign in (1.0, -1.0):
        big = dict(inputs)
        big[operand] = taint(inputs[operand], index, sign * BIG)
        big64.append(ref(_fresh(big), torch.float64))
    free, over = {}, []
    for k, c in want.items():
        assert bool(torch.isfinite(clean[k]).all()), (tag, k, "the untainted truth is not finite")
        free[k] = (c != FINITE) & _same_bits(big64[0][k], clean[k]) & _same_bits(big64[1][k], clean[k])
        n_free, n_bad = int(free[k].sum()), int((c != FINITE).sum())
        if n_free > free_share * n_bad and not cap_refuses:
            over.append((k, n_free, n_bad))
        elif n_free > free_share * n_bad:
            raise Refused(f"{tag}: {n_free} of the reference's {n_bad} non-finite elements of {k} are free (they rest on the taint "
                          f"times an exact zero); at most {free_share:g} of them may be")
    adm = Admission(tag, r64, r32, want, {k: free[k] | unclear[k] for k in free})
    adm.unclear = {k: int(u.sum()) for k, u in unclear.items()}
    adm.over_cap = over
    return adm


def default_bound(truth_finite, ref32_finite, ceiling):
    """FACTOR x max(yardstick, 2^-23) x max|truth| over the finite elements (an empty set: 0)."""
    if truth_finite.numel() == 0:
        return 0.0, 0.0, 0.0
    mag = truth_finite.abs().max().item()
    yard = (ref32_finite.double() - truth_finite).abs().max().item()
    yard = yard / mag if mag > 0 else yard
    assert yard <= ceiling, ("the reference's own float32 error on the finite elements exceeds the op's ceiling", yard, ceiling)
    return FACTOR * max(yard, FLOOR) * mag, yard, mag


def compare_part(label, got, truth, ref32, free, ceiling=1e-5, bound_fn=default_bound):
    """[] or [what is wrong with `got` (CPU) against the float64 `truth`]: the class of every element that is not free, and the
    bound where that class is finite.  Prints the confusion counts and the figures first."""
    if got.shape != truth.shape or got.dtype != torch.float32:
        return [(label, "shape or dtype", tuple(got.shape), got.dtype, tuple(truth.shape))]
    cg, cw = classes(got), classes(truth)
    counts = confusion(cg, cw)
    wrong = (cg != cw) & ~free
    fin = (cw == FINITE) & (cg == FINITE)
    bnd, yard, mag = bound_fn(truth[cw == FINITE], ref32[cw == FINITE], ceiling)
    err = (got[fin].double() - truth[fin]).abs().max().item() if bool(fin.any()) else 0.0
    print(f"{label}: reference rows x our columns over (finite, nan, +inf, -inf) {counts.tolist()}, {int(free.sum())} free, "
          f"{int(wrong.sum())} of the wrong class; finite elements: err {err:.3e}, bound {bnd:.3e} (yardstick {yard:.2e} of {mag:.3e})")
    fails = []
    if bool(wrong.any()):
        at = wrong.reshape(-1).nonzero().reshape(-1)[:6].tolist()
        pairs = sorted({(NAMES[int(cw.reshape(-1)[i])], NAMES[int(cg.reshape(-1)[i])]) for i in at})
        fails.append((label, f"{int(wrong.sum())} elements of the wrong class", [f"reference {a}, ours {b}" for a, b in pairs],
                      "first at flat indices", at))
    if not err <= bnd:
        fails.append((label, "finite elements off their bound", err, bnd))
    return fails


def compare(got, adm, ceiling=1e-5, parts=None, bound_fn=default_bound):
    """got {name: CPU tensor or None} against an Admission.  parts(name) -> [(label, f)] cuts a result into the groups its op's own
    test bounds separately (f maps the result, the truth, the float32 run and the free mask alike); default: the whole tensor."""
    fails = []
    assert set(got) == set(adm.r64), (adm.tag, sorted(got), sorted(adm.r64))
    for k in adm.r64:
        if adm.r64[k] is None or got[k] is None:
            if not (adm.r64[k] is None and got[k] is None):
                fails.append((k, "None on one side only"))
            continue
        for label, f in (parts(k) if parts else [(k, lambda t: t)]):
            g, t, r, fr = f(got[k]), f(adm.r64[k]), f(adm.r32[k]), f(adm.free[k])
            if t.numel():
                fails += compare_part(f"{adm.tag} {label}", g, t, r, fr, ceiling, bound_fn)
    assert not fails, fails
