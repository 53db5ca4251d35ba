"""What the tests and the graph tools compare and watch with, written once -- TEST INFRASTRUCTURE, not a test file: bit patterns,
the relative error, the device, and the spy on a library object's entry points.  FACTOR, FLOOR and bound are per-op decisions and
stay in the cases modules."""
import collections

import torch

_INTS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def dev():
    return torch.device("cuda:0")


def bits(t):
    """t's bit patterns, flat, as integers of its element size (floating, integer and bool tensors; views are read in their order)."""
    t = t.contiguous()
    return t.view(_INTS[t.element_size()]).reshape(-1)


def same_bits(a, b):
    """Same shape, same dtype, equal bit patterns: 0.0 is not -0.0, and a NaN equals only a NaN of its own payload."""
    return a.shape == b.shape and a.dtype == b.dtype and bool((bits(a) == bits(b)).all())


def rel_err(got, truth):
    """max|got - truth| over max|truth| (the absolute error for an all-zero truth), in float64 on the CPU."""
    got, truth = got.detach().double().cpu(), truth.detach().double().cpu()
    mag = truth.abs().max().item()
    d = (got - truth).abs().max().item()
    return d / mag if mag > 0 else d


def spy(target, names, monkeypatch=None, on_call=None):
    """Wraps target's attributes `names` so that every call is recorded and then made: returns {name: [argument tuple per call]}, an
    entry appearing with its first call.  Installed with monkeypatch.setattr where a monkeypatch is given (and undone with it), with a
    plain setattr otherwise.  on_call(name, args), if given, sees every call first, in the order of the calls across the names."""
    seen = collections.defaultdict(list)

    def wrap(name, real):
        def f(*a):
            if on_call is not None:
                on_call(name, a)
            seen[name].append(a)
            return real(*a)
        return f
    for name in names:
        (setattr if monkeypatch is None else monkeypatch.setattr)(target, name, wrap(name, getattr(target, name)))
    return seen
