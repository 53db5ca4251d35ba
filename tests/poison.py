"""Poisoned workspaces and results (tests/test_poisoned_memory.py) -- TEST INFRASTRUCTURE, not a test file and not a conftest.

`_ops.workspace`'s contract is that its contents are undefined between calls, and every op allocates its results with torch.empty /
torch.empty_like, whose contents are undefined too.  The suite alone cannot see a violation: the workspace of a size keeps the
records of the run before, and the caching allocator hands a just-freed block -- the last run's right answer -- to the next
torch.empty of its size.  Inside `poisoned(monkeypatch, byte)` both hold `byte` in every byte instead:

    0xFF   a float32 reads as NaN, an int32 as -1
    0x7F   a float32 reads as 3.3962e38: finite, so it survives fmaxf, v_max_f32 and x > 0 ? x : 0, which swallow a NaN;
           an int32 reads as 2139062143

An op that reads only what it wrote in the same call computes the bits of its clean run under either.
"""
import contextlib

import torch

from manigaussian_amd import _ops

BYTES = (0xFF, 0x7F)


class Counts:
    """What one `poisoned` context filled so far: workspace fetches, and device tensors of torch.empty / torch.empty_like."""

    def __init__(self, byte):
        self.byte, self.workspaces, self.allocations = byte, 0, 0


def fill_bytes(t, byte):
    """Every byte of the dense tensor t becomes `byte`, on the current stream."""
    if t.is_contiguous():
        t.view(torch.uint8).fill_(byte)
    else:   # (empty_like keeps the strides of a dense, permuted tensor: its elements still are one run of memory)
        torch.as_strided(t, (t.numel(),), (1,), t.storage_offset()).view(torch.uint8).fill_(byte)


@contextlib.contextmanager
def poisoned(monkeypatch, byte):
    """While active, `_ops.workspace` (replaced on the `_ops` module, where every op module looks it up) fills the whole tensor it
    returns with `byte` at EVERY fetch and returns the same tensor object, and torch.empty / torch.empty_like (replaced on the torch
    module) fill every non-empty tensor they return on a HIP device; CPU tensors are left alone.  Yields the Counts.  Everything is put
    back on exit, also after an exception.  Never entered during a graph capture: the fills would be captured with it."""
    if not 0 <= byte <= 0xFF:
        raise ValueError(f"byte = {byte!r}")
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("poisoned() inside a graph capture")
    counts = Counts(byte)
    real_workspace, real_empty, real_empty_like = _ops.workspace, torch.empty, torch.empty_like

    def workspace(dev, nbytes):
        ws = real_workspace(dev, nbytes)
        ws.fill_(byte)
        counts.workspaces += 1
        return ws

    def filled(t):
        if isinstance(t, torch.Tensor) and t.is_cuda and t.numel() > 0:
            fill_bytes(t, byte)
            counts.allocations += 1
        return t

    def empty(*a, **kw):
        return filled(real_empty(*a, **kw))

    def empty_like(*a, **kw):
        return filled(real_empty_like(*a, **kw))

    with monkeypatch.context() as m:
        m.setattr(_ops, "workspace", workspace)
        m.setattr(torch, "empty", empty)
        m.setattr(torch, "empty_like", empty_like)
        yield counts
