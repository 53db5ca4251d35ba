"""The launch layer: what an op wrapper needs between torch and the C ABI of libmgsplat.so -- the current stream, the
current device, a workspace, a pointer, a tensor the kernels can read in place, the float32-on-device check of the operands, and
the call itself with its error check.  Every op module uses these; none keeps a copy of its own.
"""
import ctypes

import torch

from . import _lib

_WORKSPACES = {}  # (device index, bytes) -> uint8 tensor


def _index(dev):
    return dev.index if dev.index is not None else torch.cuda.current_device()


def stream(dev):
    """The raw current stream of dev (the capture stream during a graph capture), as the void* the C ABI takes."""
    return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(_index(dev)))


class on_device:
    """`with torch.cuda.device(dev)` only when dev is not already current (the context manager costs ~10 us)."""

    def __init__(self, dev):
        idx = _index(dev)
        self.ctx = None if idx == torch.cuda.current_device() else torch.cuda.device(idx)

    def __enter__(self):
        if self.ctx is not None:
            self.ctx.__enter__()

    def __exit__(self, *a):
        if self.ctx is not None:
            self.ctx.__exit__(*a)


def ptr(t):
    return None if (t is None or t.numel() == 0) else t.data_ptr()


def readable(t):
    """The tensor itself when the kernels can read it in place (contiguous, 16-byte aligned), else one contiguous copy."""
    if t.is_contiguous() and t.data_ptr() % 16 == 0:
        return t
    return t.contiguous() if not t.is_contiguous() else t.clone()


def need_float32(op, optional=(), **tensors):
    """RuntimeError unless every named operand of `op` is a float32 tensor on a HIP device; an operand named in `optional` may be
    None."""
    for name, t in tensors.items():
        if t is None and name in optional:
            continue
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
            raise RuntimeError(f"{op} needs float32 tensors on a HIP device ({name} is "
                               f"{getattr(t, 'dtype', type(t))} on {getattr(t, 'device', 'the host')}); there is no CPU path")


def call(name, dev, *args):
    """Run the library's `name`(*args, current stream of dev) with dev current; a non-zero return raises RuntimeError
    "<name without mgs_>: <the library's message> (code <rc>)".  The symbol is looked up on the library object at every call,
    so a test that replaces it there is seen."""
    with on_device(dev):
        _lib.check(getattr(_lib.lib(), name)(*args, stream(dev)), name[len("mgs_"):])


def workspace(dev, nbytes):
    """The device's scratch tensor of nbytes bytes (uint8), one per (device index, bytes), allocated on first use.

    The contract every op that takes one relies on: its contents are undefined between calls; an op writes what it reads
    within the same call (tests/test_poisoned_memory.py holds every op to it: it fills the workspace with 0xFF and with 0x7F
    bytes at every fetch and asks for the bits of the clean run).  The tensor is shared by all streams of the device, so two
    streams running the same op concurrently on one device are not supported.  It is never freed, so its address stays valid
    for captured graphs."""
    key = (_index(dev), nbytes)
    ws = _WORKSPACES.get(key)
    if ws is None:
        ws = _WORKSPACES[key] = torch.empty(nbytes, dtype=torch.uint8, device=torch.device("cuda", key[0]))
    return ws
