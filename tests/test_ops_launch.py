"""The launch layer (manigaussian_amd/_ops.py): the stream, the device, the workspace and the checked call every fused op's
wrapper goes through.  The ops' own suites check what the kernels compute; these check what lies between torch and the C ABI.
"""
import ctypes

import pytest
import torch

gpu = pytest.mark.gpu


def _ops_lib():
    from manigaussian_amd import _lib, _ops
    return _ops, _lib


def _raw(dev):
    from manigaussian_amd import _ops
    return _ops.stream(dev).value or 0  # (ctypes reads a NULL void* back as None: the default stream)


def _volume(shape, dev):
    g = torch.Generator().manual_seed(7)
    return torch.randn(shape, generator=g).to(dev)


# ---- stream ------------------------------------------------------------------------------------------------------------------
@gpu
def test_stream_is_the_current_stream_of_the_device():
    _ops, _ = _ops_lib()
    dev = torch.device("cuda:0")
    assert isinstance(_ops.stream(dev), ctypes.c_void_p)
    assert _raw(dev) == torch.cuda.current_stream(dev).cuda_stream
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        assert s.cuda_stream != 0 and _raw(dev) == s.cuda_stream
        assert _raw(torch.device("cuda")) == s.cuda_stream
    assert _raw(dev) == torch.cuda.current_stream(dev).cuda_stream


@gpu
def test_an_op_enqueued_under_a_stream_runs_on_it():
    from manigaussian_amd.spatial_softmax import spatial_softmax3d
    dev = torch.device("cuda:0")
    x = _volume((1, 1, 2, 2, 4), dev)
    want = spatial_softmax3d(x).cpu()  # the default stream (and the copy waits for it: the shared workspace is free again)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        got = spatial_softmax3d(x)
        done = torch.cuda.Event()
        done.record(s)
    done.synchronize()  # waits for s alone: a kernel that went to another stream is not covered by it
    assert torch.equal(got.cpu(), want)


# ---- workspace ---------------------------------------------------------------------------------------------------------------
@gpu
def test_workspace_is_one_tensor_per_device_and_size():
    _ops, _ = _ops_lib()
    dev = torch.device("cuda:0")
    a = _ops.workspace(dev, 4096)
    assert _ops.workspace(dev, 4096) is a
    b = _ops.workspace(dev, 8192)
    assert b is not a and b.data_ptr() != a.data_ptr()
    for t, n in ((a, 4096), (b, 8192)):
        assert t.dtype == torch.uint8 and t.numel() == n and t.device == dev
    with torch.cuda.device(0):
        assert _ops.workspace(torch.device("cuda"), 4096) is a  # no index: the current device's entry


# ---- a tensor the kernels can read in place (no GPU needed) ------------------------------------------------------------------
def test_readable_keeps_a_contiguous_aligned_tensor_and_copies_the_rest():
    _ops, _ = _ops_lib()
    t = torch.arange(24.0).view(2, 3, 4)
    assert t.is_contiguous() and t.data_ptr() % 16 == 0
    assert _ops.readable(t) is t
    v = t.transpose(0, 2)
    assert not v.is_contiguous()
    c = _ops.readable(v)
    assert c is not v and c.is_contiguous() and c.data_ptr() % 16 == 0 and c.shape == v.shape and torch.equal(c, v)
    base = torch.zeros(9)
    assert base.data_ptr() % 16 == 0
    o = base[1:]
    o += torch.arange(8.0)
    assert o.is_contiguous() and o.data_ptr() % 16 == 4
    a = _ops.readable(o)
    assert a is not o and a.data_ptr() != o.data_ptr() and a.is_contiguous() and a.data_ptr() % 16 == 0 and torch.equal(a, o)


# ---- the checked call --------------------------------------------------------------------------------------------------------
@gpu
def test_call_raises_the_library_s_message_under_the_symbol_s_name():
    _ops, _ = _ops_lib()
    dev = torch.device("cuda:0")
    with pytest.raises(RuntimeError, match=r"^spatial_softmax_forward: .*\(code -1\)$"):
        # rows = 0: refused before any launch
        _ops.call("mgs_spatial_softmax_forward", dev, 0, 1, 1, 1, 1, 0.01, None, None, 0, None, 0, None, None, 0, 0)


@gpu
def test_call_looks_the_symbol_up_at_call_time(monkeypatch):
    _ops, _lib = _ops_lib()
    dev = torch.device("cuda:0")
    seen = []

    def spy(*args):
        seen.append(args)
        return 0

    monkeypatch.setattr(_lib.lib(), "mgs_spatial_softmax_forward", spy)
    _ops.call("mgs_spatial_softmax_forward", dev, 0, 1, 1, 1, 1, 0.01, None, None, 0, None, 0, None, None, 0, 0)
    assert len(seen) == 1 and seen[0][:6] == (0, 1, 1, 1, 1, 0.01)
    assert isinstance(seen[0][-1], ctypes.c_void_p) and (seen[0][-1].value or 0) == _raw(dev)  # the stream goes last


# ---- a device that is not current --------------------------------------------------------------------------------------------
@gpu
@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two devices")
def test_an_op_on_another_device_runs_there_and_leaves_the_current_device():
    from manigaussian_amd.spatial_softmax import spatial_softmax3d
    x = _volume((1, 2, 2, 2, 4), "cpu")
    with torch.cuda.device(0):
        want = spatial_softmax3d(x.to("cuda:0"))
        got = spatial_softmax3d(x.to("cuda:1"))
        assert torch.cuda.current_device() == 0
    assert got.device == torch.device("cuda:1")
    assert torch.equal(got.cpu(), want.cpu())

