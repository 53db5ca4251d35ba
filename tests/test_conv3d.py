"""The direct 3x3x3 Conv3d / ConvTranspose3d of the voxel encoder stem (manigaussian_amd/conv3d.py, csrc/mgs_conv3d.hip) against
torch's own F.conv3d / F.conv_transpose3d on the CPU (tests/conv3d_cases.py): float64 is the truth, the float32 CPU run the yardstick,
    |ours - truth| <= 16 x max(yardstick, 2^-23) x max|truth|    for y, dx and dw of every case.
"""
import importlib
import json
import os
import re

import pytest
import torch

import conv3d_cases as cc
import conv_family as cf
from manigaussian_amd import _lib
from manigaussian_amd import encoder as enc

cv = importlib.import_module("manigaussian_amd.conv3d")   # (the package's attribute of that name is the function)

gpu = pytest.mark.gpu
ROOT = cf.ROOT
FAMILY = cf.FAMILIES["conv3d"]
STEM_SITES = ["conv0", "conv1", "conv2", "conv3", "conv4", "conv5", "conv6", "conv7", "conv9", "conv11"]


@pytest.fixture
def route():
    """Sets encoder.CONV for one test and puts it back."""
    saved = enc.CONV

    def conv(value):
        enc.CONV = value
    yield conv
    enc.CONV = saved


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
FAKE = cf.FAKE
SHAPE = ("B", "Cin", "Cout", "D", "H", "W", "stride")
DEFAULTS = dict(B=1, Cin=4, Cout=8, D=5, H=6, W=7, stride=1, x=FAKE, w=FAKE, y=FAKE, g=FAKE, dx=FAKE, dw=FAKE, ws=FAKE)
_fwd = cf.fake_args("mgs_conv3d_forward", "mgs_conv3d_workspace_bytes", SHAPE, DEFAULTS, ("x", "w", "y"))
_bwd_data = cf.fake_args("mgs_conv3d_backward_data", "mgs_conv3d_workspace_bytes", SHAPE, DEFAULTS, ("g", "w", "dx"))
_bwd_weight = cf.fake_args("mgs_conv3d_backward_weight", "mgs_conv3d_workspace_bytes", SHAPE, DEFAULTS,
                           ("x", "g", "dw", "ws", "ws_bytes", "split"))


def test_the_library_refuses_bad_arguments_before_any_launch():
    """Every pointer is a fake address: a launch would fault.  Each refusal carries its message."""
    INV = _lib.MGS_ERR_INVALID_ARG
    shapes = ((dict(Cin=0), "1 to 64"), (dict(Cin=65), "1 to 64"), (dict(Cout=0), "1 to 64"), (dict(Cout=65), "1 to 64"),
              (dict(Cout=-1), "1 to 64"), (dict(stride=0), "stride must be 1 or 2"), (dict(stride=3), "stride must be 1 or 2"),
              (dict(B=0), "at least 1"), (dict(D=0), "at least 1"), (dict(H=-2), "at least 1"), (dict(W=0), "at least 1"),
              (dict(D=2048, H=1024, W=1024), "2^31"), (dict(D=1, H=1, W=1 << 31), "2^31"), (dict(D=1 << 40, H=1 << 40, W=1), "2^31"),
              (dict(B=1 << 40), "tiles"), (dict(w=None), "NULL"), (dict(w=FAKE + 4), "16-byte aligned"))
    for kw, word in shapes:
        for call in (_fwd, _bwd_data, _bwd_weight):
            if call is _bwd_weight and "w" in kw:
                continue
            assert call(**kw) == INV, (call.__name__, kw)
            assert word in _lib.last_error(), (call.__name__, kw, _lib.last_error())
    own = ((_fwd, ("x", "y")), (_bwd_data, ("g", "dx")), (_bwd_weight, ("x", "g", "dw", "ws")))
    for call, pointers in own:
        for p in pointers:
            assert call(**{p: None}) == INV and "NULL" in _lib.last_error(), (call.__name__, p, _lib.last_error())
            assert call(**{p: FAKE + 8}) == INV and "aligned" in _lib.last_error(), (call.__name__, p, _lib.last_error())
    for split in (-1, 65):
        assert _bwd_weight(split=split) == INV and "split" in _lib.last_error()
    need = _lib.lib().mgs_conv3d_workspace_bytes(1, 4, 8, 5, 6, 7, 1)
    assert _bwd_weight(ws_bytes=need - 1) == _lib.MGS_ERR_WORKSPACE and "needed" in _lib.last_error()


def test_the_workspace_size_is_zero_for_illegal_shapes_and_follows_the_records_otherwise():
    W = _lib.lib().mgs_conv3d_workspace_bytes
    for a in ((0, 4, 8, 5, 6, 7, 1), (1, 0, 8, 5, 6, 7, 1), (1, 65, 8, 5, 6, 7, 1), (1, 4, 0, 5, 6, 7, 1), (1, 4, 65, 5, 6, 7, 1),
              (1, 4, 8, 0, 6, 7, 1), (1, 4, 8, 5, -1, 7, 1), (1, 4, 8, 5, 6, 0, 1), (1, 4, 8, 5, 6, 7, 0), (1, 4, 8, 5, 6, 7, 3),
              (1, 4, 8, 2048, 1024, 1024, 1), (1 << 40, 4, 8, 5, 6, 7, 1), (1, 4, 8, 1 << 62, 4, 4, 2)):
        assert W(*a) == 0, a
    rec = 4 * 8 * 27 * 4
    assert rec <= W(1, 4, 8, 4, 8, 32, 1) < rec + 512, "one tile: one record"
    assert 2 * rec <= W(1, 4, 8, 5, 8, 32, 1) < 2 * rec + 512, "two tiles: two records"
    # 100^3 at stride 1: 25 x 13 x 4 = 1300 tiles in runs of 21: 62 records; never more than 64, whatever the volume
    assert 62 * rec <= W(1, 4, 8, 100, 100, 100, 1) < 62 * rec + 512
    assert 64 * rec <= W(1, 4, 8, 200, 200, 200, 1) == W(3, 4, 8, 400, 400, 400, 2) < 64 * rec + 512
    assert all(W(1, 4, 8, n, n, n, s) % 256 == 0 for n in (1, 13, 100) for s in (1, 2))


def test_the_abi_version_is_still_17_and_the_header_matches_the_ctypes_table():
    cf.check_abi(FAMILY.names)


def test_the_ops_refuse_cpu_tensors_and_other_dtypes():
    import manigaussian_amd as mg
    assert mg.conv3d is cv.conv3d and mg.conv_transpose3d is cv.conv_transpose3d
    x, w = torch.zeros(1, 2, 3, 3, 3), torch.zeros(4, 2, 3, 3, 3)
    with pytest.raises(RuntimeError, match="conv3d needs float32 tensors on a HIP device .*no CPU path"):
        cv.conv3d(x, w)
    with pytest.raises(RuntimeError, match="no CPU path"):
        cv.conv3d(x.double(), w.double(), stride=2)
    with pytest.raises(RuntimeError, match="conv_transpose3d needs float32 tensors on a HIP device .*no CPU path"):
        cv.conv_transpose3d(x, torch.zeros(2, 4, 3, 3, 3), output_padding=1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        cv.conv3d(x, "weight")


def test_a_cpu_stem_with_the_convolutions_forced_equals_torchs_composition_bit_for_bit(route):
    torch.manual_seed(31)
    m = enc.MultiLayer3DEncoderShallow().train()
    x = torch.randn(2, 10, 12, 12, 12, generator=torch.Generator().manual_seed(32))
    state = {k: v.clone() for k, v in m.state_dict().items()}
    assert len(state) == 62
    got = []
    for value in (False, True, None):
        route(value)
        m.load_state_dict(state, strict=True)
        m.zero_grad()
        xi = x.clone().requires_grad_(True)
        out, voxels = m(xi)
        (out.sum() + voxels[1].pow(2).sum() + voxels[2].pow(2).sum()).backward()
        got.append([out.detach(), voxels[1].detach(), voxels[2].detach(), xi.grad] + [p.grad.clone() for p in m.parameters()]
                   + [b.clone() for b in m.buffers()])
    for other in got[1:]:
        assert len(other) == len(got[0]) and all(torch.equal(a, b) for a, b in zip(got[0], other))
    # what the route looks at: everything but a bias-free 3x3x3, padding 1, stride 1 / 2 convolution stays torch's
    route(True)
    xc = torch.zeros(1, 8, 4, 4, 4)
    assert not enc._conv_routed(m.conv1.conv, xc, False) and not enc._conv_routed(m.conv9[0], torch.zeros(1, 32, 4, 4, 4), True)
    assert not enc._conv_routed(m.conv_out, xc, False)


def test_the_routing_rule_matches_the_committed_measurement():
    """profiles/conv3d_bench.json (scripts/bench_conv3d.py on an MI355X): conv_site() routes a site ONLY where the op won all four
    (pass, form) pairs, and nothing smaller than the smallest measured winner."""
    with open(os.path.join(ROOT, "profiles", "conv3d_bench.json")) as f:
        bench = json.load(f)
    assert sorted(bench["sites"]) == sorted(STEM_SITES)
    routed, smallest = [], None
    for name, v in bench["sites"].items():
        won = cf.op_wins(v)
        assert won == v["op_wins"] == bench["routing_as_measured"][name], name
        rule = enc.conv_site(v["cin"], v["cout"], v["voxels"], v["stride"], v["transposed"])
        assert bench["routing_in_the_package"][name] == rule, name
        if rule:
            assert won, name
            routed.append(name)
            smallest = v["voxels"] if smallest is None else min(smallest, v["voxels"])
        for side in ("op", "torch"):
            assert set(v["passes_us"][side]) == {"forward", "backward_data", "backward_weight"}, name
    for name, v in bench["sites"].items():   # nothing below the smallest measured winner, whatever its channels
        for voxels in (1, 8, 1000):
            if smallest is None or voxels < smallest:
                assert not enc.conv_site(v["cin"], v["cout"], voxels, v["stride"], v["transposed"]), (name, voxels)
    assert sorted(routed) == sorted(bench["routed_sites"])
    assert re.fullmatch(r"[0-9a-f]{16}", bench["build_id"])
    assert set(bench["stem"]["forward_backward"]["eager"]) >= {"rule", "conv_on", "conv_off", "parent_fused", "parent_torch"}
    assert enc.CONV is None


@pytest.mark.parametrize("case", cc.ALL)
def test_every_cases_yardstick_is_under_the_ceiling(case):
    r = cc.reference(case)
    for q in cc.QUANTITIES:
        assert r["ref_err"][q] <= cc.REF_ERR_CEILING, (case, q, r["ref_err"][q])


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
dev = cf.dev


@gpu
@pytest.mark.parametrize("case", cc.ALL)
def test_every_case_forward_and_both_gradients(case):
    cf.check_case(FAMILY, case)


@gpu
@pytest.mark.parametrize("case", ["odd_s1", "down_even", "seam_tile_s2", "long_sum", "up_odd"])
def test_the_same_bits_across_two_runs_and_across_splits(case):
    cf.check_same_bits(FAMILY, case)


@gpu
@pytest.mark.parametrize("case", ["down_mixed", "up_odd"])
def test_only_the_requested_gradients_are_computed(case, monkeypatch):
    cf.check_requested_gradients(FAMILY, case, monkeypatch)


@gpu
@pytest.mark.parametrize("case", ["odd_s1", "up_odd"])
def test_non_contiguous_and_offset_views_give_the_contiguous_result(case):
    cf.check_views(FAMILY, case)


@gpu
def test_the_stem_with_the_convolutions_routed_against_torchs_path(route):
    """[1,10,12,12,12]: the same module with every convolution site routed and with none; the truth is the module in float64 on the
    CPU, the yardstick torch's fp32 path on the GPU."""
    d = dev()
    torch.manual_seed(41)
    m = enc.MultiLayer3DEncoderShallow().to(d)
    state = {k: v.clone() for k, v in m.state_dict().items()}
    gen = torch.Generator().manual_seed(42)
    x = torch.randn(1, 10, 12, 12, 12, generator=gen).to(d)
    g_out, g_v1, g_v2 = (torch.randn(*s, generator=gen).to(d) for s in ((1, 64, 12, 12, 12), (1, 32, 3, 3, 3), (1, 16, 6, 6, 6)))

    def once(conv, dtype, where):
        route(conv)
        m.load_state_dict(state)
        m.to(where, dtype).train().zero_grad()
        out, voxels = m(x.to(where, dtype))
        to = dict(device=where, dtype=dtype)
        ((out * g_out.to(**to)).sum() + (voxels[1] * g_v1.to(**to)).sum() + (voxels[2] * g_v2.to(**to)).sum()).backward()
        r = {"out": out.detach(), "voxel1": voxels[1].detach(), "voxel2": voxels[2].detach()}
        r.update({"grad " + n: p.grad for n, p in m.named_parameters()})
        r.update({n: b.clone() for n, b in m.named_buffers() if b.dtype.is_floating_point})
        r = {k: v.detach().double().cpu().clone() for k, v in r.items()}   # (copies: m.to() below converts the gradients in place)
        m.to(d, torch.float32)
        return r

    truth = once(False, torch.float64, "cpu")
    torchs = once(False, torch.float32, d)
    routed = once(True, torch.float32, d)
    cf.compare_modules("stem", "torch's fp32 path", truth, torchs, routed)
    assert any((routed[k] != torchs[k]).any() for k in routed), "the forced route changed nothing: the kernels did not run"


@gpu
def test_forward_and_backward_captured_into_a_hip_graph():
    """In a child process: stream capture is process-wide state (tests/tools/conv_graph_capture_check.py)."""
    cf.graph_capture(FAMILY.name)


@gpu
def test_nothing_of_the_volumes_size_is_allocated_beside_the_results():
    """[1,8,16,50^3, stride 2]: one forward + backward allocates y, dx and dw (the workspace is the device's cached one)."""
    d = dev()
    gen = torch.Generator().manual_seed(51)
    x = torch.randn(1, 8, 50, 50, 50, generator=gen).to(d).requires_grad_(True)
    w = (torch.randn(16, 8, 3, 3, 3, generator=gen) * (27 * 8) ** -0.5).to(d).requires_grad_(True)
    g = torch.randn(1, 16, 25, 25, 25, generator=gen).to(d)
    cv.conv3d(x, w, 2).backward(g)   # (the cached workspace exists from here on)
    x.grad = w.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    y = cv.conv3d(x, w, 2)
    y.backward(g)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    results = 4 * (y.numel() + x.numel() + w.numel())
    print(f"results {results} bytes; forward + backward peak +{peak}")
    assert peak <= results + (1 << 20)
