"""The pointwise (1x1x1) Conv3d with bias of the voxel encoder stem's conv_out (manigaussian_amd/pointwise.py, csrc/mgs_pointwise.hip)
against torch's own F.conv3d on the CPU (tests/pointwise_cases.py): float64 is the truth, the float32 CPU run the yardstick,
    |ours - truth| <= 16 x max(yardstick, 2^-23) x max|truth|    for y, dx, dw and db of every case.
"""
import importlib
import json
import os
import re

import pytest
import torch

import conv_family as cf
import pointwise_cases as pc
from manigaussian_amd import _lib
from manigaussian_amd import encoder as enc

pw = importlib.import_module("manigaussian_amd.pointwise")

gpu = pytest.mark.gpu
ROOT = cf.ROOT
FAMILY = cf.FAMILIES["pointwise"]
BENCH_SHAPES = ("conv_out_100", "conv_out_50", "conv_out_25")


@pytest.fixture
def switches():
    """Sets encoder.POINTWISE / FORCE / CONV for one test and puts them back."""
    saved = (enc.POINTWISE, enc.FORCE, enc.CONV)

    def set_(pointwise=None, force=None, conv=None):
        enc.POINTWISE, enc.FORCE, enc.CONV = pointwise, force, conv
    yield set_
    enc.POINTWISE, enc.FORCE, enc.CONV = saved


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
FAKE = cf.FAKE
SHAPE = ("B", "Cin", "Cout", "n")
DEFAULTS = dict(B=1, Cin=4, Cout=8, n=210, x=FAKE, w=FAKE, bias=FAKE, y=FAKE, g=FAKE, dx=FAKE, dw=FAKE, db=FAKE, ws=FAKE)
_fwd = cf.fake_args("mgs_pointwise_forward", "mgs_pointwise_workspace_bytes", SHAPE, DEFAULTS, ("x", "w", "bias", "y"))
_bwd = cf.fake_args("mgs_pointwise_backward", "mgs_pointwise_workspace_bytes", SHAPE, DEFAULTS,
                    ("x", "g", "w", "dx", "dw", "db", "ws", "ws_bytes", "split"))


def test_the_library_refuses_bad_arguments_before_any_launch():
    """Every pointer is a fake address: a launch would fault.  Each refusal carries its message."""
    INV = _lib.MGS_ERR_INVALID_ARG
    shapes = ((dict(Cin=0), "1 to 64"), (dict(Cin=65), "1 to 64"), (dict(Cout=0), "1 to 64"), (dict(Cout=65), "1 to 64"),
              (dict(Cout=-1), "1 to 64"), (dict(B=0), "at least 1"), (dict(B=-3), "at least 1"), (dict(n=0), "at least 1"),
              (dict(n=-2), "at least 1"), (dict(n=1 << 31), "2^31"), (dict(n=1 << 40), "2^31"), (dict(B=1 << 40), "tiles"))
    # what a gradient needs beside these: w for dx, x for dw and db; and one of the three has to be asked for
    cf.check_refusals(_fwd, _bwd, shapes, required=(("x", "w", "y"), ("g", "ws")),
                      pointers=(("x", "w", "bias", "y"), ("x", "g", "w", "dx", "dw", "db", "ws")))
    need = _lib.lib().mgs_pointwise_workspace_bytes(1, 4, 8, 210)
    assert _bwd(ws_bytes=need - 1) == _lib.MGS_ERR_WORKSPACE and "needed" in _lib.last_error()
    assert _bwd(dw=None, db=None, ws_bytes=need - 1, split=65) == INV, "the split is checked even where dx alone is asked for"


def test_the_workspace_size_is_zero_for_illegal_shapes_and_follows_the_records_otherwise():
    W = _lib.lib().mgs_pointwise_workspace_bytes
    for a in ((0, 4, 8, 210), (1, 0, 8, 210), (1, 65, 8, 210), (1, 4, 0, 210), (1, 4, 65, 210), (1, 4, 8, 0), (1, 4, 8, -1),
              (1, 4, 8, 1 << 31), (1 << 40, 4, 8, 210), (-1, 4, 8, 210)):
        assert W(*a) == 0, a
    rec = 8 * (4 + 1) * 4
    assert rec <= W(1, 4, 8, pc.BWD_TILE_8) < rec + 512, "one tile: one record"
    assert 2 * rec <= W(1, 4, 8, pc.BWD_TILE_8 + 1) < 2 * rec + 512, "two tiles: two records"
    assert 2 * rec <= W(2, 4, 8, 5) < 2 * rec + 512, "a tile never straddles batch entries"
    # 100^3 in tiles of 256: 3907 tiles in runs of 62: 64 records; never more than 64, whatever the volume
    rec = 64 * (8 + 1) * 4
    assert 64 * rec <= W(1, 8, 64, 100 ** 3) == W(3, 8, 64, 400 ** 3) < 64 * rec + 512
    rec16 = 64 * (10 + 1) * 4
    assert 2 * rec16 <= W(1, 10, 64, pc.BWD_TILE_16 + 1) < 2 * rec16 + 512, "above 8 input channels the tile is 128 voxels"
    assert all(W(b, ci, co, n) % 256 == 0 and W(b, ci, co, n) > 0 for b in (1, 3) for ci in (1, 8, 64) for co in (1, 64)
               for n in (1, 13, 10 ** 6))


def test_the_abi_version_is_still_17_and_the_new_names_match_the_ctypes_table():
    cf.check_abi(FAMILY.names)


def test_the_op_refuses_cpu_tensors_other_dtypes_and_bad_shapes():
    import manigaussian_amd as mg
    assert mg.pointwise_conv3d is pw.pointwise_conv3d
    x, w, b = torch.zeros(1, 2, 3, 3, 3), torch.zeros(4, 2, 1, 1, 1), torch.zeros(4)
    with pytest.raises(RuntimeError, match="pointwise_conv3d needs float32 tensors on a HIP device .*no CPU path"):
        pw.pointwise_conv3d(x, w, b)
    with pytest.raises(RuntimeError, match="no CPU path"):
        pw.pointwise_conv3d(x.double(), w.double())
    with pytest.raises(RuntimeError, match="no CPU path"):
        pw.pointwise_conv3d(x, "weight")
    if torch.cuda.is_available():
        d = torch.device("cuda:0")
        with pytest.raises(RuntimeError, match="bias is .*no CPU path"):
            pw.pointwise_conv3d(x.to(d), w.to(d), b)
        for xs, ws, bs in (((1, 2, 3, 3), (4, 2, 1, 1, 1), None), ((1, 2, 0, 3, 3), (4, 2, 1, 1, 1), None),
                           ((1, 2, 3, 3, 3), (4, 2, 3, 3, 3), None), ((1, 2, 3, 3, 3), (4, 3, 1, 1, 1), None),
                           ((1, 2, 3, 3, 3), (65, 2, 1, 1, 1), None), ((1, 65, 1, 1, 1), (4, 65, 1, 1, 1), None),
                           ((1, 2, 3, 3, 3), (4, 2, 1, 1, 1), (5,)), ((1, 2, 3, 3, 3), (4, 2, 1, 1), None)):
            with pytest.raises(ValueError):
                pw.pointwise_conv3d(torch.zeros(xs, device=d), torch.zeros(ws, device=d), None if bs is None else torch.zeros(bs, device=d))


@pytest.mark.parametrize("case", pc.ALL)
def test_every_cases_yardstick_is_under_the_ceiling(case):
    r = pc.reference(case)
    assert ("db" in r["ref_err"]) == pc.has_bias(case)
    for q in pc.quantities(case):
        assert r["ref_err"][q] <= pc.REF_ERR_CEILING, (case, q, r["ref_err"][q])


def test_a_cpu_stem_is_torchs_composition_bit_for_bit_whatever_the_switch(switches):
    torch.manual_seed(31)
    m = enc.MultiLayer3DEncoderShallow().train()
    x = torch.randn(2, 10, 12, 12, 12, generator=torch.Generator().manual_seed(32))
    state = {k: v.clone() for k, v in m.state_dict().items()}
    assert len(state) == 62
    got = []
    for value in (False, True, None):
        switches(pointwise=value)
        m.load_state_dict(state, strict=True)
        m.zero_grad()
        xi = x.clone().requires_grad_(True)
        out, voxels = m(xi)
        (out.sum() + voxels[1].pow(2).sum() + voxels[2].pow(2).sum()).backward()
        got.append([out.detach(), voxels[1].detach(), voxels[2].detach(), xi.grad] + [p.grad.clone() for p in m.parameters()]
                   + [b.clone() for b in m.buffers()])
    for other in got[1:]:
        assert len(other) == len(got[0]) and all(torch.equal(a, b) for a, b in zip(got[0], other))
    assert isinstance(m.conv_out, torch.nn.Conv3d) and m.conv_out.bias is not None


def test_what_the_route_looks_at(switches):
    nn, _OnDevice = torch.nn, cf.on_device
    m = enc.MultiLayer3DEncoderShallow()
    x = torch.zeros(1, 8, 4, 4, 4)
    switches(pointwise=True)
    # a CPU tensor, whatever the convolution
    assert not enc._pointwise_routed(m.conv_out, x)
    assert not enc._pointwise_routed(m.conv_out, "x")
    others = {"3x3x3": nn.Conv3d(8, 64, 3, padding=1), "strided": nn.Conv3d(8, 64, 1, stride=2), "padded": nn.Conv3d(8, 64, 1, padding=1),
              "groups": nn.Conv3d(8, 64, 1, groups=2), "dilated 3x3x3": nn.Conv3d(8, 64, 3, padding=2, dilation=2),
              "circular": nn.Conv3d(8, 64, 1, padding_mode="circular"), "65 channels": nn.Conv3d(8, 65, 1),
              "other channels": nn.Conv3d(4, 64, 1), "fp64 weight": nn.Conv3d(8, 64, 1).double()}
    if torch.cuda.is_available():
        d = torch.device("cuda:0")
        xd, real = x.to(d), True
        m.to(d)
        others = {k: c.to(d) for k, c in others.items()}
        others["weight on the host"] = nn.Conv3d(8, 64, 1)
    else:
        xd, real = _OnDevice(x), False   # (the module's weights stay where they are: their device is compared with x's)
    assert enc._pointwise_routed(m.conv_out, xd), "conv_out itself is eligible"
    for name, conv in others.items():
        assert not enc._pointwise_routed(conv, xd), name
    x64 = xd.double() if real else _OnDevice(x.double())
    assert not enc._pointwise_routed(m.conv_out, x64), "fp64"
    x4 = xd[0] if real else _OnDevice(x[0])
    assert not enc._pointwise_routed(m.conv_out, x4), "4-D"
    empty = torch.zeros(1, 8, 0, 4, 4)
    assert not enc._pointwise_routed(m.conv_out, empty.to(xd.device) if real else _OnDevice(empty)), "empty"
    # the switches: POINTWISE = False and FORCE = False switch it off; FORCE = True and CONV = True do not switch it on
    for kw, want in ((dict(pointwise=True), True), (dict(pointwise=False), False), (dict(pointwise=True, force=False), False),
                     (dict(pointwise=None, force=False), False), (dict(pointwise=True, force=True, conv=False), True),
                     (dict(pointwise=None, force=True, conv=True), enc.pointwise_site(8, 64, 64))):
        switches(**kw)
        assert enc._pointwise_routed(m.conv_out, xd) == want, kw
    # the convolutions' own route still leaves conv_out alone
    switches(pointwise=True, conv=True)
    assert not enc._conv_routed(m.conv_out, xd, False)
    assert not enc._conv_routed(m.conv_out, x, False)


def test_the_routing_rule_matches_the_committed_measurement():
    """profiles/pointwise_bench.json (scripts/bench_pointwise.py on an MI355X): pointwise_site() routes a shape ONLY where the op won
    all four (pass, form) pairs, and nothing smaller than the smallest measured winner or at channel counts nobody measured."""
    with open(os.path.join(ROOT, "profiles", "pointwise_bench.json")) as f:
        bench = json.load(f)
    assert sorted(bench["shapes"]) == sorted(BENCH_SHAPES)
    routed, smallest = [], None
    for name, v in bench["shapes"].items():
        won = cf.op_wins(v)
        assert won == v["op_wins"] == bench["routing_as_measured"][name], name
        assert (v["cin"], v["cout"]) == (8, 64) and v["values_per_channel"] == v["side"] ** 3
        rule = enc.pointwise_site(v["cin"], v["cout"], v["values_per_channel"])
        assert bench["routing_in_the_package"][name] == rule, name
        if rule:
            assert won, name
            routed.append(name)
            smallest = v["values_per_channel"] if smallest is None else min(smallest, v["values_per_channel"])
        for side in ("op", "torch"):   # torch's conv_out on its own, pass by pass: the figure DESIGN.md 7m had by subtraction only
            assert set(v["passes_us"][side]) == {"forward", "backward_data", "backward_weight_bias"}, name
    assert sorted(routed) == sorted(bench["routed_shapes"])
    assert enc.POINTWISE_MIN_VALUES == smallest
    for values in (1, 8, 1000, 12 ** 3):   # nothing below the smallest measured winner
        if smallest is None or values < smallest:
            assert not enc.pointwise_site(8, 64, values), values
    for cin, cout in ((8, 32), (10, 64), (64, 64), (1, 1)):   # nothing at channel counts nobody measured
        assert not enc.pointwise_site(cin, cout, 100 ** 3), (cin, cout)
    assert re.fullmatch(r"[0-9a-f]{16}", bench["build_id"])
    stem = bench["stem"]["forward_backward"]
    assert set(stem["eager"]) >= {"rule", "pointwise_off", "all_torch"} and set(stem["graph"]) >= {"rule", "pointwise_off", "all_torch"}
    assert set(bench["patchify"]["passes_us"]) == {"forward", "backward_data", "backward_weight_bias"}
    assert enc.POINTWISE is None


def test_the_switch_follows_the_rule_at_import():
    assert enc.POINTWISE is None and enc.FORCE is None and enc.CONV is None


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
dev = cf.dev


@gpu
@pytest.mark.parametrize("case", pc.ALL)
def test_every_case_forward_and_all_gradients(case):
    cf.check_case(FAMILY, case)


@gpu
@pytest.mark.parametrize("case", ["odd", "tail_3", "stem_out_batch", "long_sum", "wide_odd"])
def test_the_same_bits_across_two_runs_and_across_splits(case):
    cf.check_same_bits(FAMILY, case)


@gpu
@pytest.mark.parametrize("case", ["odd", "in_pre", "wide_odd"])
def test_only_the_requested_gradients_are_computed(case, monkeypatch):
    """dx alone: dw and db are passed as null (and it is the forward's kernel on the transposed weight, adding in the fused kernel's
    order: the same bits)."""
    cf.check_requested_gradients(FAMILY, case, monkeypatch)


@gpu
def test_non_contiguous_and_offset_views_give_the_contiguous_result():
    cf.check_views(FAMILY, "odd")


@gpu
def test_the_stem_with_conv_out_routed_against_torchs_path(switches, monkeypatch):
    """[1,10,12,12,12]: the same module with conv_out routed and not; the truth is the module in float64 on the CPU, the yardstick
    torch's fp32 path on the GPU.  That the kernels ran is read off the library calls, not off differing bits."""
    d = dev()
    torch.manual_seed(41)
    m = enc.MultiLayer3DEncoderShallow().to(d)
    state = {k: v.clone() for k, v in m.state_dict().items()}
    assert len(state) == 62
    gen = torch.Generator().manual_seed(42)
    x = torch.randn(1, 10, 12, 12, 12, generator=gen).to(d)
    g_out, g_v1, g_v2 = (torch.randn(*s, generator=gen).to(d) for s in ((1, 64, 12, 12, 12), (1, 32, 3, 3, 3), (1, 16, 6, 6, 6)))
    calls = cf.count_calls(monkeypatch, FAMILY)

    def once(pointwise, dtype, where):
        switches(pointwise=pointwise)
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
    assert calls == [], "POINTWISE = False: the module's own convolution"
    routed = once(True, torch.float32, d)
    assert calls == [("forward",), ("backward", True, True, True)], calls
    cf.compare_modules("stem", "torch's fp32 path", truth, torchs, routed)
    # the rule leaves a 12^3 volume to torch: the existing small-shape tests run the code they ran before
    del calls[:]
    once(None, torch.float32, d)
    assert calls == []


@gpu
def test_forward_and_backward_captured_into_a_hip_graph():
    """In a child process: stream capture is process-wide state (tests/tools/conv_graph_capture_check.py)."""
    cf.graph_capture(FAMILY.name)


@gpu
def test_nothing_of_the_volumes_size_is_allocated_beside_the_results():
    """[1,8,64,50^3]: after one warm call a forward + backward allocates y, dx, dw and db (the workspace is the device's cached one)."""
    d = dev()
    gen = torch.Generator().manual_seed(51)
    x = torch.randn(1, 8, 50, 50, 50, generator=gen).to(d).requires_grad_(True)
    w = (torch.randn(64, 8, 1, 1, 1, generator=gen) * 8 ** -0.5).to(d).requires_grad_(True)
    b = torch.randn(64, generator=gen).to(d).requires_grad_(True)
    g = torch.randn(1, 64, 50, 50, 50, generator=gen).to(d)
    pw.pointwise_conv3d(x, w, b).backward(g)   # (the cached workspace exists from here on)
    x.grad = w.grad = b.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    y = pw.pointwise_conv3d(x, w, b)
    y.backward(g)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    results = 4 * (y.numel() + x.numel() + w.numel() + b.numel())
    print(f"results {results} bytes; forward + backward peak +{peak}")
    assert peak <= results + (1 << 20)
