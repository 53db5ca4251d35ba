"""The pointwise (1x1x1) Conv3d for 1..16 input and 65..256 output channels -- the voxel encoder stem's conv_out at final_dim = 128
(manigaussian_amd/pointwise.py: wide_pointwise_conv3d; csrc/mgs_pointwise.hip: mgs_pointwise_wide_*) -- against torch's own F.conv3d
on the CPU (tests/wide_pointwise_cases.py): float64 is the truth, the float32 CPU run the yardstick,
    |ours - truth| <= 16 x max(yardstick, 2^-23) x max|truth|    for y, dx, dw and db of every case.

Who writes and who first reads every region of the op, read off the host code and the kernel before any of this ran on a GPU (the
form of tests/test_poisoned_memory.py's table; "ws": the region of `_ops.workspace`; "-": never read by a kernel):

op (module)           region                                 first writer                         first reader
--------------------  -------------------------------------  -----------------------------------  ------------------------------------
pointwise (wide op)   ws records [nrec, Cout, Cin + 1]       pw_bwd_kernel<.., BLOCKS>, ONE       records_merge_kernel
                                                             launch: rows 64 c .. 64 c + 63 of a
                                                             run's record in the run's block c,
                                                             the bias column with them
                      dx (empty_like), with dw or db         pw_bwd_kernel, block 0 of the run    pw_bwd_kernel, block 1 of the SAME
                                                             that holds the tile: every element   run: every thread reads back the
                                                             of the tile by one thread            elements it stored itself, and stores
                                                                                                  them again; block c + 1 reads block c's
                      dx alone | y | dw, db                  pw_fwd_wide<TRANS> | pw_fwd_narrow   -
                                                             | merge
"""
import importlib
import json
import os
import re

import pytest
import torch

import conv_family as cf
import nonfinite as nf
import poison
import wide_pointwise_cases as wc
from child import run_graph_tool
from manigaussian_amd import _lib
from manigaussian_amd import encoder as enc
from numerics import same_bits

pw = importlib.import_module("manigaussian_amd.pointwise")

gpu = pytest.mark.gpu
ROOT = cf.ROOT
FAMILY = cf.Family("pointwise_wide", wc, "mgs_pointwise_wide_", wc.call, ("stem_out_128_batch", "in_16"))
BENCH_SHAPES = ("conv_out128_100", "conv_out128_50", "conv_out128_25")


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
DEFAULTS = dict(B=1, Cin=4, Cout=72, n=210, x=FAKE, w=FAKE, bias=FAKE, y=FAKE, g=FAKE, dx=FAKE, dw=FAKE, db=FAKE, ws=FAKE)
_fwd = cf.fake_args("mgs_pointwise_wide_forward", "mgs_pointwise_wide_workspace_bytes", SHAPE, DEFAULTS, ("x", "w", "bias", "y"))
_bwd = cf.fake_args("mgs_pointwise_wide_backward", "mgs_pointwise_wide_workspace_bytes", SHAPE, DEFAULTS,
                    ("x", "g", "w", "dx", "dw", "db", "ws", "ws_bytes", "split"))


def test_the_library_refuses_bad_arguments_before_any_launch():
    """Every pointer is a fake address: a launch would fault.  Each refusal carries its message."""
    INV = _lib.MGS_ERR_INVALID_ARG
    shapes = ((dict(Cin=0), "1 to 16"), (dict(Cin=17), "1 to 16"), (dict(Cout=64), "65 to 256"), (dict(Cout=257), "65 to 256"),
              (dict(Cout=-1), "65 to 256"), (dict(B=0), "at least 1"), (dict(B=-3), "at least 1"), (dict(n=0), "at least 1"),
              (dict(n=-2), "at least 1"), (dict(n=1 << 31), "2^31"), (dict(n=1 << 40), "2^31"), (dict(B=1 << 40), "tiles"))
    cf.check_refusals(_fwd, _bwd, shapes, required=(("x", "w", "y"), ("g", "ws")),
                      pointers=(("x", "w", "bias", "y"), ("x", "g", "w", "dx", "dw", "db", "ws")))
    need = _lib.lib().mgs_pointwise_wide_workspace_bytes(1, 4, 72, 210)
    assert _bwd(ws_bytes=need - 1) == _lib.MGS_ERR_WORKSPACE and "needed" in _lib.last_error()
    assert _bwd(dw=None, db=None, ws_bytes=need - 1, split=65) == INV, "the split is checked even where dx alone is asked for"


ALIGN, MAX_REC = 256, 64   # csrc/mgs_common.h


def _ceil(a, b):
    return -(-a // b)


def cut_runs(items, most):
    """(records, items per record, items of the last record): csrc/mgs_records.hip's cut_runs, restated."""
    per = _ceil(items, min(items, most))
    n = _ceil(items, per)
    return n, per, items - (n - 1) * per


def records(B, cin, cout, n):
    """(tiles, bytes of a record, the workspace bytes restated, the library's own): the host code, restated."""
    items, rec = B * _ceil(n, wc.BWD_TILE_8 if cin <= 8 else wc.BWD_TILE_16), 4 * cout * (cin + 1)
    need = _ceil(cut_runs(items, MAX_REC)[0] * rec, ALIGN) * ALIGN + ALIGN
    return items, rec, need, _lib.lib().mgs_pointwise_wide_workspace_bytes(B, cin, cout, n)


def test_the_workspace_size_is_zero_for_illegal_shapes_and_follows_the_records_otherwise():
    W = _lib.lib().mgs_pointwise_wide_workspace_bytes
    for a in ((0, 4, 72, 210), (1, 0, 72, 210), (1, 17, 72, 210), (1, 4, 64, 210), (1, 4, 1, 210), (1, 4, 257, 210), (1, 4, -1, 210),
              (1, 4, 72, 0), (1, 4, 72, -1), (1, 4, 72, 1 << 31), (1 << 40, 4, 72, 210), (-1, 4, 72, 210)):
        assert W(*a) == 0, a
    rec = 72 * (4 + 1) * 4
    assert rec <= W(1, 4, 72, wc.BWD_TILE_8) < rec + 512, "one tile: one record [Cout, Cin + 1], whatever the number of blocks"
    assert 2 * rec <= W(1, 4, 72, wc.BWD_TILE_8 + 1) < 2 * rec + 512, "two tiles: two records"
    assert 2 * rec <= W(2, 4, 72, 5) < 2 * rec + 512, "a tile never straddles batch entries"
    # 100^3 in tiles of 256: 3907 tiles in runs of 62: 64 records; never more than 64, whatever the volume
    rec = 128 * (8 + 1) * 4
    assert 64 * rec <= W(1, 8, 128, 100 ** 3) == W(3, 8, 128, 400 ** 3) < 64 * rec + 512
    rec16 = 130 * (16 + 1) * 4
    assert 2 * rec16 <= W(1, 16, 130, wc.BWD_TILE_16 + 1) < 2 * rec16 + 512, "above 8 input channels the tile is 128 voxels"
    assert all(W(b, ci, co, n) % 256 == 0 and W(b, ci, co, n) > 0 for b in (1, 3) for ci in (1, 8, 16) for co in (65, 128, 256)
               for n in (1, 13, 10 ** 6))
    for case in wc.ALL:
        B, cin, cout, ext, _ = wc.CASES[case]["shape"]
        items, rec, need, got = records(B, cin, cout, ext[0] * ext[1] * ext[2])
        print(case, "tiles", items, "records, per, last", cut_runs(items, MAX_REC), "workspace", got)
        assert need == got, (case, "the restated workspace size is not the library's", need, got)
    tiles = records(*wc.CASES["long_sum_stem"]["shape"][:3], 40 ** 3)[0]
    assert cut_runs(tiles, MAX_REC) == (63, 4, 2), "long_sum_stem: 250 tiles in 63 runs, a shorter last run"
    assert cut_runs(records(1, 2, 65, 27)[0], MAX_REC) == (1, 1, 1) and cut_runs(records(2, 8, 128, 210)[0], MAX_REC)[0] == 2


def test_the_abi_version_is_still_17_and_the_new_names_match_the_ctypes_table():
    cf.check_abi(FAMILY.names)
    assert FAMILY.names == ("mgs_pointwise_wide_workspace_bytes", "mgs_pointwise_wide_forward", "mgs_pointwise_wide_backward")
    assert cf.parameters("mgs_pointwise_wide_backward") == cf.parameters("mgs_pointwise_backward")
    assert cf.parameters("mgs_pointwise_wide_forward") == cf.parameters("mgs_pointwise_forward")


def test_the_op_refuses_cpu_tensors_other_dtypes_and_bad_shapes():
    import manigaussian_amd as mg
    assert mg.wide_pointwise_conv3d is pw.wide_pointwise_conv3d
    x, w, b = torch.zeros(1, 2, 3, 3, 3), torch.zeros(72, 2, 1, 1, 1), torch.zeros(72)
    with pytest.raises(RuntimeError, match="wide_pointwise_conv3d needs float32 tensors on a HIP device .*no CPU path"):
        pw.wide_pointwise_conv3d(x, w, b)
    with pytest.raises(RuntimeError, match="no CPU path"):
        pw.wide_pointwise_conv3d(x.double(), w.double())
    with pytest.raises(RuntimeError, match="no CPU path"):
        pw.wide_pointwise_conv3d(x, "weight")
    # the channel ranges (a tensor that answers is_cuda with True gets as far as the shape checks without a GPU)
    d = torch.device("cuda:0") if torch.cuda.is_available() else None
    z = (lambda *s: torch.zeros(s, device=d)) if d is not None else (lambda *s: cf.on_device(torch.zeros(s)))
    for cin, cout in ((2, 64), (2, 257), (17, 72), (2, 1)):
        with pytest.raises(ValueError, match="1 to 16 input and 65 to 256 output channels"):
            pw.wide_pointwise_conv3d(z(1, cin, 3, 3, 3), z(cout, cin, 1, 1, 1))
    with pytest.raises(ValueError, match="1 to 64"):
        pw.pointwise_conv3d(z(1, 2, 3, 3, 3), z(65, 2, 1, 1, 1))
    if d is not None:
        with pytest.raises(RuntimeError, match="bias is .*no CPU path"):
            pw.wide_pointwise_conv3d(x.to(d), w.to(d), b)
        for xs, ws, bs in (((1, 2, 3, 3), (72, 2, 1, 1, 1), None), ((1, 2, 0, 3, 3), (72, 2, 1, 1, 1), None),
                           ((1, 2, 3, 3, 3), (72, 2, 3, 3, 3), None), ((1, 2, 3, 3, 3), (72, 3, 1, 1, 1), None),
                           ((1, 2, 3, 3, 3), (72, 2, 1, 1, 1), (5,)), ((1, 2, 3, 3, 3), (72, 2, 1, 1), None)):
            with pytest.raises(ValueError):
                pw.wide_pointwise_conv3d(torch.zeros(xs, device=d), torch.zeros(ws, device=d),
                                         None if bs is None else torch.zeros(bs, device=d))


@pytest.mark.parametrize("case", wc.ALL)
def test_every_cases_yardstick_is_under_the_ceiling(case):
    assert pw.wide_pointwise_conv3d is not None
    r = wc.reference(case)
    assert ("db" in r["ref_err"]) == wc.has_bias(case)
    for q in wc.quantities(case):
        assert r["ref_err"][q] <= wc.REF_ERR_CEILING, (case, q, r["ref_err"][q])
    B, cin, cout, _, _ = wc.CASES[case]["shape"]
    assert 1 <= cin <= pw.WIDE_MAX_CIN and pw.WIDE_MIN_COUT <= cout <= pw.WIDE_MAX_COUT


def test_a_cpu_stem_with_128_output_channels_is_torchs_composition_bit_for_bit_whatever_the_switch(switches):
    assert hasattr(enc, "_wide_pointwise_routed")
    torch.manual_seed(31)
    m = enc.MultiLayer3DEncoderShallow(out_channels=128).train()
    x = torch.randn(2, 10, 12, 12, 12, generator=torch.Generator().manual_seed(32))
    state = {k: v.clone() for k, v in m.state_dict().items()}
    assert len(state) == 62 and tuple(m.conv_out.weight.shape) == (128, 8, 1, 1, 1)
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
    m = enc.MultiLayer3DEncoderShallow(out_channels=128)
    x = torch.zeros(1, 8, 4, 4, 4)
    switches(pointwise=True)
    # a CPU tensor, whatever the convolution
    assert not enc._wide_pointwise_routed(m.conv_out, x)
    assert not enc._wide_pointwise_routed(m.conv_out, "x")
    others = {"3x3x3": nn.Conv3d(8, 128, 3, padding=1), "strided": nn.Conv3d(8, 128, 1, stride=2),
              "padded": nn.Conv3d(8, 128, 1, padding=1), "groups": nn.Conv3d(8, 128, 1, groups=2),
              "dilated 3x3x3": nn.Conv3d(8, 128, 3, padding=2, dilation=2), "circular": nn.Conv3d(8, 128, 1, padding_mode="circular"),
              "64 channels": nn.Conv3d(8, 64, 1), "257 channels": nn.Conv3d(8, 257, 1), "other input channels": nn.Conv3d(4, 128, 1),
              "fp64 weight": nn.Conv3d(8, 128, 1).double()}
    if torch.cuda.is_available():
        d = torch.device("cuda:0")
        xd, real = x.to(d), True
        m.to(d)
        others = {k: c.to(d) for k, c in others.items()}
        others["weight on the host"] = nn.Conv3d(8, 128, 1)
        x17, c17 = torch.zeros(1, 17, 4, 4, 4, device=d), nn.Conv3d(17, 128, 1).to(d)
        x16, c16 = torch.zeros(1, 16, 4, 4, 4, device=d), nn.Conv3d(16, 256, 1).to(d)
    else:
        xd, real = _OnDevice(x), False   # (the module's weights stay where they are: their device is compared with x's)
        x17, c17 = _OnDevice(torch.zeros(1, 17, 4, 4, 4)), nn.Conv3d(17, 128, 1)
        x16, c16 = _OnDevice(torch.zeros(1, 16, 4, 4, 4)), nn.Conv3d(16, 256, 1)
        other = nn.Conv3d(8, 128, 1)
        other.weight = nn.Parameter(torch.empty(128, 8, 1, 1, 1, device="meta"))   # another device, where there is only the host
        others["weight on another device"] = other
    assert enc._wide_pointwise_routed(m.conv_out, xd), "conv_out itself is eligible"
    assert enc._wide_pointwise_routed(c16, x16), "16 -> 256: both limits"
    assert not enc._wide_pointwise_routed(c17, x17), "17 input channels"
    for name, conv in others.items():
        assert not enc._wide_pointwise_routed(conv, xd), name
    x64 = xd.double() if real else _OnDevice(x.double())
    assert not enc._wide_pointwise_routed(m.conv_out, x64), "fp64"
    x4 = xd[0] if real else _OnDevice(x[0])
    assert not enc._wide_pointwise_routed(m.conv_out, x4), "4-D"
    empty = torch.zeros(1, 8, 0, 4, 4)
    assert not enc._wide_pointwise_routed(m.conv_out, empty.to(xd.device) if real else _OnDevice(empty)), "empty"
    # the switches: POINTWISE = False and FORCE = False switch it off; FORCE = True and CONV = True do not switch it on
    for kw, want in ((dict(pointwise=True), True), (dict(pointwise=False), False), (dict(pointwise=True, force=False), False),
                     (dict(pointwise=None, force=False), False), (dict(pointwise=True, force=True, conv=False), True),
                     (dict(pointwise=None, force=True, conv=True), enc.wide_pointwise_site(8, 128, 64))):
        switches(**kw)
        assert enc._wide_pointwise_routed(m.conv_out, xd) == want, kw
    # the narrow op's route and the convolutions' own leave the 128-channel conv_out alone
    switches(pointwise=True, conv=True)
    assert not enc._pointwise_routed(m.conv_out, xd)
    assert not enc._conv_routed(m.conv_out, xd, False)
    # and the wide route leaves the 64-channel one to the narrow op
    m64 = enc.MultiLayer3DEncoderShallow()
    if real:
        m64.to(xd.device)
    assert enc._pointwise_routed(m64.conv_out, xd) and not enc._wide_pointwise_routed(m64.conv_out, xd)


def test_the_switch_follows_the_rule_at_import():
    assert enc.POINTWISE is None and enc.FORCE is None and enc.CONV is None
    assert enc.WIDE_POINTWISE_CHANNELS == (8, 128)


def test_the_routing_rule_matches_the_committed_measurement():
    """profiles/wide_pointwise_bench.json (scripts/bench_wide_pointwise.py on an MI355X): wide_pointwise_site() routes a shape ONLY
    where the op won all four (pass, form) pairs, and nothing smaller than the smallest measured winner or at channel counts nobody
    measured."""
    with open(os.path.join(ROOT, "profiles", "wide_pointwise_bench.json")) as f:
        bench = json.load(f)
    assert sorted(bench["shapes"]) == sorted(BENCH_SHAPES)
    routed, smallest = [], None
    for name, v in bench["shapes"].items():
        won = cf.op_wins(v)
        assert won == v["op_wins"] == bench["routing_as_measured"][name], name
        assert (v["cin"], v["cout"]) == (8, 128) and v["values_per_channel"] == v["side"] ** 3
        rule = enc.wide_pointwise_site(v["cin"], v["cout"], v["values_per_channel"])
        assert bench["routing_in_the_package"][name] == rule, name
        if rule:
            assert won, name
            routed.append(name)
            smallest = v["values_per_channel"] if smallest is None else min(smallest, v["values_per_channel"])
        for side in ("op", "torch", "halves"):
            assert set(v["passes_us"][side]) == {"forward", "backward_data", "backward_weight_bias"}, name
        for p in ("forward", "forward_backward"):
            for form in ("eager", "graph"):
                assert set(v[p][form]) >= {"op", "torch", "torch_benchmark", "halves"}, (name, p, form)
                assert all({"q1_us", "median_us", "q3_us"} <= set(v[p][form][s]) for s in ("op", "torch", "torch_benchmark", "halves"))
    assert sorted(routed) == sorted(bench["routed_shapes"])
    assert enc.WIDE_POINTWISE_MIN_VALUES == smallest
    for values in (1, 8, 1000, 12 ** 3):   # nothing below the smallest measured winner
        if smallest is None or values < smallest:
            assert not enc.wide_pointwise_site(8, 128, values), values
    for cin, cout in ((8, 64), (8, 96), (10, 128), (16, 256), (8, 256), (1, 65)):   # nothing at channel counts nobody measured
        assert not enc.wide_pointwise_site(cin, cout, 100 ** 3), (cin, cout)
    assert re.fullmatch(r"[0-9a-f]{16}", bench["build_id"])
    stem = bench["stem"]["forward_backward"]
    assert set(stem["eager"]) >= {"rule", "wide_off", "all_torch"} and set(stem["graph"]) >= {"rule", "wide_off", "all_torch"}
    assert enc.POINTWISE is None


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
dev = cf.dev


@gpu
@pytest.mark.parametrize("case", wc.ALL)
def test_every_case_forward_and_all_gradients(case):
    cf.check_case(FAMILY, case)


@gpu
@pytest.mark.parametrize("case", ["odd", "first_wide", "in_16", "stem_out_128_batch", "long_sum_stem"])
def test_the_same_bits_across_two_runs_and_across_splits(case):
    assert FAMILY.splits == (1, 2, 7, 64)
    cf.check_same_bits(FAMILY, case)


@gpu
@pytest.mark.parametrize("case", ["odd", "in_10", "top"])
def test_only_the_requested_gradients_are_computed(case, monkeypatch):
    """dx alone: dw and db are passed as null, and it is the forward's kernel on the transposed weight, a chain per 8 output channels
    added in ascending order -- the order in which the fused kernel's blocks and waves form dx: the same bits."""
    cf.check_requested_gradients(FAMILY, case, monkeypatch)


@gpu
def test_non_contiguous_and_offset_views_give_the_contiguous_result():
    cf.check_views(FAMILY, "odd")


@gpu
def test_the_stem_with_conv_out_128_routed_against_torchs_path(switches, monkeypatch):
    """[1,10,12,12,12], out_channels = 128: the same module with conv_out routed and not; the truth is the module in float64 on the
    CPU, the yardstick torch's fp32 path on the GPU.  That the kernels ran is read off the library calls, not off differing bits."""
    d = dev()
    torch.manual_seed(41)
    m = enc.MultiLayer3DEncoderShallow(out_channels=128).to(d)
    state = {k: v.clone() for k, v in m.state_dict().items()}
    assert len(state) == 62
    gen = torch.Generator().manual_seed(42)
    x = torch.randn(1, 10, 12, 12, 12, generator=gen).to(d)
    g_out, g_v1, g_v2 = (torch.randn(*s, generator=gen).to(d) for s in ((1, 128, 12, 12, 12), (1, 32, 3, 3, 3), (1, 16, 6, 6, 6)))
    calls = cf.count_calls(monkeypatch, FAMILY)
    narrow = cf.count_calls(monkeypatch, cf.FAMILIES["pointwise"])

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
    cf.compare_modules("stem 128", "torch's fp32 path", truth, torchs, routed)
    # the rule leaves a 12^3 volume to torch
    del calls[:]
    once(None, torch.float32, d)
    assert calls == [] and narrow == []


POISONED = ("first_wide", "stem_out_128_batch", "long_sum_stem")
_CLEAN = {}


@gpu
@pytest.mark.parametrize("byte", poison.BYTES)
@pytest.mark.parametrize("case", POISONED)
def test_poisoned_workspace_and_results_give_the_clean_runs_bits(case, byte, monkeypatch):
    """Every split and every combination of requested gradients with the workspace and every torch.empty result holding `byte`: the
    bits of the clean all-requested run in every requested quantity, None for a gradient not asked for (the form of
    test_poisoned_memory.test_conv_family).  A block after the first that read a dx element block 0 had not written would show here."""
    if case not in _CLEAN:
        _CLEAN[case] = cf.run(FAMILY, case)
    want = _CLEAN[case]
    fails, fetched, allocated = [], 0, 0
    for split in (0,) + tuple(FAMILY.splits):
        for need in list(cf.ALL_NEEDS) + [(True, True, True)]:
            with poison.poisoned(monkeypatch, byte) as p:
                got = cf.run(FAMILY, case, split=split, need=need)
            tag = f"{case} 0x{byte:02X} split {split} need {need}"
            if not same_bits(got["y"], want["y"]):
                fails.append((tag, "y"))
            for q, asked in zip(("dx", "dw", "db"), need):
                if not asked:
                    if got[q] is not None:
                        fails.append((tag, q, "not asked for and not None"))
                elif got[q] is None or not same_bits(got[q], want[q]):
                    n = -1 if got[q] is None else int((got[q].view(torch.int32) != want[q].view(torch.int32)).sum())
                    fails.append((tag, q, f"{n} elements differ"))
            assert p.allocations >= 1, tag
            fetched, allocated = fetched + p.workspaces, allocated + p.allocations
    print(f"{case}: {fetched} workspace fetches and {allocated} device allocations poisoned; {len(fails)} differences")
    assert not fails, fails[:20]
    assert fetched >= 1 and allocated >= 1


def _centre(shape, lead):
    """The flat index of the centre voxel of entry `lead` (a flat index over the two leading dimensions) of a 5-D tensor."""
    d, h, w = shape[2:]
    return lead * d * h * w + (d // 2) * h * w + (h // 2) * w + w // 2


def _taints(case):
    t = wc.make_inputs(case)
    taints = {}
    for k in ("x", "w", "g"):
        s = t[k].shape
        taints[k] = dict(centre_first=_centre(s, 0), centre_last=_centre(s, s[0] * s[1] - 1))
    taints["x"]["first"] = 0
    taints["g"]["last"] = t["g"].numel() - 1
    taints["b"] = dict(first=0, last=-1)
    return [(k, pos, index) for k, at in taints.items() for pos, index in at.items()]


@gpu
@pytest.mark.parametrize("case", ["first_wide", "in_16"])
def test_one_nan_or_infinity_in_one_operand_lands_where_torch_puts_it(case):
    """One NaN, +inf or -inf at one position of x, w, g or b: the class (finite, NaN, +inf, -inf) of every element of y, dx, dw and db
    is the float64 reference's, and the finite ones keep the bound (tests/nonfinite.py; free_share and ceiling as
    test_nonfinite._conv_subject sets them for the Conv3d families)."""
    inputs = {k: v for k, v in wc.make_inputs(case).items() if k in ("x", "w", "b", "g")}

    def ref(t, dtype):
        r = wc.torchs(t, dtype)
        return {q: r[q] for q in wc.quantities(case)}

    fails = []
    for operand, position, index in _taints(case):
        for name, value in nf.VALUES.items():
            tag = f"pointwise_wide {case} {operand}[{position}={index}]={name}"
            adm = nf.admit(tag, ref, inputs, operand, index, value, nf.FREE_SHARE, clean_key=("pointwise_wide", case))
            t = dict(inputs)
            t[operand] = nf.taint(t[operand], index, value)
            r = cf.run(FAMILY, case, **{k: v.to(dev()) for k, v in t.items() if v is not None})
            try:
                nf.compare({q: r[q] for q in wc.quantities(case)}, adm, ceiling=wc.REF_ERR_CEILING)
            except AssertionError as e:
                fails.append((tag, str(e)[:600]))
    assert not fails, fails


@gpu
def test_forward_and_backward_captured_into_a_hip_graph():
    """In a child process: stream capture is process-wide state (tests/tools/wide_pointwise_graph_capture_check.py)."""
    run_graph_tool("wide_pointwise_graph_capture_check.py", *FAMILY.graph_cases)


@gpu
def test_nothing_of_the_volumes_size_is_allocated_beside_the_results():
    """[1,8,128,50^3]: after one warm call a forward + backward allocates y, dx, dw and db (the workspace is the device's cached one)."""
    d = dev()
    gen = torch.Generator().manual_seed(51)
    x = torch.randn(1, 8, 50, 50, 50, generator=gen).to(d).requires_grad_(True)
    w = (torch.randn(128, 8, 1, 1, 1, generator=gen) * 8 ** -0.5).to(d).requires_grad_(True)
    b = torch.randn(128, generator=gen).to(d).requires_grad_(True)
    g = torch.randn(1, 128, 50, 50, 50, generator=gen).to(d)
    pw.wide_pointwise_conv3d(x, w, b).backward(g)   # (the cached workspace exists from here on)
    x.grad = w.grad = b.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    y = pw.wide_pointwise_conv3d(x, w, b)
    y.backward(g)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    results = 4 * (y.numel() + x.numel() + w.numel() + b.numel())
    print(f"results {results} bytes; forward + backward peak +{peak}")
    assert peak <= results + (1 << 20)
