"""The narrow-output 3x3x3 Conv3d with its pad folded into the addressing (manigaussian_amd/narrow.py, csrc/mgs_narrow.hip; the
Perceiver's trans_decoder) against torch's own F.conv3d(F.pad(...)) on the CPU (tests/narrow_conv_cases.py): float64 is the truth,
the float32 CPU run the yardstick,
    |ours - truth| <= 16 x max(yardstick, 2^-23) x max|truth|    for y, dx, dw and db of every case,
and one case of small integers whose every sum is exact: bit-equal to the truth.
"""
import importlib
import json
import os
import re

import pytest
import torch

import conv_family as cf
import narrow_conv_cases as nc
from manigaussian_amd import _lib, _ops
from manigaussian_amd import volume as vol

nw = importlib.import_module("manigaussian_amd.narrow")

gpu = pytest.mark.gpu
ROOT = cf.ROOT
FAMILY = cf.FAMILIES["narrow"]
BENCH_SHAPES = ("trans_decoder_100", "trans_decoder_50", "trans_decoder_25")


@pytest.fixture
def switch():
    """Sets volume.NARROW for one test and puts it back."""
    saved = vol.NARROW

    def set_(value):
        vol.NARROW = value
    yield set_
    vol.NARROW = saved


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
FAKE = cf.FAKE
SHAPE = ("B", "Cin", "Cout", "D", "H", "W", "zeros")
DEFAULTS = dict(B=1, Cin=4, Cout=2, D=5, H=6, W=7, zeros=0, x=FAKE, w=FAKE, bias=FAKE, y=FAKE, g=FAKE, dx=FAKE, dw=FAKE, db=FAKE, ws=FAKE)
_fwd = cf.fake_args("mgs_narrow_conv3d_forward", "mgs_narrow_conv3d_workspace_bytes", SHAPE, DEFAULTS, ("x", "w", "bias", "y"), SHAPE[:6])
_bwd = cf.fake_args("mgs_narrow_conv3d_backward", "mgs_narrow_conv3d_workspace_bytes", SHAPE, DEFAULTS,
                    ("x", "g", "w", "dx", "dw", "db", "ws", "ws_bytes", "split"), SHAPE[:6])


def test_the_library_refuses_bad_arguments_before_any_launch():
    """Every pointer is a fake address: a launch would fault.  Each refusal carries its message."""
    INV = _lib.MGS_ERR_INVALID_ARG
    shapes = ((dict(Cin=0), "1 to 256"), (dict(Cin=257), "1 to 256"), (dict(Cout=0), "1 to 4"), (dict(Cout=5), "1 to 4"),
              (dict(Cout=-1), "1 to 4"), (dict(B=0), "at least 1"), (dict(B=-3), "at least 1"), (dict(D=0), "at least 1"),
              (dict(H=0), "at least 1"), (dict(W=-2), "at least 1"), (dict(D=1 << 11, H=1 << 10, W=1 << 10), "2^31"),
              (dict(W=1 << 40), "2^31"), (dict(B=1 << 40), "tiles"), (dict(zeros=2), "zeros_pad"), (dict(zeros=-1), "zeros_pad"))
    # what a gradient needs beside these: w for dx, x for dw; and one of the three has to be asked for
    cf.check_refusals(_fwd, _bwd, shapes, required=(("x", "w", "y"), ("g", "ws")),
                      pointers=(("x", "w", "bias", "y"), ("x", "g", "w", "dx", "dw", "db", "ws")))
    need = _lib.lib().mgs_narrow_conv3d_workspace_bytes(1, 4, 2, 5, 6, 7)
    assert _bwd(ws_bytes=need - 1) == _lib.MGS_ERR_WORKSPACE and "needed" in _lib.last_error()
    assert _bwd(dw=None, db=None, ws_bytes=need - 1, split=65) == INV, "the split is checked even where dx alone is asked for"


def test_the_workspace_size_is_zero_for_illegal_shapes_and_follows_the_records_otherwise():
    W = _lib.lib().mgs_narrow_conv3d_workspace_bytes
    for a in ((0, 4, 2, 5, 6, 7), (1, 0, 2, 5, 6, 7), (1, 257, 2, 5, 6, 7), (1, 4, 0, 5, 6, 7), (1, 4, 5, 5, 6, 7), (1, 4, 2, 0, 6, 7),
              (1, 4, 2, 5, -1, 7), (1, 4, 2, 5, 6, 0), (1, 4, 2, 1 << 11, 1 << 10, 1 << 10), (1 << 40, 4, 2, 5, 6, 7), (-1, 4, 2, 5, 6, 7)):
        assert W(*a) == 0, a
    rec = 2 * (27 * 4 + 1) * 4
    assert rec <= W(1, 4, 2, nc.TILE_D, nc.TILE_H, nc.TILE_W) < rec + 512, "one tile: one record"
    assert 2 * rec <= W(1, 4, 2, nc.TILE_D, nc.TILE_H, nc.TILE_W + 1) < 2 * rec + 512, "two tiles: two records"
    assert 2 * rec <= W(1, 4, 2, nc.TILE_D + 1, nc.TILE_H, nc.TILE_W) < 2 * rec + 512
    assert 2 * rec <= W(2, 4, 2, 2, 2, 2) < 2 * rec + 512, "a tile never straddles batch entries"
    # 100^3 in tiles of 32 x 8 x 8: 4 x 13 x 13 = 676 tiles in runs of 11: 62 records; never more than 64, whatever the volume
    rec = (27 * 128 + 1) * 4
    assert 62 * rec <= W(1, 128, 1, 100, 100, 100) < 62 * rec + 512
    assert W(3, 128, 1, 400, 400, 400) <= nc.MAX_RUNS * rec + 512
    assert all(W(b, ci, co, d, 3, 5) % 256 == 0 and W(b, ci, co, d, 3, 5) > 0 for b in (1, 3) for ci in (1, 128, 256) for co in (1, 4)
               for d in (1, 13, 100))


def test_the_abi_version_is_still_17_and_the_new_names_match_the_ctypes_table():
    cf.check_abi(FAMILY.names)


def test_the_op_refuses_cpu_tensors_other_dtypes_and_bad_shapes():
    import manigaussian_amd as mg
    assert mg.narrow_conv3d is nw.narrow_conv3d
    x, w, b = torch.zeros(1, 2, 3, 3, 3), torch.zeros(1, 2, 3, 3, 3), torch.zeros(1)
    with pytest.raises(RuntimeError, match="narrow_conv3d needs float32 tensors on a HIP device .*no CPU path"):
        nw.narrow_conv3d(x, w, b)
    with pytest.raises(RuntimeError, match="no CPU path"):
        nw.narrow_conv3d(x.double(), w.double())
    with pytest.raises(RuntimeError, match="no CPU path"):
        nw.narrow_conv3d(x, "weight")
    if torch.cuda.is_available():
        d = torch.device("cuda:0")
        with pytest.raises(RuntimeError, match="bias is .*no CPU path"):
            nw.narrow_conv3d(x.to(d), w.to(d), b)
        with pytest.raises(RuntimeError, match="no CPU path"):
            nw.narrow_conv3d(x.to(d).double(), w.to(d).double())
        with pytest.raises(ValueError, match="padding_mode"):
            nw.narrow_conv3d(x.to(d), w.to(d), b.to(d), "circular")
        for xs, ws, bs in (((1, 2, 3, 3), (1, 2, 3, 3, 3), None), ((1, 2, 0, 3, 3), (1, 2, 3, 3, 3), None),
                           ((1, 2, 5, 5, 5), (1, 2, 5, 5, 5), None), ((1, 2, 3, 3, 3), (1, 3, 3, 3, 3), None),
                           ((1, 2, 3, 3, 3), (5, 2, 3, 3, 3), None), ((1, 257, 1, 1, 1), (1, 257, 3, 3, 3), None),
                           ((1, 2, 3, 3, 3), (2, 2, 3, 3, 3), (3,)), ((1, 2, 3, 3, 3), (1, 2, 1, 1, 1), None)):
            with pytest.raises(ValueError):
                nw.narrow_conv3d(torch.zeros(xs, device=d), torch.zeros(ws, device=d), None if bs is None else torch.zeros(bs, device=d))


@pytest.mark.parametrize("case", nc.ALL + ["exact"])
def test_every_cases_yardstick_is_under_the_ceiling(case):
    r = nc.reference(case)
    if case == "exact":   # every sum is exact: the float32 reference IS the truth
        assert all(v == 0.0 for v in r["ref_err"].values()), r["ref_err"]
        assert max(r[q + "64"].abs().max().item() for q in ("y", "dx", "dw", "db")) < 2 ** 24
        return
    assert ("db" in r["ref_err"]) == nc.has_bias(case)
    for q in nc.quantities(case):
        assert r["ref_err"][q] <= nc.REF_ERR_CEILING, (case, q, r["ref_err"][q])


def test_the_routing_rule_matches_the_committed_measurement():
    """profiles/narrow_conv_bench.json (scripts/bench_narrow.py on an MI355X): narrow_site() routes a shape ONLY where the op won all
    four (pass, form) pairs, and nothing smaller than the smallest measured winner or at channel counts nobody measured."""
    with open(os.path.join(ROOT, "profiles", "narrow_conv_bench.json")) as f:
        bench = json.load(f)
    assert sorted(bench["shapes"]) == sorted(BENCH_SHAPES)
    routed, smallest = [], None
    for name, v in bench["shapes"].items():
        won = cf.op_wins(v)
        assert won == v["op_wins"] == bench["routing_as_measured"][name], name
        assert (v["cin"], v["cout"]) == (128, 1) and v["voxels"] == v["side"] ** 3
        rule = vol.narrow_site(v["cin"], v["cout"], v["voxels"])
        assert bench["routing_in_the_package"][name] == rule, name
        if rule:
            assert won, name
            routed.append(name)
            smallest = v["voxels"] if smallest is None else min(smallest, v["voxels"])
        for side in ("op", "torch"):
            assert set(v["passes_us"][side]) == {"forward", "backward_data", "backward_weight_bias"}, name
        assert {"op", "torch", "torch_benchmark"} <= set(v["forward_backward"]["eager"]), name
        assert all("peak_bytes" in v["forward_backward"]["eager"][s] for s in ("op", "torch")), name
    assert sorted(routed) == sorted(bench["routed_shapes"])
    assert vol.NARROW_MIN_VOXELS == smallest
    for voxels in (1, 8, 1000, 12 ** 3):   # nothing below the smallest measured winner
        if smallest is None or voxels < smallest:
            assert not vol.narrow_site(128, 1, voxels), voxels
    for cin, cout in ((128, 2), (64, 1), (256, 4), (1, 1)):   # nothing at channel counts nobody measured
        assert not vol.narrow_site(cin, cout, 100 ** 3), (cin, cout)
    assert re.fullmatch(r"[0-9a-f]{16}", bench["build_id"])
    assert vol.NARROW is None


def test_the_switch_follows_the_rule_at_import():
    assert vol.NARROW is None


def test_a_cpu_block_is_todays_result_bit_for_bit_whatever_the_switch(switch):
    torch.manual_seed(61)
    m = vol.Conv3DBlock(128, 1, kernel_sizes=3, strides=1, norm=None, activation=None)
    assert sorted(m.state_dict()) == ["conv3d.bias", "conv3d.weight"]
    with torch.no_grad():
        m.conv3d.bias.normal_()
    x = torch.randn(1, 128, 4, 5, 6, generator=torch.Generator().manual_seed(62))
    got = []
    for value in (False, True, None):
        switch(value)
        m.zero_grad()
        xi = x.clone().requires_grad_(True)
        y = m(xi)
        y.pow(2).sum().backward()
        got.append([y.detach(), xi.grad, m.conv3d.weight.grad.clone(), m.conv3d.bias.grad.clone()])
        assert not vol._narrow_routed(m.conv3d, xi)
    want = m.conv3d(x)   # nn.Conv3d in replicate mode: what the block has always computed on a CPU
    assert torch.equal(got[0][0], want.detach())
    for other in got[1:]:
        assert all(torch.equal(a, b) for a, b in zip(got[0], other))


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
dev = cf.dev


@gpu
@pytest.mark.parametrize("case", nc.ALL)
def test_every_case_forward_and_all_gradients(case):
    cf.check_case(FAMILY, case)


@gpu
def test_the_exact_case_is_bit_equal_to_the_truth():
    r = nc.reference("exact")
    got = cf.run(FAMILY, "exact")
    for q in ("y", "dx", "dw", "db"):
        truth = r[q + "64"]
        wrong = int((got[q].double() != truth).sum())
        print(f"exact {q}: {wrong} of {truth.numel()} differ, max|truth| {truth.abs().max().item():.0f}")
        assert wrong == 0 and nc.same_bits(got[q], truth.float()), q


@gpu
@pytest.mark.parametrize("case", ["odd", "seams", "long_sum", "long_sum_head"])
def test_the_same_bits_across_two_runs_and_across_splits(case):
    cf.check_same_bits(FAMILY, case)


@gpu
@pytest.mark.parametrize("case", ["odd", "odd_zeros", "wide_in"])
def test_only_the_requested_gradients_are_computed(case, monkeypatch):
    """dx alone: dw, db and the workspace are passed as null."""
    cf.check_requested_gradients(FAMILY, case, monkeypatch)


@gpu
def test_non_contiguous_and_offset_views_give_the_contiguous_result():
    cf.check_views(FAMILY, "odd")


@gpu
@pytest.mark.parametrize("cout,activation", [(1, None), (2, "lrelu")])
def test_the_block_routed_against_the_same_module_not_routed(cout, activation, switch, monkeypatch):
    """Conv3DBlock(128, cout, 3) at 6 x 7 x 8: the truth is the module's nn.Conv3d and activation in float64 on the CPU, the yardstick the module's own path
    (resample_pad + F.conv3d) in fp32 on the GPU.  That the kernels ran is read off the library calls, not off differing bits."""
    d = dev()
    torch.manual_seed(71 + cout)
    m = vol.Conv3DBlock(128, cout, kernel_sizes=3, strides=1, norm=None, activation=activation).to(d)
    with torch.no_grad():
        m.conv3d.bias.normal_()
    state = {k: v.clone() for k, v in m.state_dict().items()}
    assert sorted(state) == ["conv3d.bias", "conv3d.weight"]
    gen = torch.Generator().manual_seed(72)
    x = torch.randn(1, 128, 6, 7, 8, generator=gen).to(d)
    g = torch.randn(1, cout, 6, 7, 8, generator=gen).to(d)
    calls = cf.count_calls(monkeypatch, FAMILY)
    pads = []
    real_call = _ops.call

    def spy(name, *a):
        if name.startswith("mgs_volume_resample_pad"):
            pads.append(name)
        return real_call(name, *a)
    monkeypatch.setattr(_ops, "call", spy)

    def once(narrow, dtype, where, as_list=False):
        switch(narrow)
        m.load_state_dict(state)
        m.to(where, dtype).zero_grad()
        xi = x.to(where, dtype).clone().requires_grad_(True)   # (a leaf of its own per run: .to() may hand x itself back)
        if dtype == torch.float64:   # (resample_pad is fp32 only: the block's own nn.Conv3d and activation, which is what it computes)
            y = m.conv3d(xi)
            y = m.activation(y) if m.activation is not None else y
        else:
            y = m([xi] if as_list else xi)
        (y * g.to(where, dtype)).sum().backward()
        r = {"y": y.detach(), "dx": xi.grad}
        r.update({"grad " + n: p.grad for n, p in m.named_parameters()})
        r = {k: v.detach().double().cpu().clone() for k, v in r.items()}
        m.to(d, torch.float32)
        return r

    truth = once(False, torch.float64, "cpu")
    del pads[:]
    torchs = once(False, torch.float32, d)
    assert calls == [] and len(pads) == 2, "NARROW = False: resample_pad forward and backward, then the module's own convolution"
    del pads[:]
    routed = once(True, torch.float32, d)
    assert calls == [("forward",), ("backward", True, True, True, True)], calls
    assert pads == [], "NARROW = True: the input is not padded first"
    cf.compare_modules(f"block {cout}", "the module's fp32 path", truth, torchs, routed)
    # a list input still takes the old path, and so does this shape under the rule: the existing tests run the code they ran before
    del calls[:], pads[:]
    once(True, torch.float32, d, as_list=True)
    assert calls == [] and len(pads) == 2
    del calls[:], pads[:]
    once(None, torch.float32, d)
    assert calls == [] and len(pads) == 2


@gpu
def test_forward_and_backward_captured_into_a_hip_graph():
    """In a child process: stream capture is process-wide state (tests/tools/conv_graph_capture_check.py)."""
    cf.graph_capture(FAMILY.name)


@gpu
def test_nothing_of_the_volumes_size_is_allocated_beside_the_results():
    """[1,128 -> 1,50^3]: after one warm call a forward + backward allocates y, dx, dw and db (the workspace is the device's cached
    one): no padded copy of the volume, and none of its gradient."""
    d = dev()
    gen = torch.Generator().manual_seed(81)
    x = torch.randn(1, 128, 50, 50, 50, generator=gen).to(d).requires_grad_(True)
    w = (torch.randn(1, 128, 3, 3, 3, generator=gen) * (27 * 128) ** -0.5).to(d).requires_grad_(True)
    b = torch.randn(1, generator=gen).to(d).requires_grad_(True)
    g = torch.randn(1, 1, 50, 50, 50, generator=gen).to(d)
    nw.narrow_conv3d(x, w, b).backward(g)   # (the cached workspace exists from here on)
    x.grad = w.grad = b.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    y = nw.narrow_conv3d(x, w, b)
    y.backward(g)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    results = 4 * (y.numel() + x.numel() + w.numel() + b.numel())
    print(f"results {results} bytes; forward + backward peak +{peak}")
    assert peak <= results + (1 << 20)
