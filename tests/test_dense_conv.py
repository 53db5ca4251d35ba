"""The dense 3x3x3 / 5x5x5 Conv3d with bias and leaky ReLU on the exact-f32 MFMA (manigaussian_amd/dense.py, csrc/mgs_dense.hip; the
Perceiver decoder's up0 and final) against torch's own F.conv3d (+ F.leaky_relu) on the CPU (tests/dense_conv_cases.py): float64 is
the truth, the float32 CPU run the yardstick,
    |ours - truth| <= 16 x max(yardstick, 2^-23) x max|truth|    for y, dx, dw and db of every case,
and two cases of small integers whose every sum is exact: bit-equal to the truth, which is what catches a dropped or misplaced tap
(one term of 16 000 is below the float bound).
"""
import importlib
import json
import os
import re

import pytest
import torch

import conv_family as cf
import dense_conv_cases as dc
from manigaussian_amd import _lib
from manigaussian_amd import volume as vol

dn = importlib.import_module("manigaussian_amd.dense")

gpu = pytest.mark.gpu
ROOT = cf.ROOT
FAMILY = cf.FAMILIES["dense"]
BENCH_SHAPES = ("up0_first_20", "up0_last_100", "up0_last_50", "final_100", "final_50")
SITES = {"up0_first": (256, 128, 5), "up0_last": (128, 128, 5), "final": (256, 128, 3)}


@pytest.fixture
def switch():
    """Sets volume.DENSE for one test and puts it back."""
    saved = vol.DENSE

    def set_(value):
        vol.DENSE = value
    yield set_
    vol.DENSE = saved


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
FAKE = cf.FAKE
SHAPE = ("B", "Cin", "Cout", "k", "D", "H", "W")
DEFAULTS = dict(B=1, Cin=8, Cout=32, k=3, D=5, H=6, W=7, slope=0.02, x=FAKE, y=FAKE, w=FAKE, bias=FAKE, g=FAKE, dx=FAKE, dw=FAKE, db=FAKE,
                scratch=FAKE, ws=FAKE)
_fwd = cf.fake_args("mgs_dense_conv3d_forward", "mgs_dense_conv3d_workspace_bytes", SHAPE, DEFAULTS,
                    ("slope", "x", "w", "bias", "y", "ws", "ws_bytes"))
_bwd = cf.fake_args("mgs_dense_conv3d_backward", "mgs_dense_conv3d_workspace_bytes", SHAPE, DEFAULTS,
                    ("slope", "x", "y", "g", "w", "dx", "dw", "db", "scratch", "ws", "ws_bytes", "split"))


def test_the_library_refuses_bad_arguments_before_any_launch():
    """Every pointer is a fake address: a launch would fault.  Each refusal carries its message."""
    INV = _lib.MGS_ERR_INVALID_ARG
    shapes = ((dict(Cin=0), "Cin"), (dict(Cin=12), "Cin"), (dict(Cin=264), "Cin"), (dict(Cin=-8), "Cin"), (dict(Cout=0), "Cout"),
              (dict(Cout=16), "Cout"), (dict(Cout=48), "Cout"), (dict(Cout=288), "Cout"), (dict(k=1), "3 or 5"), (dict(k=4), "3 or 5"),
              (dict(k=7), "3 or 5"), (dict(k=0), "3 or 5"), (dict(B=0), "at least 1"), (dict(B=-3), "at least 1"), (dict(D=2), "at least k"),
              (dict(H=0), "at least k"), (dict(W=-2), "at least k"), (dict(k=5, D=4), "at least k"),
              (dict(D=1 << 11, H=1 << 10, W=1 << 10), "2^31"), (dict(D=1289, H=1289, W=1289), "2^31"), (dict(W=1 << 40), "2^31"),
              (dict(B=1 << 40), "tiles"), (dict(B=65536), "tiles"), (dict(slope=float("nan")), "NaN"))
    # what a gradient needs beside these: w and the scratch for dx, x for dw; and one of the three has to be asked for
    cf.check_refusals(_fwd, _bwd, shapes, required=(("x", "w", "y", "ws"), ("g", "y", "ws", "scratch")),
                      pointers=(("x", "w", "bias", "y", "ws"), ("x", "y", "g", "w", "dx", "dw", "db", "scratch", "ws")))
    need = _lib.lib().mgs_dense_conv3d_workspace_bytes(1, 8, 32, 3, 5, 6, 7)
    for call in (_fwd, _bwd):
        assert call(ws_bytes=need - 1) == _lib.MGS_ERR_WORKSPACE and "needed" in _lib.last_error()
    assert _bwd(dw=None, db=None, ws_bytes=need - 1, split=65) == INV, "the split is checked even where dx alone is asked for"


def test_the_workspace_size_is_zero_for_illegal_shapes_and_follows_the_records_otherwise():
    W = _lib.lib().mgs_dense_conv3d_workspace_bytes
    for a in ((0, 8, 32, 3, 5, 6, 7), (1, 0, 32, 3, 5, 6, 7), (1, 12, 32, 3, 5, 6, 7), (1, 264, 32, 3, 5, 6, 7), (1, 8, 0, 3, 5, 6, 7),
              (1, 8, 48, 3, 5, 6, 7), (1, 8, 288, 3, 5, 6, 7), (1, 8, 32, 4, 5, 6, 7), (1, 8, 32, 5, 4, 6, 7), (1, 8, 32, 3, 2, 6, 7),
              (1, 8, 32, 3, 5, -1, 7), (1, 8, 32, 3, 5, 6, 0), (1, 8, 32, 3, 1 << 11, 1 << 10, 1 << 10), (1 << 40, 8, 32, 3, 5, 6, 7),
              (-1, 8, 32, 3, 5, 6, 7)):
        assert W(*a) == 0, a

    def parts(cin, cout, k):
        pad = lambda c: (c + dc.N_TILE - 1) // dc.N_TILE * dc.N_TILE   # noqa: E731
        weights = 4 * k ** 3 * max(cin * pad(cout), cout * pad(cin))   # the rearranged weights of the forward or of backward-data
        return weights, 4 * cout * (cin * k ** 3 + 1)

    wts, rec = parts(8, 32, 3)
    assert wts + rec <= W(1, 8, 32, 3, 3, 3, dc.W_SEG + 2) < wts + rec + 1024, "one segment: one record"
    assert wts + 2 * rec <= W(1, 8, 32, 3, 3, 3, dc.W_SEG + 3) < wts + 2 * rec + 1024, "a row one longer than a segment: two records"
    assert wts + 2 * rec <= W(1, 8, 32, 3, 3, 4, 5) < wts + 2 * rec + 1024, "two rows"
    assert wts + 2 * rec <= W(2, 8, 32, 3, 3, 3, 3) < wts + 2 * rec + 1024, "a segment never straddles batch entries"
    assert wts + dc.MAX_RUNS * rec <= W(2, 8, 32, 3, 42, 42, 42) < wts + dc.MAX_RUNS * rec + 1024, "small records: the most there are"
    assert W(3, 8, 32, 3, 400, 400, 400) < wts + dc.MAX_RUNS * rec + 1024
    # the sites: as many records as fit 128 MB, at least 8, never more than MAX_RUNS
    for (cin, cout, k), side in (((128, 128, 5), 100), ((256, 128, 3), 100), ((256, 128, 5), 20), ((256, 256, 5), 100)):
        wts, rec = parts(cin, cout, k)
        n = min(dc.MAX_RUNS, max(8, (128 << 20) // rec))
        got = W(1, cin, cout, k, side + k - 1, side + k - 1, side + k - 1)
        assert wts + n * rec <= got < wts + n * rec + 1024, (cin, cout, k, side, got)
    assert all(W(b, ci, co, k, d, 7, 9) % 256 == 0 and W(b, ci, co, k, d, 7, 9) > 0 for b in (1, 3) for ci in (8, 128, 256)
               for co in (32, 160, 256) for k in (3, 5) for d in (5, 13, 100))


def test_the_abi_version_is_still_17_and_the_new_names_match_the_ctypes_table():
    cf.check_abi(FAMILY.names)


def test_the_op_refuses_cpu_tensors_other_dtypes_and_bad_shapes():
    import manigaussian_amd as mg
    assert mg.dense_conv3d is dn.dense_conv3d
    x, w, b = torch.zeros(1, 8, 3, 3, 3), torch.zeros(32, 8, 3, 3, 3), torch.zeros(32)
    with pytest.raises(RuntimeError, match="dense_conv3d needs float32 tensors on a HIP device .*no CPU path"):
        dn.dense_conv3d(x, w, b)
    with pytest.raises(RuntimeError, match="no CPU path"):
        dn.dense_conv3d(x.double(), w.double())
    with pytest.raises(RuntimeError, match="no CPU path"):
        dn.dense_conv3d(x, "weight")
    if torch.cuda.is_available():
        d = torch.device("cuda:0")
        with pytest.raises(RuntimeError, match="bias is .*no CPU path"):
            dn.dense_conv3d(x.to(d), w.to(d), b)
        with pytest.raises(RuntimeError, match="no CPU path"):
            dn.dense_conv3d(x.to(d).double(), w.to(d).double())
        for slope in (-0.1, float("nan"), "lrelu"):
            with pytest.raises(ValueError, match="negative_slope"):
                dn.dense_conv3d(x.to(d), w.to(d), b.to(d), slope)
        for xs, ws, bs in (((1, 8, 3, 3), (32, 8, 3, 3, 3), None), ((1, 8, 0, 3, 3), (32, 8, 3, 3, 3), None),
                           ((1, 8, 7, 7, 7), (32, 8, 7, 7, 7), None), ((1, 8, 3, 3, 3), (32, 16, 3, 3, 3), None),
                           ((1, 8, 5, 5, 5), (32, 8, 3, 5, 3), None), ((1, 8, 3, 3, 3), (48, 8, 3, 3, 3), None),
                           ((1, 8, 3, 3, 3), (16, 8, 3, 3, 3), None), ((1, 12, 3, 3, 3), (32, 12, 3, 3, 3), None),
                           ((1, 264, 3, 3, 3), (32, 264, 3, 3, 3), None), ((1, 8, 3, 3, 3), (288, 8, 3, 3, 3), None),
                           ((1, 8, 3, 3, 3), (32, 8, 3, 3, 3), (31,)), ((1, 8, 4, 5, 5), (32, 8, 5, 5, 5), None),
                           ((1, 8, 3, 3, 2), (32, 8, 3, 3, 3), None), ((1, 8, 3, 3, 3), (32, 8, 1, 1, 1), None)):
            with pytest.raises(ValueError):
                dn.dense_conv3d(torch.zeros(xs, device=d), torch.zeros(ws, device=d), None if bs is None else torch.zeros(bs, device=d))


@pytest.mark.parametrize("case", dc.ALL + list(dc.EXACT))
def test_every_cases_yardstick_is_under_the_ceiling(case):
    r = dc.reference(case)
    if case in dc.EXACT:   # every sum is exact: the float32 reference IS the truth; results are multiples of 1/4 below 2^22
        assert all(v == 0.0 for v in r["ref_err"].values()), r["ref_err"]
        assert dc.exact_partial_sum_bound(case) < 2 ** 22
        assert r["z64"].abs().min().item() >= 0.5
        return
    assert ("db" in r["ref_err"]) == dc.has_bias(case)
    for q in dc.quantities(case):
        assert r["ref_err"][q] <= dc.REF_ERR_CEILING, (case, q, r["ref_err"][q])
    if dc.slope_of(case) is not None:   # no pre-activation near the activation's kink
        assert r["z64"].abs().min().item() >= dc.KINK, (case, r["seed"], r["z64"].abs().min().item())


def test_the_seam_cases_straddle_the_kernels_tiles():
    def shape(case):
        B, cin, cout, k, ext = dc.CASES[case]["shape"]
        return B, cin, cout, k, ext, ext[0] * ext[1] * ext[2]
    assert shape("m_seam")[5] == dc.M_TILE + 1 and shape("m_seam")[4][2] < dc.M_TILE and dc.M_TILE % shape("m_seam")[4][2]
    assert dc.N_TILE < 256 and shape("n_seam")[2] == dc.N_TILE + 32
    assert shape("k_seam")[1] == dc.K_SLAB + 8
    assert shape("row_seam")[4][2] == dc.W_SEG + 1
    B, cin, cout, k, ext, vox = shape("seams")
    assert k == 5 and B > 1 and vox > 2 * dc.M_TILE and vox % dc.M_TILE and cout > dc.N_TILE and cout % dc.N_TILE
    assert cin > 2 * dc.K_SLAB and dc.W_SEG < ext[2] < 2 * dc.W_SEG and (ext[2] + 4) * (ext[1] + 4) * (ext[0] + 4) % dc.M_TILE
    assert dc.W_NTILE == 128 and cin % 4 == 0   # 4 channels (k = 3) or 1 (k = 5) per N-tile of the weight gradient: cin of them
    assert [dc.CASES[c]["shape"][:4] for c in ("final_head", "up0_last_head", "up0_first_head")] == [(1,) + SITES[s] for s in
                                                                                                    ("final", "up0_last", "up0_first")]


def test_the_routing_rule_matches_the_committed_measurement():
    """profiles/dense_conv_bench.json (scripts/bench_dense.py on an MI355X): dense_site() routes a shape ONLY where the op won all four
    (pass, form) pairs, and nothing smaller than the smallest measured winner of its channel counts or at channel counts nobody
    measured."""
    with open(os.path.join(ROOT, "profiles", "dense_conv_bench.json")) as f:
        bench = json.load(f)
    assert sorted(bench["shapes"]) == sorted(BENCH_SHAPES)
    routed, smallest = [], {}
    for name, v in bench["shapes"].items():
        won = cf.op_wins(v, benchmark_may_be_missing=True)   # (the file records torch_benchmark children that did not finish)
        assert won == v["op_wins"] == bench["routing_as_measured"][name], name
        key = (v["cin"], v["cout"], v["k"])
        assert key == SITES[name.rsplit("_", 1)[0]] and v["voxels"] == v["side"] ** 3 and v["side"] == int(name.rsplit("_", 1)[1])
        rule = vol.dense_site(*key, v["voxels"])
        assert bench["routing_in_the_package"][name] == rule, name
        if rule:
            assert won, name
            routed.append(name)
            smallest[key] = min(smallest.get(key, v["voxels"]), v["voxels"])
        for side in ("op", "torch"):
            assert set(v["passes_us"][side]) == {"forward", "backward_data", "backward_weight_bias"}, name
        assert {"op", "torch"} <= set(v["forward_backward"]["eager"]), name
        assert all("peak_bytes" in v["forward_backward"]["eager"][s] for s in ("op", "torch")), name
        assert set(v["achieved_tflops"]) >= {"forward", "backward_data", "backward_weight_bias"}, name
    assert sorted(routed) == sorted(bench["routed_shapes"])
    assert vol.DENSE_MIN_VOXELS == smallest
    for key in SITES.values():   # nothing below the smallest measured winner
        for voxels in (1, 8, 1000, 12 ** 3):
            if key not in smallest or voxels < smallest[key]:
                assert not vol.dense_site(*key, voxels), (key, voxels)
    for key in ((128, 128, 3), (256, 256, 5), (64, 128, 5), (256, 128, 7), (8, 32, 3)):   # nothing at channel counts nobody measured
        assert not vol.dense_site(*key, 100 ** 3), key
    assert re.fullmatch(r"[0-9a-f]{16}", bench["build_id"])
    assert set(bench["decoder_segment"]) >= {"rule", "forced_on", "forced_off"}
    assert vol.DENSE is None


def test_the_switch_follows_the_rule_at_import():
    assert vol.DENSE is None


def test_a_cpu_block_is_todays_result_bit_for_bit_whatever_the_switch(switch):
    torch.manual_seed(61)
    m = vol.Conv3DBlock(8, 32, kernel_sizes=3, strides=1, norm=None, activation="lrelu")
    up = vol.Conv3DUpsampleBlock(8, 32, 2, kernel_sizes=3, norm=None, activation="lrelu")
    assert sorted(m.state_dict()) == ["conv3d.bias", "conv3d.weight"]
    assert sorted(up.state_dict()) == ["conv_up.0.conv3d.bias", "conv_up.0.conv3d.weight", "conv_up.2.conv3d.bias", "conv_up.2.conv3d.weight"]
    with torch.no_grad():
        m.conv3d.bias.normal_()
    x = torch.randn(1, 8, 4, 5, 6, generator=torch.Generator().manual_seed(62))
    for mod in (m, up):
        got = []
        for value in (False, True, None):
            switch(value)
            mod.zero_grad()
            xi = x.clone().requires_grad_(True)
            y = mod(xi)
            y.pow(2).sum().backward()
            got.append([y.detach(), xi.grad] + [p.grad.clone() for p in mod.parameters()])
            assert not vol._dense_routed(m.conv3d, xi)
        for other in got[1:]:
            assert all(torch.equal(a, b) for a, b in zip(got[0], other))
    want = m.activation(m.conv3d(x))   # nn.Conv3d in replicate mode: what the block has always computed on a CPU
    switch(True)
    assert torch.equal(m(x).detach(), want.detach())


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
dev = cf.dev


@gpu
@pytest.mark.parametrize("case", dc.ALL)
def test_every_case_forward_and_all_gradients(case):
    cf.check_case(FAMILY, case)


@gpu
@pytest.mark.parametrize("case", list(dc.EXACT))
def test_the_exact_cases_are_bit_equal_to_the_truth(case):
    r = dc.reference(case)
    got = cf.run(FAMILY, case)
    for q in ("y", "dx", "dw", "db"):
        truth = r[q + "64"]
        wrong = int((got[q].double() != truth).sum())
        print(f"{case} {q}: {wrong} of {truth.numel()} differ, max|truth| {truth.abs().max().item():.2f}")
        assert wrong == 0 and dc.same_bits(got[q], truth.float()), q


@gpu
@pytest.mark.parametrize("case", ["odd_k3", "seams", "long_sum", "long_sum_head"])
def test_the_same_bits_across_two_runs_and_across_splits(case):
    cf.check_same_bits(FAMILY, case)


@gpu
@pytest.mark.parametrize("case", ["odd_k3", "odd_k5", "plain"])
def test_only_the_requested_gradients_are_computed(case, monkeypatch):
    """dx alone: dw and db are passed as null; no dx: no padded gradient is allocated."""
    cf.check_requested_gradients(FAMILY, case, monkeypatch)


@gpu
def test_non_contiguous_and_offset_views_give_the_contiguous_result():
    cf.check_views(FAMILY, "odd_k3")


def _float64(module, x):
    """The block in float64 on the CPU in torch's own modules (resample_pad is fp32 only): nn.Conv3d in replicate mode, the
    activation, nn.Upsample -- which is what the blocks compute."""
    def block(m, v):
        v = m.conv3d(v)
        return m.activation(v) if m.activation is not None else v
    if isinstance(module, vol.Conv3DBlock):
        return block(module, x)
    first, up, last = module.conv_up
    return block(last, up(block(first, x)))


@gpu
@pytest.mark.parametrize("which", ["final", "up0"])
def test_the_block_routed_against_the_same_module_not_routed(which, switch, monkeypatch):
    """Conv3DBlock(256, 128, 3, lrelu) at 4 x 5 x 6 and Conv3DUpsampleBlock(128, 128, 2, kernel_sizes=5, lrelu) at 3 x 3 x 4: the truth
    is the module in float64 on the CPU, the yardstick the module's own path (resample_pad + F.conv3d + the activation) in fp32 on the
    GPU.  That the kernels ran is read off the library calls, not off differing bits."""
    d = dev()
    torch.manual_seed(91)
    if which == "final":
        m, cin, ext, n = vol.Conv3DBlock(256, 128, kernel_sizes=3, strides=1, norm=None, activation="lrelu"), 256, (4, 5, 6), 1
        out_ext = ext
    else:
        m, cin, ext, n = vol.Conv3DUpsampleBlock(128, 128, 2, kernel_sizes=5, norm=None, activation="lrelu"), 128, (3, 3, 4), 2
        out_ext = tuple(2 * e for e in ext)
    m = m.to(d)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("bias"):
                p.normal_()
    state = {k: v.clone() for k, v in m.state_dict().items()}
    gen = torch.Generator().manual_seed(92)
    x = torch.randn(1, cin, *ext, generator=gen).to(d)
    g = torch.randn(1, 128, *out_ext, generator=gen).to(d)
    calls = cf.count_calls(monkeypatch, FAMILY)

    def once(dense, dtype, where):
        switch(dense)
        m.load_state_dict(state)
        m.to(where, dtype).zero_grad()
        xi = x.to(where, dtype).clone().requires_grad_(True)   # (a leaf of its own per run: .to() may hand x itself back)
        y = _float64(m, xi) if dtype == torch.float64 else m(xi)
        (y * g.to(where, dtype)).sum().backward()
        r = {"y": y.detach(), "dx": xi.grad}
        r.update({"grad " + k: p.grad for k, p in m.named_parameters()})
        r = {k: v.detach().double().cpu().clone() for k, v in r.items()}
        m.to(d, torch.float32)
        return r

    truth = once(False, torch.float64, "cpu")
    torchs = once(False, torch.float32, d)
    assert calls == [], "DENSE = False: the module's own convolution"
    routed = once(True, torch.float32, d)
    assert calls == [("forward",)] * n + [("backward", True, True, True, True)] * n, calls
    cf.compare_modules(f"block {which}", "the module's fp32 path", truth, torchs, routed)
    # under the rule these toy shapes take today's path: the existing tests run the code they ran before
    del calls[:]
    once(None, torch.float32, d)
    assert calls == []


@gpu
def test_a_block_without_padding_and_one_with_another_activation_reach_the_op(switch, monkeypatch):
    d = dev()
    torch.manual_seed(93)
    calls = cf.count_calls(monkeypatch, FAMILY)
    x = torch.randn(1, 8, 5, 6, 7, generator=torch.Generator().manual_seed(94)).to(d)
    for activation, padding in (("relu", 0), ("tanh", None), (None, 0)):
        m = vol.Conv3DBlock(8, 32, kernel_sizes=3, strides=1, norm=None, activation=activation, padding=padding).to(d)
        switch(False)
        want = m(x)
        assert calls == []
        switch(True)
        got = m(x)
        assert calls == [("forward",)], (activation, padding)
        del calls[:]
        assert got.shape == want.shape
        assert (got - want).abs().max().item() <= 1e-5 * max(want.abs().max().item(), 1.0), (activation, padding)


@gpu
def test_forward_and_backward_captured_into_a_hip_graph():
    """In a child process: stream capture is process-wide state (tests/tools/conv_graph_capture_check.py)."""
    cf.graph_capture(FAMILY.name)


@gpu
def test_one_padded_gradient_is_all_that_is_allocated_beside_the_results():
    """[1, 128 -> 128, k 5, 36^3 -> 32^3]: after one warm call a forward + backward allocates y, dx, dw and db and ONE temporary of the
    padded output gradient's size (the workspace is the device's cached one)."""
    d = dev()
    gen = torch.Generator().manual_seed(95)
    x = torch.randn(1, 128, 36, 36, 36, generator=gen).to(d).requires_grad_(True)
    w = (torch.randn(128, 128, 5, 5, 5, generator=gen) * (125 * 128) ** -0.5).to(d).requires_grad_(True)
    b = torch.randn(128, generator=gen).to(d).requires_grad_(True)
    g = torch.randn(1, 128, 32, 32, 32, generator=gen).to(d)
    dn.dense_conv3d(x, w, b, 0.02).backward(g)   # (the cached workspace exists from here on)
    x.grad = w.grad = b.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    y = dn.dense_conv3d(x, w, b, 0.02)
    y.backward(g)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    results = 4 * (y.numel() + x.numel() + w.numel() + b.numel())
    padded = 4 * 128 * 40 ** 3
    print(f"results {results} bytes, the padded gradient {padded}; forward + backward peak +{peak}")
    assert peak <= results + padded + (1 << 20)
