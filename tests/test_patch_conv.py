"""The patch-embedding Conv3d (kernel = stride) with its pad folded in and bias and ReLU / leaky ReLU fused, on the exact-f32 MFMA
(manigaussian_amd/patch.py, csrc/mgs_patch.hip; the Perceiver's patchify) against torch's own act(F.conv3d(F.pad(...), stride=k)) on
the CPU (tests/patch_conv_cases.py): float64 is the truth, the float32 CPU run the yardstick,
    |ours - truth| <= 16 x max(yardstick, 2^-23) x max|truth|    for y, dx, dw and db of every case,
and one case of small integers whose every sum is exact: bit-equal to the truth, which is what catches a dropped or misplaced tap.
"""
import importlib
import json
import os
import re

import pytest
import torch
import torch.nn.functional as F

import conv_family as cf
import patch_conv_cases as pc
from manigaussian_amd import _lib, _ops
from manigaussian_amd import volume as vol

pt = importlib.import_module("manigaussian_amd.patch")

gpu = pytest.mark.gpu
ROOT = cf.ROOT
FAMILY = cf.FAMILIES["patch"]   # (the workspace is passed where dw or db is asked for)
BENCH_SHAPES = {"patchify_100": (128, 128, 100), "patchify_50": (128, 128, 50), "patchify_25": (128, 128, 25), "peract_100": (64, 64, 100)}


@pytest.fixture
def switch():
    """Sets volume.PATCH for one test and puts it back."""
    saved = vol.PATCH

    def set_(value):
        vol.PATCH = value
    yield set_
    vol.PATCH = saved


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
FAKE = cf.FAKE
SHAPE = ("B", "Cin", "Cout", "k", "pad", "D", "H", "W", "zeros", "slope")
DEFAULTS = dict(B=1, Cin=8, Cout=32, k=3, pad=1, D=5, H=6, W=7, zeros=0, slope=0.0, x=FAKE, y=FAKE, w=FAKE, bias=FAKE, g=FAKE, dx=FAKE, dw=FAKE,
                db=FAKE, ws=FAKE)
QUERY = "mgs_patch_conv3d_workspace_bytes"
_fwd = cf.fake_args("mgs_patch_conv3d_forward", QUERY, SHAPE, DEFAULTS, ("x", "w", "bias", "y", "ws", "ws_bytes"), SHAPE[:8])
_bwd = cf.fake_args("mgs_patch_conv3d_backward", QUERY, SHAPE, DEFAULTS, ("x", "y", "g", "w", "dx", "dw", "db", "ws", "ws_bytes", "split"),
                    SHAPE[:8])


def test_the_family_record_matches_the_backwards_parameter_list():
    names = cf.parameters("mgs_patch_conv3d_backward")
    assert cf.backward_positions(FAMILY) == {"mgs_patch_conv3d_backward": tuple(names.index(p) for p in ("dx", "dw", "db", "workspace"))}
    assert names[:10] == ["B", "Cin", "Cout", "k", "pad", "Di", "Hi", "Wi", "zeros_pad", "negative_slope"]
    assert names[10:] == ["x", "y", "g_y", "w", "dx", "dw", "db", "workspace", "workspace_bytes", "split", "stream"]


def test_the_library_refuses_bad_arguments_before_any_launch():
    """Every pointer is a fake address: a launch would fault.  Each refusal carries its message."""
    INV = _lib.MGS_ERR_INVALID_ARG
    shapes = ((dict(Cin=0), "Cin"), (dict(Cin=12), "Cin"), (dict(Cin=264), "Cin"), (dict(Cin=-8), "Cin"), (dict(Cin=3), "Cin"),
              (dict(Cout=0), "Cout"), (dict(Cout=4), "Cout"), (dict(Cout=16), "Cout"), (dict(Cout=48), "Cout"), (dict(Cout=288), "Cout"),
              (dict(k=1), "2 to 5"), (dict(k=6), "2 to 5"), (dict(k=0), "2 to 5"), (dict(k=-3), "2 to 5"),
              (dict(pad=3), "pad"), (dict(pad=-1), "pad"), (dict(k=5, pad=5), "pad"), (dict(k=2, pad=2), "pad"),
              (dict(B=0), "at least 1"), (dict(B=-3), "at least 1"), (dict(D=0), "at least 1"), (dict(H=0), "at least 1"),
              (dict(W=-2), "at least 1"), (dict(k=5, pad=0, D=4), "no patch"), (dict(k=5, pad=1, W=2), "no patch"),
              (dict(D=1 << 11, H=1 << 10, W=1 << 10), "2^31"), (dict(D=1291, H=1291, W=1291), "2^31"), (dict(W=1 << 40), "2^31"),
              (dict(B=65535, k=2, pad=0, D=66, H=64, W=64), "2^31"), (dict(B=1 << 40), "tiles"), (dict(B=65536), "tiles"),
              (dict(zeros=2), "zeros_pad"), (dict(zeros=-1), "zeros_pad"), (dict(slope=float("nan")), "NaN"))
    # what a gradient needs beside these: w for dx, x for dw; and one of the three has to be asked for
    cf.check_refusals(_fwd, _bwd, shapes, required=(("x", "w", "y", "ws"), ("g", "y", "ws")),
                      pointers=(("x", "w", "bias", "y", "ws"), ("x", "y", "g", "w", "dx", "dw", "db", "ws")))
    need = _lib.lib().mgs_patch_conv3d_workspace_bytes(1, 8, 32, 3, 1, 5, 6, 7)
    for call in (_fwd, _bwd):
        assert call(ws_bytes=need - 1) == _lib.MGS_ERR_WORKSPACE and "needed" in _lib.last_error()
    assert _bwd(dw=None, db=None, ws_bytes=need - 1, split=65) == INV, "the split is checked even where dx alone is asked for"


def test_the_workspace_size_is_zero_for_illegal_shapes_and_follows_the_records_otherwise():
    W = _lib.lib().mgs_patch_conv3d_workspace_bytes
    for a in ((0, 8, 32, 3, 1, 5, 6, 7), (1, 0, 32, 3, 1, 5, 6, 7), (1, 12, 32, 3, 1, 5, 6, 7), (1, 264, 32, 3, 1, 5, 6, 7),
              (1, 3, 4, 5, 2, 10, 10, 10), (1, 8, 0, 3, 1, 5, 6, 7), (1, 8, 48, 3, 1, 5, 6, 7), (1, 8, 288, 3, 1, 5, 6, 7),
              (1, 8, 32, 1, 0, 5, 6, 7), (1, 8, 32, 6, 0, 6, 6, 7), (1, 8, 32, 3, 3, 5, 6, 7), (1, 8, 32, 3, -1, 5, 6, 7),
              (1, 8, 32, 5, 0, 4, 6, 7), (1, 8, 32, 3, 1, 5, -1, 7), (1, 8, 32, 3, 1, 5, 6, 0), (1, 8, 32, 3, 1, 1 << 11, 1 << 10, 1 << 10),
              (65535, 8, 32, 2, 0, 66, 64, 64), (1 << 40, 8, 32, 3, 1, 5, 6, 7), (65536, 8, 32, 3, 1, 5, 6, 7), (-1, 8, 32, 3, 1, 5, 6, 7)):
        assert W(*a) == 0, a

    def parts(cin, cout, k):
        pad = lambda c: (c + pc.N_TILE - 1) // pc.N_TILE * pc.N_TILE   # noqa: E731
        return 4 * k ** 3 * cin * pad(cout), 4 * cout * (cin * k ** 3 + 1)   # the forward's rearranged weights; one record

    def follows(got, cin, cout, k, records):
        wts, rec = parts(cin, cout, k)
        need = max(wts, records * rec)   # (the two share the bytes)
        return need <= got < need + 1024

    # [., 8 -> 128], k = 2, pad 0: a row of 2 W voxels is W patches; at 128 output channels one record outweighs the weights
    assert parts(8, 128, 2)[1] > parts(8, 128, 2)[0]
    assert follows(W(1, 8, 128, 2, 0, 2, 2, 2 * pc.M_TILE), 8, 128, 2, 1), "one tile: one record"
    assert follows(W(1, 8, 128, 2, 0, 2, 2, 2 * pc.M_TILE + 2), 8, 128, 2, 2), "one patch more than a tile: two records"
    assert follows(W(2, 8, 128, 2, 0, 2, 2, 2), 8, 128, 2, 2), "a tile never straddles batch entries"
    assert follows(W(2, 8, 32, 5, 2, 60, 60, 60), 8, 32, 5, 54), "108 tiles in runs of 2"
    assert follows(W(3, 8, 32, 2, 0, 200, 200, 200), 8, 32, 2, pc.MAX_RUNS), "small records: the most there are"
    # the sites: as many records as fit REC_BYTES, at least MIN_RUNS, never more than MAX_RUNS; 250 tiles in runs of 32 are 8 records
    assert follows(W(1, 128, 128, 5, 2, 100, 100, 100), 128, 128, 5, 8)
    for (cin, cout, k), side in (((128, 128, 5), 100), ((64, 64, 5), 100), ((256, 256, 5), 100), ((256, 256, 2), 64)):
        rec = parts(cin, cout, k)[1]
        most = min(pc.MAX_RUNS, max(pc.MIN_RUNS, pc.REC_BYTES // rec))
        tiles = -(-(((side + 2 * (k // 2) - k) // k + 1) ** 3) // pc.M_TILE)
        per = -(-tiles // min(tiles, most))
        assert follows(W(1, cin, cout, k, k // 2, side, side, side), cin, cout, k, -(-tiles // per)), (cin, cout, k)
    assert W(1, 256, 256, 5, 2, 100, 100, 100) <= 2 * parts(256, 256, 5)[1] + 1024, "the largest records: two of them"
    assert all(W(b, ci, co, k, p, d, 7, 9) % 256 == 0 and W(b, ci, co, k, p, d, 7, 9) > 0 for b in (1, 3) for ci in (8, 128, 256)
               for co in (32, 160, 256) for k, p in ((2, 0), (3, 1), (4, 3), (5, 2)) for d in (5, 13, 100))


def test_the_abi_version_is_still_17_and_the_new_names_match_the_ctypes_table():
    cf.check_abi(FAMILY.names)
    assert FAMILY.names == ("mgs_patch_conv3d_workspace_bytes", "mgs_patch_conv3d_forward", "mgs_patch_conv3d_backward")


def test_the_op_refuses_cpu_tensors_other_dtypes_and_bad_shapes():
    import manigaussian_amd as mg
    assert mg.patch_conv3d is pt.patch_conv3d
    x, w, b = torch.zeros(1, 8, 5, 5, 5), torch.zeros(32, 8, 5, 5, 5), torch.zeros(32)
    with pytest.raises(RuntimeError, match="patch_conv3d needs float32 tensors on a HIP device .*no CPU path"):
        pt.patch_conv3d(x, w, b)
    with pytest.raises(RuntimeError, match="no CPU path"):
        pt.patch_conv3d(x.double(), w.double())
    with pytest.raises(RuntimeError, match="no CPU path"):
        pt.patch_conv3d(x, "weight")
    if torch.cuda.is_available():
        d = torch.device("cuda:0")
        with pytest.raises(RuntimeError, match="bias is .*no CPU path"):
            pt.patch_conv3d(x.to(d), w.to(d), b)
        with pytest.raises(RuntimeError, match="no CPU path"):
            pt.patch_conv3d(x.to(d).double(), w.to(d).double())
        for slope in (-0.1, float("nan"), "relu"):
            with pytest.raises(ValueError, match="negative_slope"):
                pt.patch_conv3d(x.to(d), w.to(d), b.to(d), 0, "replicate", slope)
        with pytest.raises(ValueError, match="padding_mode"):
            pt.patch_conv3d(x.to(d), w.to(d), b.to(d), 0, "circular")
        for padding in (5, -1, 2.0, (2, 2, 2), True):
            with pytest.raises(ValueError, match="padding"):
                pt.patch_conv3d(x.to(d), w.to(d), b.to(d), padding)
        for xs, ws, bs, pad in (((1, 8, 5, 5), (32, 8, 5, 5, 5), None, 0), ((1, 8, 0, 5, 5), (32, 8, 5, 5, 5), None, 0),
                                ((1, 8, 7, 7, 7), (32, 8, 7, 7, 7), None, 0), ((1, 8, 6, 6, 6), (32, 8, 6, 6, 6), None, 0),
                                ((1, 8, 5, 5, 5), (32, 8, 1, 1, 1), None, 0), ((1, 8, 5, 5, 5), (32, 16, 5, 5, 5), None, 0),
                                ((1, 8, 5, 5, 5), (32, 8, 3, 5, 3), None, 0), ((1, 8, 5, 5, 5), (48, 8, 5, 5, 5), None, 0),
                                ((1, 8, 5, 5, 5), (16, 8, 5, 5, 5), None, 0), ((1, 12, 5, 5, 5), (32, 12, 5, 5, 5), None, 0),
                                ((1, 3, 5, 5, 5), (4, 3, 5, 5, 5), None, 2), ((1, 264, 5, 5, 5), (32, 264, 5, 5, 5), None, 0),
                                ((1, 8, 5, 5, 5), (288, 8, 5, 5, 5), None, 0), ((1, 8, 5, 5, 5), (32, 8, 5, 5, 5), (31,), 0),
                                ((1, 8, 4, 5, 5), (32, 8, 5, 5, 5), None, 0), ((1, 8, 5, 5, 2), (32, 8, 5, 5, 5), None, 1)):
            with pytest.raises(ValueError):
                pt.patch_conv3d(torch.zeros(xs, device=d), torch.zeros(ws, device=d), None if bs is None else torch.zeros(bs, device=d), pad)


@pytest.mark.parametrize("case", pc.ALL + ["exact"])
def test_every_cases_yardstick_is_under_the_ceiling(case):
    r = pc.reference(case)
    assert tuple(r["y64"].shape[2:]) == pc.out_extents(case)
    if case == "exact":   # every sum is exact: the float32 reference IS the truth; the results are multiples of 1/4 below 2^22
        assert all(v == 0.0 for v in r["ref_err"].values()), r["ref_err"]
        assert max(r[q + "64"].abs().max().item() for q in ("y", "dx", "dw", "db")) < 2 ** 22
        assert r["z64"].abs().min().item() >= 0.5
        return
    assert ("db" in r["ref_err"]) == pc.has_bias(case)
    for q in pc.quantities(case):
        assert r["ref_err"][q] <= pc.REF_ERR_CEILING, (case, q, r["ref_err"][q])
    if pc.slope_of(case) is not None:   # no pre-activation near the activation's kink
        assert r["z64"].abs().min().item() >= pc.KINK, (case, r["seed"], r["z64"].abs().min().item())


def test_the_cases_reach_what_they_are_there_for():
    assert [pc.out_extents(c) for c in ("one_patch", "one_voxel", "site_small", "odd", "k2", "k3", "k4_rest", "max_c", "row100", "long_sum")] == \
        [(1, 1, 1), (1, 1, 1), (2, 2, 2), (2, 3, 3), (3, 4, 4), (3, 3, 4), (2, 2, 2), (1, 1, 1), (1, 2, 20), (12, 12, 12)]
    assert pc.out_extents("exact") == (1, 2, 2)
    assert pc.patches("seam_m") == pc.M_TILE + 1 and pc.M_TILE % pc.out_extents("seam_m")[2]
    assert pc.N_TILE < 256 and pc.shape_of("seam_n")[2] == pc.N_TILE + 32
    assert pc.shape_of("seam_k")[1] == pc.K_SLAB + 8 and pc.shape_of("seam_cin")[1] == pc.CIN_GROUP + 8
    B, cin, cout, ext, k, pad = pc.shape_of("seams")
    assert B > 1 and cin > pc.CIN_GROUP and cin % pc.CIN_GROUP and cout > pc.N_TILE and cout % pc.N_TILE
    assert pc.patches("seams") > 2 * pc.M_TILE and pc.patches("seams") % pc.M_TILE and pc.M_TILE % pc.out_extents("seams")[2]
    assert pc.W_NTILE == 128 and all(c["shape"][1] % 4 == 0 for c in pc.CASES.values())   # 4, 2 or 1 channels per N-tile: cin of them
    # the uncovered voxels of site_small: 8 and 9 of each axis, 48.8 % of dx, exactly zero in the truth
    dx = pc.reference("site_small")["dx64"]
    uncovered = torch.ones(10, 10, 10, dtype=torch.bool)
    uncovered[:8, :8, :8] = False
    assert abs(uncovered.float().mean().item() - 0.488) < 1e-6 and (dx[0, :, uncovered] == 0).all() and (dx[0, :, ~uncovered] != 0).all()
    # long_sum: 2 x 54 tiles of patches in 54 records
    assert 2 * -(-pc.patches("long_sum") // pc.M_TILE) == 108


def _conv(cin=128, cout=128, k=5, stride=5, **kw):
    return torch.nn.Conv3d(cin, cout, k, stride, padding=kw.pop("padding", k // 2), padding_mode=kw.pop("padding_mode", "replicate"), **kw)


def test_the_route_declines_what_the_kernels_do_not_take(switch):
    switch(True)
    def volume(channels, *ext):
        return cf.on_device(torch.zeros(1, channels, *(ext or (10, 10, 10))))
    x = volume(128)
    relu = torch.nn.ReLU()
    assert vol._patch_routed(_conv(), x, relu) and vol._patch_routed(_conv(), x) and vol._patch_routed(_conv(), x, torch.nn.LeakyReLU(0.02))
    assert vol._patch_routed(_conv(padding_mode="zeros"), x, relu) and vol._patch_routed(_conv(64, 32, 2, 2, padding=1), volume(64), relu)
    assert not vol._patch_routed(_conv(), [x], relu), "a list of tensors"
    assert not vol._patch_routed(_conv(), torch.zeros(1, 128, 10, 10, 10), relu), "a CPU tensor"
    assert not vol._patch_routed(_conv(), x.double(), relu) and not vol._patch_routed(_conv().double(), x, relu)
    assert not vol._patch_routed(_conv(stride=1), x, relu) and not vol._patch_routed(_conv(stride=4), x, relu)
    assert not vol._patch_routed(_conv(stride=(5, 5, 1)), x, relu)
    assert not vol._patch_routed(torch.nn.Conv3d(128, 128, (5, 5, 3), (5, 5, 3), padding=1, padding_mode="replicate"), x, relu)
    assert not vol._patch_routed(_conv(k=6, stride=6), x, relu) and not vol._patch_routed(_conv(k=1, stride=1, padding=0), x, relu)
    assert not vol._patch_routed(_conv(k=2, stride=2, padding=0, dilation=2), x, relu)
    assert not vol._patch_routed(_conv(groups=2), x, relu)
    assert not vol._patch_routed(_conv(padding_mode="circular"), x, relu) and not vol._patch_routed(_conv(padding_mode="reflect"), x, relu)
    assert not vol._patch_routed(_conv(padding=(2, 2, 1)), x, relu) and not vol._patch_routed(_conv(padding=5), x, relu)
    assert not vol._patch_routed(torch.nn.Conv3d(128, 128, 5, 5, padding="valid"), x, relu), "a padding given as a string"
    assert not vol._patch_routed(_conv(3, 4), volume(3), relu), "tests/volume_cases.py's conv_k5_s5 stays on today's path"
    assert not vol._patch_routed(_conv(12, 32), volume(12), relu) and not vol._patch_routed(_conv(8, 48), volume(8), relu)
    assert not vol._patch_routed(_conv(8, 16), volume(8), relu) and not vol._patch_routed(_conv(64, 128), x, relu)
    assert not vol._patch_routed(_conv(padding=0), volume(128, 4, 10, 10), relu), "no patch fits"
    for activation in (torch.nn.Tanh(), torch.nn.ELU(), torch.nn.PReLU(), torch.nn.LeakyReLU(-0.1)):
        assert not vol._patch_routed(_conv(), x, activation), activation
    switch(False)
    assert not vol._patch_routed(_conv(), x, relu)
    switch(None)
    assert vol._patch_routed(_conv(), x, relu) == vol.patch_site(128, 128, 5, 1000)


def test_the_routing_rule_matches_the_committed_measurement():
    """profiles/patch_conv_bench.json (scripts/bench_patch.py on an MI355X): patch_site() routes a shape ONLY where the op won all four
    (pass, form) pairs, and nothing smaller than the smallest measured winner of its channel counts or at channel counts nobody
    measured."""
    with open(os.path.join(ROOT, "profiles", "patch_conv_bench.json")) as f:
        bench = json.load(f)
    assert sorted(bench["shapes"]) == sorted(BENCH_SHAPES)
    routed, smallest = [], {}
    for name, v in bench["shapes"].items():
        won = cf.op_wins(v, benchmark_may_be_missing=True)   # (the file records torch_benchmark children that did not finish)
        assert won == v["op_wins"] == bench["routing_as_measured"][name], name
        key = (v["cin"], v["cout"], v["k"])
        assert key + (v["side"],) == BENCH_SHAPES[name][:2] + (5, BENCH_SHAPES[name][2]) and v["voxels"] == v["side"] ** 3 and v["pad"] == 2
        rule = vol.patch_site(*key, v["voxels"])
        assert bench["routing_in_the_package"][name] == rule, name
        if rule:
            assert won, name
            routed.append(name)
            smallest[key] = min(smallest.get(key, v["voxels"]), v["voxels"])
        for side in ("op", "torch"):
            assert set(v["passes_us"][side]) == {"forward", "backward_data", "backward_weight_bias"}, name
        assert {"op", "torch", "torch_benchmark"} <= set(v["forward_backward"]["eager"]), name
        assert all("peak_bytes" in v["forward_backward"]["eager"][s] for s in ("op", "torch")), name
        assert set(v["achieved_tflops"]) >= {"forward", "backward_data", "backward_weight_bias"}, name
    assert sorted(routed) == sorted(bench["routed_shapes"])
    assert vol.PATCH_MIN_VOXELS == smallest
    for key in ((128, 128, 5), (64, 64, 5)):   # nothing below the smallest measured winner
        for voxels in (1, 8, 1000, 12 ** 3):
            if key not in smallest or voxels < smallest[key]:
                assert not vol.patch_site(*key, voxels), (key, voxels)
    for key in ((128, 128, 3), (256, 256, 5), (64, 128, 5), (128, 128, 7), (8, 32, 5), (3, 4, 5)):   # nothing at triples nobody measured
        assert not vol.patch_site(*key, 100 ** 3), key
    assert re.fullmatch(r"[0-9a-f]{16}", bench["build_id"])
    assert set(bench["patchify_block"]) >= {"rule", "forced_on", "forced_off"}
    assert vol.PATCH is None


def test_a_cpu_block_is_todays_result_bit_for_bit_whatever_the_switch(switch):
    torch.manual_seed(61)
    m = vol.Conv3DBlock(128, 128, kernel_sizes=5, strides=5, norm=None, activation="relu")
    assert sorted(m.state_dict()) == ["conv3d.bias", "conv3d.weight"]
    with torch.no_grad():
        m.conv3d.bias.normal_()
    x = torch.randn(1, 128, 10, 10, 12, generator=torch.Generator().manual_seed(62))
    got = []
    for value in (False, True, None):
        switch(value)
        m.zero_grad()
        xi = x.clone().requires_grad_(True)
        y = m(xi)
        y.pow(2).sum().backward()
        got.append([y.detach(), xi.grad, m.conv3d.weight.grad.clone(), m.conv3d.bias.grad.clone()])
        assert not vol._patch_routed(m.conv3d, xi, m.activation)
    c = m.conv3d   # torch's composition: what the block has always computed on a CPU
    want = F.relu(F.conv3d(F.pad(x, (2,) * 6, mode="replicate"), c.weight, c.bias, stride=5))
    assert got[0][0].shape == (1, 128, 2, 2, 3) and torch.equal(got[0][0], want.detach())
    for other in got[1:]:
        assert all(torch.equal(a, b) for a, b in zip(got[0], other))


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
dev = cf.dev


@gpu
@pytest.mark.parametrize("case", pc.ALL)
def test_every_case_forward_and_all_gradients(case):
    cf.check_case(FAMILY, case)


@gpu
def test_the_uncovered_voxels_gradient_is_exactly_zero(monkeypatch):
    """site_small: voxels 8 and 9 of each axis belong to no patch; the op writes their dx itself, into memory that held NaNs."""
    r, d = pc.reference("site_small"), dev()
    x = r["x"].to(d).requires_grad_(True)
    w, b = r["w"].to(d), r["b"].to(d)
    real_empty_like = torch.empty_like

    def poisoned(t, *a, **kw):
        return real_empty_like(t, *a, **kw).fill_(float("nan"))
    monkeypatch.setattr(torch, "empty_like", poisoned)
    pc.call("site_small", x, w, b).backward(r["g"].to(d))
    monkeypatch.undo()
    dx = x.grad.cpu()
    uncovered = torch.ones(10, 10, 10, dtype=torch.bool)
    uncovered[:8, :8, :8] = False
    assert not torch.isnan(dx).any() and (dx[0, :, uncovered] == 0).all() and (dx[0, :, ~uncovered] != 0).all()


@gpu
def test_the_exact_case_is_bit_equal_to_the_truth():
    r = pc.reference("exact")
    got = cf.run(FAMILY, "exact")
    for q in ("y", "dx", "dw", "db"):
        truth = r[q + "64"]
        wrong = int((got[q].double() != truth).sum())
        print(f"exact {q}: {wrong} of {truth.numel()} differ, max|truth| {truth.abs().max().item():.2f}")
        assert wrong == 0 and pc.same_bits(got[q], truth.float()), q


@gpu
@pytest.mark.parametrize("case", ["odd", "seams", "long_sum"])
def test_the_same_bits_across_two_runs_and_across_splits(case):
    cf.check_same_bits(FAMILY, case)


@gpu
@pytest.mark.parametrize("case", ["odd", "odd_zeros", "k3"])
def test_only_the_requested_gradients_are_computed(case, monkeypatch):
    """dx alone: dw, db and the workspace are passed as null; dx has the bits it has when everything is asked for."""
    cf.check_requested_gradients(FAMILY, case, monkeypatch)


@gpu
def test_non_contiguous_and_offset_views_give_the_contiguous_result():
    cf.check_views(FAMILY, "odd")


@gpu
def test_the_block_routed_against_the_same_module_not_routed(switch, monkeypatch):
    """Conv3DBlock(128, 128, 5, 5, relu) at 10 x 10 x 15: the truth is the module's nn.Conv3d and activation in float64 on the CPU, the
    yardstick the module's own path (resample_pad + F.conv3d(stride=5) + ReLU) in fp32 on the GPU.  That the kernels ran is read off the
    library calls, not off differing bits."""
    d = dev()
    torch.manual_seed(71)
    m = vol.Conv3DBlock(128, 128, kernel_sizes=5, strides=5, norm=None, activation="relu").to(d)
    with torch.no_grad():
        m.conv3d.bias.normal_()
    state = {k: v.clone() for k, v in m.state_dict().items()}
    assert sorted(state) == ["conv3d.bias", "conv3d.weight"]
    gen = torch.Generator().manual_seed(72)
    x = torch.randn(1, 128, 10, 10, 15, generator=gen).to(d)
    g = torch.randn(1, 128, 2, 2, 3, generator=gen).to(d)
    calls = cf.count_calls(monkeypatch, FAMILY)
    pads = []
    real_call = _ops.call

    def spy(name, *a):
        if name.startswith("mgs_volume_resample_pad"):
            pads.append(name)
        return real_call(name, *a)
    monkeypatch.setattr(_ops, "call", spy)

    def once(patch, dtype, where, as_list=False):
        switch(patch)
        m.load_state_dict(state)
        m.to(where, dtype).zero_grad()
        xi = x.to(where, dtype).clone().requires_grad_(True)   # (a leaf of its own per run: .to() may hand x itself back)
        if dtype == torch.float64:   # (resample_pad is fp32 only: the block's own nn.Conv3d and activation, which is what it computes)
            y = m.activation(m.conv3d(xi))
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
    assert calls == [] and len(pads) == 2, "PATCH = False: resample_pad forward and backward, then the module's own convolution"
    del pads[:]
    routed = once(True, torch.float32, d)
    assert calls == [("forward",), ("backward", True, True, True, True)], calls
    assert pads == [], "PATCH = True: the input is not padded first"
    assert routed["y"].shape == (1, 128, 2, 2, 3)
    cf.compare_modules("patchify block", "the module's fp32 path", truth, torchs, routed)
    # a list input still takes the old path, and so does this shape under the rule: the existing tests run the code they ran before
    del calls[:], pads[:]
    once(True, torch.float32, d, as_list=True)
    assert calls == [] and len(pads) == 2
    del calls[:], pads[:]
    once(None, torch.float32, d)
    assert calls == [] and len(pads) == 2
    # a state_dict round trip: the routed block is the same module
    other = vol.Conv3DBlock(128, 128, kernel_sizes=5, strides=5, norm=None, activation="relu").to(d)
    other.load_state_dict(m.state_dict(), strict=True)
    switch(True)
    with torch.no_grad():
        assert pc.same_bits(other(x).cpu(), m(x).cpu())


@gpu
def test_forward_and_backward_captured_into_a_hip_graph():
    """In a child process: stream capture is process-wide state (tests/tools/conv_graph_capture_check.py)."""
    cf.graph_capture(FAMILY.name)


@gpu
def test_nothing_of_the_volumes_size_is_allocated_beside_the_results():
    """[1, 128 -> 128, 50^3], k 5, pad 2: after one warm call a forward + backward allocates y, dx, dw and db (the workspace is the
    device's cached one): no padded copy of the volume, and none of its gradient."""
    d = dev()
    gen = torch.Generator().manual_seed(81)
    x = torch.randn(1, 128, 50, 50, 50, generator=gen).to(d).requires_grad_(True)
    w = (torch.randn(128, 128, 5, 5, 5, generator=gen) * (125 * 128) ** -0.5).to(d).requires_grad_(True)
    b = torch.randn(128, generator=gen).to(d).requires_grad_(True)
    g = torch.randn(1, 128, 10, 10, 10, generator=gen).to(d)
    pt.patch_conv3d(x, w, b, 2, "replicate", 0.0).backward(g)   # (the cached workspace exists from here on)
    x.grad = w.grad = b.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    y = pt.patch_conv3d(x, w, b, 2, "replicate", 0.0)
    y.backward(g)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    results = 4 * (y.numel() + x.numel() + w.numel() + b.numel())
    print(f"results {results} bytes; forward + backward peak +{peak}")
    assert peak <= results + (1 << 20)
