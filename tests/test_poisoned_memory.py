"""Every fused op reads only what it wrote in the same call: one clean run of an op, then the same call with its workspace and every
torch.empty / torch.empty_like result filled with 0xFF bytes (float32 NaN, int32 -1) and with 0x7F bytes (float32 3.3962e38, which
survives fmaxf and x > 0 ? x : 0 where a NaN does not; int32 2139062143) -- tests/poison.py.  Every returned tensor and every gradient
must have the clean run's bits and no non-finite element the clean run has not.  The reference is the clean run of the same op; what
the ops compute is the business of their own test files.  This is the test `_ops.workspace`'s docstring and the header of
csrc/mgs_records.hip name.

Not enrolled HERE: the rasterizer (_C.py, rasterizer.py, views.py).  Its binning buffers hold keys, offsets and counts that kernels use
as addresses, so a 0xFF fill could turn a stale read into an out-of-bounds access; tests/test_rasterizer_dirty_workspace.py holds it to
the same property with fills chosen by the kind of region (zeros, a donor call's bytes, 0xFF / 0x7F over the float regions only:
tests/dirty_workspace.py).  NOT_ENROLLED lists it and the other modules that call torch.empty without being an op.

Who writes and who first reads every region, read off the host code and the kernels before any of this ran on a GPU ("ws": the region
of `_ops.workspace`; "-": never read by a kernel):

op (module)           region                                 first writer                         first reader
--------------------  -------------------------------------  -----------------------------------  ------------------------------------
conv3d                ws records [nrec, Cout, Cin, 27]       cv_bwd_weight_kernel: every record   records_merge_kernel
                      y | dx | dw (empty, empty_like)        cv_fwd / cv_bwd_data_s2 | merge      -
pointwise             ws records [nrec, Cout, Cin + 1]       pw_bwd_kernel, one launch per 16     records_merge_kernel
                                                             input channels; the bias column by
                                                             the first launch
                      y | dx | dw, db                        pw_fwd_* | pw_bwd or pw_fwd | merge  -
narrow                ws records [nrec, Cout, 27 Cin + 1]    nc_bwd_weight_kernel; the dw         records_merge_kernel, which skips the
                                                             columns only when dw is asked for    columns of a gradient not asked for
                      y | dx | dw, db                        nc_fwd | nc_bwd_data | merge         -
dense                 ws weights [Cin k^3, Cout to 128]      dc_prep_kernel (padding: zeros)      dc_fwd_kernel
                      ws records [nrec, Cout, Cin k^3 + 1]   dc_bwd_weight_kernel (as narrow)     records_merge_kernel (as narrow)
                      g_scratch (empty): the padded g'       dc_pad_kernel: every element         dc_fwd_kernel (backward-data)
                      y | dx | dw, db                        dc_fwd | dc_fwd | merge              -
patch                 ws weights (forward)                   pc_prep_kernel                       pc_fwd_kernel
                      ws records (backward, the same bytes)  pc_bwd_weight_kernel (as narrow)     records_merge_kernel (as narrow)
                      y | dx | dw, db                        pc_fwd | pc_bwd_data, uncovered      -
                                                             voxels included | merge
spatial_softmax       ws records [rows, slices, 8]           ss_fwd_kernel: one per workgroup     ss_combine_kernel: slices per row
                      out [B, 4C], stats [rows, 6]           ss_combine_kernel                    stats: ss_bwd_kernel
                      g_feature                              ss_bwd_kernel                        -
attention             ws delta [B H Nq]                      attn_delta_kernel                    attn_dq_kernel, attn_dkv_kernel
                      out, lse                               attn_fwd_kernel                      attn_delta / dq / dkv (saved)
                      dq | dkv                               attn_dq_kernel | attn_dkv_kernel     -
encoder (abn)         ws records [rows, nsub, 4]             abn_stats_kernel | abn_bwd_sums      abn_apply_kernel | abn_bwd_dx_kernel
                                                             (every sub-slice of every row)       (abn_channel_merge)
                      y, stats [C, 2]                        abn_apply_kernel                     stats: abn_bwd_sums, abn_bwd_dx
                      dx, dwb [2, C]                         abn_bwd_dx_kernel                    -
feedforward           ws partial [slabs, 2, cols]            ln_bwd_kernel | geglu_bwd_kernel     ff_colsum_kernel: `slabs` rows
                      y, stats [rows, 2] | out               ln_fwd_kernel | geglu_fwd_kernel     stats: ln_bwd_kernel
                      dx | dh | dw, db                       ln_bwd | geglu_bwd | ff_colsum       -
volume                ws xy sums [B Ct, s D + 2 p, H, W]     vol_bwd_xy_kernel (scale > 1)        vol_bwd_z_kernel
                      (scale 1: fetched, neither written nor read: vol_bwd_copy_kernel reads g_out alone)
                      out | the sources' gradients           vol_fwd_kernel | vol_bwd_z / copy    -
augmentation          ws records [B, 16]                     se3_select_kernel: all 16 floats     se3_apply_kernel
                                                             of every sample, identity or not
                      out_trans, out_rot, info               se3_select_kernel                    -
                      clouds, poses                          se3_apply_kernel                     -
voxelizer             ws head [B V^3] and its padding        voxelize_clear_kernel (zeros), then  voxelize_mean_kernel, write kernels
                                                             atomicExch in voxelize_link_kernel
                      ws vid [B N]                           voxelize_link_kernel: EVERY point    voxelize_mean_kernel
                      ws next [B N]                          voxelize_link_kernel: kept points    voxelize_mean_kernel: list members
                      ws mean [B N, stride]                  voxelize_mean_kernel: the rows of    write kernels: row head - 1 of an
                                                             the list heads                       occupied voxel
                      grid                                   voxelize_write_cf / _cl_kernel       -
deform                out | g_lat, g_z | xyz, rot | g_delta  assemble fwd | bwd | apply fwd | bwd -
                      a, xb (_relu_bias)                     mgs_mlp_relu_bias                    (the GEMMs that follow)
regressor             the seven outputs | g_raw              epilogue forward | backward          -
voxel                 out [N, C + 3 + 6 K]                   voxel_sample_pe_fwd_kernel           -
                      (backward: torch.zeros and float atomics, no torch.empty and no bits to repeat: forward only here)
camera                wvt, fpt, centre, fov, tanfov          novel_calib kernel                   -
losses                buf: unit gradients | partials | mm    render_loss_fwd | fwd | minmax       bwd | finalize | fwd (l2_norm only)
                      | terms | loss; out_c, out_f           finalize | finalize; bwd             -
photometric           buf: unit | maps | partials            grad | fwd | fwd                     bwd | grad (with halo, inside the
                      | terms | loss; out                    finalize | finalize; bwd             image) | finalize
optim (FusedLamb)     ws partials [chunks] (its own empty)   lamb_moments_kernel                  lamb_apply_kernel
                      (m, v, statistics, the flat gradient and the tables are torch.zeros)

The voxelizer is the one op that keeps integers in its workspace.  voxelize_link_kernel runs one thread per point i < B N and stores
vid[i] = keep ? voxel : -1 unconditionally, before it looks at `keep`: out-of-bounds, NaN and infinite points included.  next[i] is
stored only for a kept point, by the same statement that pushes it on its voxel's list; voxelize_mean_kernel loads next[] only while
it walks a list from its head (vid[i] >= 0 and head[voxel] == p + 1), and a list holds nothing but points that pushed themselves, so
the next[] of a dropped point is never loaded.  head is cleared with its padding before the link launch and afterwards holds 0 or p + 1
<= N: the one word that becomes an address (row head - 1 of `mean`) is never stale.  The long-list path scans vid[0 .. N), all stored.
No region of any enrolled op is read before it is written in the same call.
"""
import importlib
import os
import re
import struct

import pytest
import torch

import abn_cases as ac
import attention_cases as atc
import conv_family as cf
import embed_cases as ec
import feedforward_cases as fc
import lamb_cases as lac
import loss_cases as lc
import patch_conv_cases as pc
import photometric_cases as phc
import poison
import se3_cases as sc3
import spatial_softmax_cases as ssc
import volume_cases as vc
import voxelize_cases as vz
from manigaussian_amd import _lib, _ops
from numerics import bits, same_bits

gpu = pytest.mark.gpu
ROOT = cf.ROOT
BYTES = poison.BYTES
FLOAT_7F = struct.unpack("<f", b"\x7f" * 4)[0]   # 3.3962e38
dev = cf.dev


def _mod(name):
    return importlib.import_module("manigaussian_amd." + name)


# ---- enrolment -----------------------------------------------------------------------------------------------------------------
# module -> the tests of this file that run it poisoned; the modules that call _ops.workspace(
WITH_WORKSPACE = {
    "conv3d": ["test_conv_family"], "pointwise": ["test_conv_family"], "narrow": ["test_conv_family"], "dense": ["test_conv_family"],
    "patch": ["test_conv_family"], "spatial_softmax": ["test_spatial_softmax"], "attention": ["test_attention"],
    "encoder": ["test_batch_norm_act"], "feedforward": ["test_layer_norm", "test_bias_geglu"], "volume": ["test_resample_pad"],
    "augmentation": ["test_se3_augmentation"], "voxelizer": ["test_voxelizer"],
}
# ... and the modules that only allocate results, or carve scratch out of a torch.empty buffer of their own
ALLOCATING = {
    "deform": ["test_deform"], "regressor": ["test_gaussian_epilogue"], "voxel": ["test_point_latent"], "camera": ["test_novel_calib"],
    "losses": ["test_rendering_loss"], "photometric": ["test_photometric_loss"], "optim": ["test_fused_lamb"],
}
NOT_ENROLLED = {
    "_C": "the rasterizer: its binning buffers hold keys, offsets and counts that kernels use as addresses; "
          "test_rasterizer_dirty_workspace.py dirties its workspaces and results with fills chosen by the kind of region",
    "parallel": "host staging buffers and communication results that a collective fills; no kernel of the library",
    "_ops": "the workspace's own allocation: what poisoned() fills",
    "_conv": "backward_begin allocates dx, dw and db for pointwise, narrow, dense and patch, which are enrolled",
}


def _sources():
    out = {}
    folder = os.path.join(ROOT, "manigaussian_amd")
    for name in sorted(os.listdir(folder)):
        if name.endswith(".py"):
            with open(os.path.join(folder, name)) as f:
                out[name[:-3]] = f.read()
    return out


def test_every_module_that_takes_a_workspace_or_allocates_a_result_is_enrolled_or_excused():
    src = _sources()
    takes = {m for m, s in src.items() if "_ops.workspace(" in s}
    assert takes == set(WITH_WORKSPACE), "a module calls _ops.workspace( and has no poisoned test (or the other way round)"
    assert takes == {"attention", "augmentation", "conv3d", "dense", "encoder", "feedforward", "narrow", "patch", "pointwise",
                     "spatial_softmax", "volume", "voxelizer"}
    allocates = {m for m, s in src.items() if re.search(r"\btorch\.empty(_like)?\(", s)}
    enrolled = set(WITH_WORKSPACE) | set(ALLOCATING)
    assert not enrolled & set(NOT_ENROLLED)
    assert allocates == enrolled | set(NOT_ENROLLED), sorted(allocates ^ (enrolled | set(NOT_ENROLLED)))
    assert set(NOT_ENROLLED) == {"_C", "parallel", "_ops", "_conv"} and all(NOT_ENROLLED.values())
    for tests in list(WITH_WORKSPACE.values()) + list(ALLOCATING.values()):
        for name in tests:
            marks = [m.name for m in getattr(globals()[name], "pytestmark", [])]
            assert "gpu" in marks and "parametrize" in marks, name


# ---- the wrappers, without a GPU -----------------------------------------------------------------------------------------------
def test_the_wrappers_leave_cpu_tensors_alone(monkeypatch):
    monkeypatch.setattr(torch, "empty", lambda *a, **kw: torch.zeros(*a, **kw))       # (what the wrapper then wraps: known contents)
    monkeypatch.setattr(torch, "empty_like", lambda *a, **kw: torch.zeros_like(*a, **kw))
    with poison.poisoned(monkeypatch, 0xFF) as p:
        a, b = torch.empty(5), torch.empty_like(torch.ones(2, 3))
        c = torch.empty(3, dtype=torch.int32)
    assert not a.any() and not b.any() and not c.any() and b.shape == (2, 3) and c.dtype == torch.int32
    assert p.allocations == 0 and p.workspaces == 0 and p.byte == 0xFF


def test_the_wrappers_are_taken_off_again_also_after_an_exception(monkeypatch):
    before = (torch.empty, torch.empty_like, _ops.workspace)
    with poison.poisoned(monkeypatch, 0x7F):
        assert torch.empty is not before[0] and torch.empty_like is not before[1] and _ops.workspace is not before[2]
    assert (torch.empty, torch.empty_like, _ops.workspace) == before
    with pytest.raises(KeyError):
        with poison.poisoned(monkeypatch, 0x7F):
            raise KeyError("inside")
    assert torch.empty is before[0] and torch.empty_like is before[1] and _ops.workspace is before[2]
    with pytest.raises(ValueError):
        with poison.poisoned(monkeypatch, 256):
            pass


def test_the_two_bytes_read_back_as_the_issue_says():
    for byte, as_float, as_int in ((0xFF, None, -1), (0x7F, FLOAT_7F, 2139062143)):
        raw = torch.full((4,), byte, dtype=torch.uint8)
        f, i = raw.view(torch.float32).item(), raw.view(torch.int32).item()
        assert i == as_int and (f != f if as_float is None else (f == as_float and f < float("inf")))
    assert f"{FLOAT_7F:.4e}" == "3.3962e+38"


# ---- comparing --------------------------------------------------------------------------------------------------------------------
def differences(tag, got, want, also=same_bits):
    """[] or [what is wrong with `got` against the clean `want` (CPU tensors, or None: not asked for)]; prints the count of differing
    elements, the largest difference, the newly non-finite ones and the first differing flat indices before anyone asserts."""
    if want is None or got is None:
        return [] if got is None and want is None else [(tag, "None on one side only")]
    if got.shape != want.shape or got.dtype != want.dtype:
        return [(tag, tuple(got.shape), got.dtype, "clean:", tuple(want.shape), want.dtype)]
    wrong = bits(got) != bits(want)
    n = int(wrong.sum())
    worse, largest = 0, 0.0
    if got.numel():
        largest = torch.nan_to_num((got.double() - want.double()).abs(), nan=float("inf")).max().item()
        if got.dtype.is_floating_point:
            worse = int((~torch.isfinite(got) & torch.isfinite(want)).sum())
    where = wrong.nonzero().reshape(-1)[:8].tolist()
    print(f"{tag}: {n} of {got.numel()} elements differ, largest difference {largest:.3e}, {worse} newly non-finite" +
          (f", first at flat indices {where}" if n else ""))
    return [(tag, n, largest, worse, where)] if (n or worse or not also(got, want)) else []


_CLEAN = {}


def clean(key, run):
    """The clean run of `run`, made once per key and shared (do not modify)."""
    if key not in _CLEAN:
        _CLEAN[key] = run()
    return _CLEAN[key]


def poisoned_equals_clean(key, run, byte, monkeypatch, workspace, also=same_bits):
    """run() -> {name: CPU tensor or None}: under the poison, the clean run's bits in every entry."""
    want = clean(key, run)
    with poison.poisoned(monkeypatch, byte) as p:
        got = run()
    assert set(got) == set(want)
    fails = [f for name in want for f in differences(f"{key} 0x{byte:02X} {name}", got[name], want[name], also)]
    print(f"{key}: {p.workspaces} workspace fetches and {p.allocations} device allocations poisoned")
    assert not fails, fails
    assert p.allocations >= 1 and (p.workspaces >= 1 if workspace else p.workspaces == 0), (p.workspaces, p.allocations)


def cpu(t):
    return None if t is None else t.detach().cpu()


# ---- controls: no library code ----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("byte", BYTES)
def test_control_what_is_not_written_stays_poison(byte, monkeypatch):
    d = dev()
    real = (torch.empty, torch.empty_like, _ops.workspace)
    plain = _ops.workspace(d, 4096)
    with poison.poisoned(monkeypatch, byte) as p:
        t = torch.empty(4, device=d)
        t[:3] = 1
        u = torch.empty_like(t)
        e = torch.empty(0, device=d)
        h = torch.empty(4)
        permuted = torch.empty_like(torch.zeros(2, 3, 4, device=d).permute(2, 0, 1))
        assert (p.workspaces, p.allocations) == (0, 3), "a CPU tensor and an empty tensor are not counted"
        ws = _ops.workspace(d, 4096)
        assert (p.workspaces, p.allocations) == (1, 3)
        ws[:8] = 0
        again = _ops.workspace(d, 4096)   # (filled at every fetch)
        assert p.workspaces == 2
    t, u = t.cpu(), u.cpu()
    assert t[:3].tolist() == [1.0, 1.0, 1.0]
    if byte == 0xFF:
        assert torch.isnan(t[3]) and torch.isnan(u).all()
    else:
        assert t[3].item() == FLOAT_7F and (u == t[3]).all()
    assert ws is plain and again is plain and ws.dtype == torch.uint8 and ws.numel() == 4096 and bool((ws == byte).all())
    assert not permuted.is_contiguous() and bool((bits(permuted.cpu()).view(torch.uint8) == byte).all())
    assert e.numel() == 0 and h.device.type == "cpu"
    assert (torch.empty, torch.empty_like, _ops.workspace) == real


# ---- the Conv3d families ------------------------------------------------------------------------------------------------------------
ALIGN, MAX_REC = 256, 64   # csrc/mgs_common.h


def _ceil(a, b):
    return -(-a // b)


def _up(n):
    return _ceil(n, ALIGN) * ALIGN


def cut_runs(items, most):
    """(records, items per record, items of the last record): csrc/mgs_records.hip's cut_runs."""
    per = _ceil(items, min(items, most))
    n = _ceil(items, per)
    return n, per, items - (n - 1) * per


class Invented:
    """A cases module of one case per family, "short_last": no small case of the families' own modules has more items than records,
    so none has a last record that is shorter than the others.  Shapes as in the family's module; the reference is the clean run, so
    the inputs are plain seeded normals."""
    SHAPES = {   # family: (x, w, bias or None, g); the items of dw | db; the op
        "conv3d":    ((1, 1, 33, 17, 65), (2, 1, 3, 3, 3), None, (1, 2, 33, 17, 65)),      # 9 x 3 x 3 = 81 tiles of 4 x 8 x 32
        "pointwise": ((1, 3, 1, 5, 3277), (5, 3, 1, 1, 1), (5,), (1, 5, 1, 5, 3277)),      # n = 16385 = 64 x 256 + 1: 65 tiles
        "narrow":    ((1, 2, 17, 17, 257), (1, 2, 3, 3, 3), (1,), (1, 1, 17, 17, 257)),    # 3 x 3 x 9 = 81 tiles of 8 x 8 x 32
        "dense":     ((1, 8, 7, 15, 5), (32, 8, 3, 3, 3), (32,), (1, 32, 5, 13, 3)),       # 5 x 13 rows of one segment: 65
        "patch":     ((65, 8, 5, 5, 5), (32, 8, 5, 5, 5), (32,), (65, 32, 1, 1, 1)),       # one patch, one tile per batch entry: 65
    }
    CALLS = {
        "conv3d": lambda m, x, w, b, split: m._conv3d(x, w, 1, split),
        "pointwise": lambda m, x, w, b, split: m._pointwise_conv3d(x, w, b, split),
        "narrow": lambda m, x, w, b, split: m._narrow_conv3d(x, w, b, "replicate", split),
        "dense": lambda m, x, w, b, split: m._dense_conv3d(x, w, b, 0.02, split),
        "patch": lambda m, x, w, b, split: m._patch_conv3d(x, w, b, 0, "replicate", 0.0, split),
    }

    def __init__(self, family):
        self.family, self._t = family, None

    def reference(self, case):
        assert case == "short_last"
        if self._t is None:
            xs, ws, bs, gs = self.SHAPES[self.family]
            gen = torch.Generator().manual_seed(9900 + sorted(self.SHAPES).index(self.family))
            fan = ws[1] * ws[2] * ws[3] * ws[4]
            self._t = {"x": torch.randn(xs, generator=gen), "w": torch.randn(ws, generator=gen) * fan ** -0.5,
                       "b": None if bs is None else torch.randn(bs, generator=gen), "g": torch.randn(gs, generator=gen)}
        return self._t


def family_of(name, case):
    f = cf.FAMILIES[name]
    if case != "short_last":
        return f
    call = Invented.CALLS[name]
    return cf.Family(name, Invented(name), f.prefix, lambda case, x, w, b, split=0: call(_mod(name), x, w, b, split), (),
                     splits=f.splits, needs=f.needs)


# family: (cases whose dw | db is exactly one record, cases cut into several records, the invented one whose last record is shorter,
# cases with a batch and partial last tiles)
CONV_CASES = {
    "conv3d": (("tiny",), ("stem_in", "up_op1"), "short_last", ("odd_s1",)),
    "pointwise": (("one_voxel",), ("in_pre",), "short_last", ("stem_out_batch",)),
    "narrow": (("head",), ("seams",), "short_last", ("odd",)),
    "dense": (("one_out_k3",), ("row_seam",), "short_last", ("odd_k3",)),
    "patch": (("one_patch", "site_small"), ("seam_m",), "short_last", ("odd", "odd_zeros")),
}
CONV_PARAMS = [(n, c) for n, (one, several, short, batch) in CONV_CASES.items() for c in one + several + (short,) + batch]
FORBIDDEN = ("long_sum", "long_sum_head", "max_c", "max_channels")


def conv_shape(name, case):
    """(B, Cin, Cout, input extents, the family's last arguments) of a case."""
    if case == "short_last":
        xs, ws, _, _ = Invented.SHAPES[name]
        return xs[0], xs[1], ws[0], tuple(xs[2:]), ws[2]
    cases = family_of(name, case).cases
    if name == "conv3d":
        B, a, b, ext, last = (cases.TRANSPOSED if cases.is_transposed(case) else cases.CASES)[case]["shape"]
        if cases.is_transposed(case):   # the convolution it transposes: this op's output is its input side, stride 2
            return B, b, a, tuple(2 * i - 1 + last for i in ext), 2
        return B, a, b, ext, last
    if name == "dense":
        B, cin, cout, k, ext = cases.CASES[case]["shape"]
        return B, cin, cout, tuple(e + k - 1 for e in ext), k
    if name == "patch":
        B, cin, cout, ext, k, pad = cases.CASES[case]["shape"]
        return B, cin, cout, ext, (k, pad)
    B, cin, cout, ext = cases.CASES[case]["shape"][:4]
    return B, cin, cout, ext, None


def conv_records(name, case):
    """(items, most records, bytes of a record, the library's workspace bytes as restated here, the library's own) of a case: the host
    code of the five families, restated."""
    B, cin, cout, ext, last = conv_shape(name, case)
    L = _lib.lib()
    pad128 = lambda c: _ceil(c, 128) * 128   # noqa: E731
    if name == "conv3d":
        stride = 1 if case == "short_last" else last
        out = tuple((i - 1) // stride + 1 for i in ext)
        items = B * _ceil(out[0], 4 if stride == 1 else 2) * _ceil(out[1], 8) * _ceil(out[2], 32)
        rec, most = 4 * cout * cin * 27, MAX_REC
        need = lambda n: _up(n * rec) + ALIGN   # noqa: E731
        got = L.mgs_conv3d_workspace_bytes(B, cin, cout, *ext, stride)
    elif name == "pointwise":
        n = ext[0] * ext[1] * ext[2]
        items, rec, most = B * _ceil(n, 256 if cin <= 8 else 128), 4 * cout * (cin + 1), MAX_REC
        need = lambda n: _up(n * rec) + ALIGN   # noqa: E731
        got = L.mgs_pointwise_workspace_bytes(B, cin, cout, n)
    elif name == "narrow":
        items, rec, most = B * _ceil(ext[0], 8) * _ceil(ext[1], 8) * _ceil(ext[2], 32), 4 * cout * (27 * cin + 1), MAX_REC
        need = lambda n: _up(n * rec) + ALIGN   # noqa: E731
        got = L.mgs_narrow_conv3d_workspace_bytes(B, cin, cout, *ext)
    elif name == "dense":
        k = last
        o = tuple(e - k + 1 for e in ext)
        items, rec = B * o[0] * o[1] * _ceil(o[2], 64), 4 * cout * (cin * k ** 3 + 1)
        most = min(MAX_REC, max(8, (128 << 20) // rec))
        weights = _up(4 * k ** 3 * max(cin * pad128(cout), cout * pad128(cin)))
        need = lambda n: weights + _up(n * rec) + ALIGN   # noqa: E731
        got = L.mgs_dense_conv3d_workspace_bytes(B, cin, cout, k, *ext)
    else:
        k, pad = (5, 0) if case == "short_last" else last
        o = tuple((e + 2 * pad - k) // k + 1 for e in ext)
        items, rec = B * _ceil(o[0] * o[1] * o[2], 32), 4 * cout * (cin * k ** 3 + 1)
        most = min(MAX_REC, max(2, (64 << 20) // rec))
        weights = _up(4 * cin * k ** 3 * pad128(cout))
        need = lambda n: max(weights, _up(n * rec)) + ALIGN   # noqa: E731
        got = L.mgs_patch_conv3d_workspace_bytes(B, cin, cout, k, pad, *ext)
    return items, most, rec, need(cut_runs(items, most)[0]), got


@pytest.mark.parametrize("name", list(CONV_CASES))
def test_the_conv_cases_are_cut_into_records_as_they_claim(name):
    one, several, short, batch = CONV_CASES[name]
    assert not set(one + several + batch) & set(FORBIDDEN) and not any(c.endswith("_head") for c in one + several + batch)
    for case in one + several + (short,) + batch:
        items, most, rec, need, got = conv_records(name, case)
        print(name, case, "items", items, "most", most, "records, per, last", cut_runs(items, most), "workspace", got)
        assert need == got, (name, case, "the restated workspace size is not the library's", need, got)
    for case in one:
        assert cut_runs(*conv_records(name, case)[:2]) == (1, 1, 1)
    for case in several:
        assert cut_runs(*conv_records(name, case)[:2])[0] > 1
    n, per, rest = cut_runs(*conv_records(name, short)[:2])
    assert n > 1 and per > 1 and 0 < rest < per, "a shorter last record"
    for case in batch:
        B, _, _, ext, _ = conv_shape(name, case)
        assert B > 1 and cut_runs(*conv_records(name, case)[:2])[0] > 1 and any(e % 2 for e in ext)   # (odd extents: partial last tiles)


@gpu
@pytest.mark.parametrize("byte", BYTES)
@pytest.mark.parametrize("name, case", CONV_PARAMS)
def test_conv_family(name, case, byte, monkeypatch):
    """Every split and every combination of requested gradients, poisoned: the bits of the clean all-requested run at the library's
    split in every requested quantity, None for a gradient not asked for.  A dw-only or db-only call can no longer read the records the
    full call before it left behind."""
    family = family_of(name, case)
    want = clean(("conv", name, case), lambda: cf.run(family, case))
    width = len(family.needs[0])
    fails, fetched, allocated = [], 0, 0
    for split in (0,) + tuple(family.splits):
        for need in list(family.needs) + [(True,) * width]:
            with poison.poisoned(monkeypatch, byte) as p:
                got = cf.run(family, case, split=split, need=need)
            asked = dict(zip(("dx", "dw", "db"), tuple(need) + (True,) * (3 - width)))
            tag = f"{name} {case} 0x{byte:02X} split {split} need {need}"
            fails += differences(tag + " y", got["y"], want["y"], family.cases.same_bits if hasattr(family.cases, "same_bits") else same_bits)
            for q in ("dx", "dw", "db"):
                fails += differences(f"{tag} {q}", got[q], want[q] if asked[q] else None)
            assert p.allocations >= 1, tag
            fetched, allocated = fetched + p.workspaces, allocated + p.allocations
    print(f"{name} {case}: {fetched} workspace fetches and {allocated} device allocations poisoned")
    assert not fails, fails
    assert fetched >= 1 and allocated >= 1


# ---- the other ops with a workspace -----------------------------------------------------------------------------------------------
def _spatial_softmax(case, slices):
    x, g_k, g_m = ssc.make_inputs(case)
    d = dev()
    x = x.to(d).requires_grad_(True)
    kp, mx = _mod("spatial_softmax")._spatial_softmax3d(x, ssc.TEMPERATURE, slices=slices)
    torch.autograd.backward([kp, mx], [g_k.to(d), g_m.to(d)])
    return dict(keypoints=cpu(kp), maxpool=cpu(mx), dx=cpu(x.grad))


@gpu
@pytest.mark.parametrize("byte", BYTES)
@pytest.mark.parametrize("case, slices", [("odd31", 0), ("odd31", 3), ("odd31", 7), ("noncube", 0), ("noncube", 2)])
def test_spatial_softmax(case, slices, byte, monkeypatch):
    """odd31: rows of 29 791 elements (odd: the second row starts misaligned), 1, 3 and 7 workgroup records per row; noncube: a batch."""
    poisoned_equals_clean(("spatial_softmax", case, slices), lambda: _spatial_softmax(case, slices), byte, monkeypatch, True,
                          ssc.same_bits)


def _attention(case):
    """The case's q and kv projections (made on the CPU from its x, context and weights) through the fused op and its backward."""
    c = atc.CASES[case]
    x, context, mask, grad, params = atc.make_inputs(case)
    d = dev()
    q = (x @ params["to_q.weight"].t()).to(d).requires_grad_(True)
    kv = ((x if context is None else context) @ params["to_kv.weight"].t()).to(d).requires_grad_(True)
    g = torch.randn(q.shape, generator=torch.Generator().manual_seed(1900 + list(atc.CASES).index(case))).to(d)
    out = _mod("attention").fused_attention_kv(q, kv, c["H"], mask=None if mask is None else mask.to(d))
    out.backward(g)
    return dict(out=cpu(out), dq=cpu(q.grad), dkv=cpu(kv.grad))


@gpu
@pytest.mark.parametrize("byte", BYTES)
@pytest.mark.parametrize("case", ["masked", "cross_enc"])
def test_attention(case, byte, monkeypatch):
    """masked: Nq = 9, Nk = 70 with masked keys and a batch entry masked as a whole; cross_enc: Nq = 130, Nk = 338; all off the 64-wide
    tiles.  The backward's D_i come from the workspace."""
    c = atc.CASES[case]
    assert c["Nq"] % 64 and c["Nk"] % 64 and c["p"] == 0.0 and (c["mask"] is not None) == (case == "masked")
    poisoned_equals_clean(("attention", case), lambda: _attention(case), byte, monkeypatch, True, atc.same_bits)


ABN_LONG = (2, 3, 11, 19, 21)   # rows of 4389 elements: the one shape here that the library cuts into 2 sub-slices (512 vectors each at least)


def _abn_inputs(case, residual):
    if case != "long":
        t = dict(ac.load_fixture(case))
    else:
        g = torch.Generator().manual_seed(4100)
        C = ABN_LONG[1]
        t = {"x": torch.randn(ABN_LONG, generator=g), "residual": torch.randn(ABN_LONG, generator=g), "g": torch.randn(ABN_LONG, generator=g),
             "weight": 1.0 + 0.5 * torch.randn(C, generator=g), "bias": 0.3 * torch.randn(C, generator=g)}
    if not residual:
        t.pop("residual", None)
    return t


def _batch_norm_act(case, residual, slices):
    t, d = _abn_inputs(case, residual), dev()
    x, w, b = (t[k].to(d).clone().requires_grad_(True) for k in ("x", "weight", "bias"))
    res = t["residual"].to(d).clone().requires_grad_(True) if "residual" in t else None
    C = w.numel()
    rm, rv, nbt = torch.zeros(C, device=d), torch.ones(C, device=d), torch.zeros((), dtype=torch.int64, device=d)
    y = _mod("encoder")._batch_norm_act(x, w, b, rm, rv, nbt, True, ac.MOMENTUM, ac.EPS, 0.01, res, slices=slices)
    y.backward(t["g"].to(d))
    return dict(y=cpu(y), dx=cpu(x.grad), dweight=cpu(w.grad), dbias=cpu(b.grad), dres=None if res is None else cpu(res.grad),
                running_mean=cpu(rm), running_var=cpu(rv), num_batches_tracked=cpu(nbt))


@gpu
@pytest.mark.parametrize("byte", BYTES)
@pytest.mark.parametrize("case, residual, slices", [("odd", True, 1), ("odd", False, 0), ("long", True, 1), ("long", True, 2),
                                                    ("long", False, 0), ("long", False, 2)])
def test_batch_norm_act(case, residual, slices, byte, monkeypatch):
    """Training-mode forward and backward, with and without the skip add.  odd (the fixture): one sub-slice per row; long: two, reduced by
    one workgroup (slices 1) and by two."""
    if case == "long":
        assert ABN_LONG[2] * ABN_LONG[3] * ABN_LONG[4] // 4 // 512 == 2 and (ABN_LONG[2] * ABN_LONG[3] * ABN_LONG[4]) % 4
    poisoned_equals_clean(("batch_norm_act", case, residual, slices), lambda: _batch_norm_act(case, residual, slices), byte, monkeypatch,
                          True, ac.same_bits)


def _feedforward(fn, inputs):
    *leaves, g = inputs
    r = fc.run_op(fn, leaves, g, device=dev())
    return {k: cpu(v) for k, v in r.items()}


@gpu
@pytest.mark.parametrize("byte", BYTES)
@pytest.mark.parametrize("split", (0,) + fc.SPLITS)
def test_layer_norm(split, byte, monkeypatch):
    case = fc.SPLIT_CASES[0]
    assert case in fc.LN_CASES and fc.LN_CASES[case]["rows"] == 257
    ff = _mod("feedforward")
    poisoned_equals_clean(("layer_norm", case, split), lambda: _feedforward(lambda x, w, b: ff.layer_norm(x, w, b, fc.EPS, split),
                                                                            fc.ln_inputs(case)), byte, monkeypatch, True, fc.same_bits)


@gpu
@pytest.mark.parametrize("byte", BYTES)
@pytest.mark.parametrize("split", (0,) + fc.SPLITS)
def test_bias_geglu(split, byte, monkeypatch):
    case = fc.SPLIT_CASES[1]
    assert case in fc.GEGLU_CASES and fc.GEGLU_CASES[case]["rows"] == 257
    ff = _mod("feedforward")
    h, b, g = fc.geglu_inputs(case)
    poisoned_equals_clean(("bias_geglu", case, split), lambda: _feedforward(lambda h, b: ff.bias_geglu(h, b, split), (h, b, g)), byte,
                          monkeypatch, True, fc.same_bits)


def _resample_pad(case):
    _, scale, pad = vc.CASES[case]
    d = dev()
    sources = [t.detach().requires_grad_(True) for t in vc.make_sources(case, d)]
    out = _mod("volume").resample_pad(sources, scale, pad)
    out.backward(vc.make_upstream(case, d))
    r = {"out": cpu(out)}
    r.update({f"g_source{k}": cpu(t.grad) for k, t in enumerate(sources)})
    return r


@gpu
@pytest.mark.parametrize("byte", BYTES)
@pytest.mark.parametrize("case", ["cat_pad1", "cat3_up2"])
def test_resample_pad(case, byte, monkeypatch):
    """cat_pad1: two sources, one a channel slice, scale 1 (the backward is one launch and leaves the workspace alone); cat3_up2: three
    sources, a batch, scale 2 and a pad: the x y sums go through the workspace."""
    assert vc.CASES[case][1] == (1 if case == "cat_pad1" else 2)
    poisoned_equals_clean(("resample_pad", case), lambda: _resample_pad(case), byte, monkeypatch, True, vc.same_bits)


def _se3(name, cameras):
    c, d = sc3.load_cases()[name], dev()
    m = _mod("augmentation").Se3Augmentation(sc3.trans_aug_tensor(float(c["trans_aug_range"])), [float(v) for v in c["rot_aug_range"]],
                                             sc3.ROT_AUG_RESOLUTION, sc3.VOXEL_SIZE, sc3.ROT_RESOLUTION, layer=int(c["layer"]),
                                             attempts=sc3.ATTEMPTS)
    t = lambda a: torch.from_numpy(a).to(d)   # noqa: E731
    n = int(c["n_cams"])
    trans, rot, pcd, pose = m([t(c[f"pcd{i}"]) for i in range(n)], [t(c[f"pose{i}"]) for i in range(n)] if cameras else None, t(c["gripper"]),
                              t(c["action_trans"]), t(c["action_rot_grip"]), t(c["bounds"]), draws=t(c["draws"]))
    assert len(pose) == (n if cameras else 0)
    r = dict(action_trans=cpu(trans), action_rot_grip=cpu(rot), info=cpu(m.last_info))
    r.update({f"pcd{i}": cpu(p) for i, p in enumerate(pcd)})
    r.update({f"pose{i}": cpu(p) for i, p in enumerate(pose)})
    return r


@gpu
@pytest.mark.parametrize("byte", BYTES)
@pytest.mark.parametrize("name, cameras", [("b3_5x7_c2_low", True), ("b3_4x4_c3_never", False), ("b8_4x4_c3", False)])
def test_se3_augmentation(name, cameras, byte, monkeypatch):
    """The draws are given, so the run repeats.  One workspace fetch serves mgs_se3_select and mgs_se3_apply.  _low: a sample accepted at
    its third attempt, with cameras; _never: one sample is never accepted, so the whole batch takes the identity record; without cameras
    no pose is transformed."""
    poisoned_equals_clean(("se3", name, cameras), lambda: _se3(name, cameras), byte, monkeypatch, True)


@gpu
@pytest.mark.parametrize("byte", BYTES)
@pytest.mark.parametrize("memory", ["channels_first", "channels_last"])
@pytest.mark.parametrize("case", ["odd_v37_n1000", "edges_nonfinite"])
def test_voxelizer(case, memory, byte, monkeypatch):
    """Against the committed fixture, bit for bit.  odd_v37_n1000: 37^3 voxels (no multiple of 4: the scalar write path), a sixth of the
    points outside; edges_nonfinite: points on every boundary, NaN, infinite and 1e30 coordinates, most voxels empty."""
    f = vz.load_fixture(case)
    vz.assert_case_is_what_it_claims(case, f["coords"], f["bounds"], f["V"])
    truth = vz.grid_of_fixture(f)

    def run():
        d = dev()
        grid = _mod("voxelizer").voxelize(f["coords"].to(d), None if f["features"] is None else f["features"].to(d), f["bounds"].to(d),
                                          f["V"], memory)
        return dict(grid=cpu(grid).contiguous())
    poisoned_equals_clean(("voxelizer", case, memory), run, byte, monkeypatch, True, vz.same_bits)
    assert vz.same_bits(clean(("voxelizer", case, memory), run)["grid"], truth), "the clean run is not the fixture"


# ---- ops that only allocate results: N = 257, off every block size ------------------------------------------------------------------
N = 257


def _grads(outs, leaves, cots):
    torch.autograd.backward(list(outs), [c.to(dev()) for c in cots])
    return [cpu(t.grad) for t in leaves]


def _deform():
    d = dev()
    a = ec.assembly_inputs(N, 32, 16, 8, True)
    t = {k: (None if v is None else v.to(d)) for k, v in a.items()}
    lat, z = t["point_latent"].requires_grad_(True), t["z_feature"].requires_grad_(True)
    dfm = _mod("deform")
    out = dfm.assemble_deform_input(lat, z, t["xyz"], t["sh"], t["rot"], t["scale"], t["opacity"], t["feature"], t["action"])
    g = torch.randn(out.shape, generator=torch.Generator().manual_seed(7290))
    g_lat, g_z = _grads([out], [lat, z], [g])
    delta, xyz, rot, cot = ec.apply_inputs(N)
    delta = delta.to(d).requires_grad_(True)
    nx, nr = dfm.deform_apply(delta, xyz.to(d), rot.to(d))
    (g_delta,) = _grads([nx, nr], [delta], cot)
    x = torch.randn(N, 64, generator=torch.Generator().manual_seed(7291)).to(d)
    act, xb = dfm._relu_bias(x, torch.randn(64, generator=torch.Generator().manual_seed(7292)).to(d))
    return dict(assembled=cpu(out), g_point_latent=g_lat, g_z_feature=g_z, next_xyz=cpu(nx), next_rot=cpu(nr), g_delta=g_delta,
                relu=cpu(act), x_plus_bias=cpu(xb))


def _gaussian_epilogue():
    d = dev()
    raw, xyz_in, cot = ec.epilogue_inputs(N)
    raw, xyz_in = raw.to(d).requires_grad_(True), xyz_in.to(d).requires_grad_(True)
    out = _mod("regressor").gaussian_epilogue(raw, xyz_in)
    g_raw, g_xyz = _grads([out[k] for k in ec.EPILOGUE_OUTPUTS], [raw, xyz_in], [cot[k] for k in ec.EPILOGUE_OUTPUTS])
    r = {k: cpu(v) for k, v in out.items()}
    r.update(g_raw=g_raw, g_xyz_in=g_xyz)
    return r


def _point_latent():
    case = ((2, 3, 4), 8, 6, N)
    assert case in ec.VOXEL_CASES
    vox, xyz, _ = ec.voxel_inputs(case)
    d = dev()
    return dict(out=cpu(_mod("voxel").point_latent_pe(vox.to(d), xyz.to(d), ec.BOUNDS, 6)))


def _novel_calib():
    g = torch.Generator().manual_seed(7400)
    q, _ = torch.linalg.qr(torch.randn(N, 3, 3, generator=g))
    extr = torch.eye(4).repeat(N, 1, 1)
    extr[:, :3, :3], extr[:, :3, 3] = q, torch.randn(N, 3, generator=g)
    intr = torch.zeros(N, 3, 3)
    intr[:, 0, 0], intr[:, 1, 1] = 100.0 + 50.0 * torch.rand(N, generator=g), 100.0 + 50.0 * torch.rand(N, generator=g)
    intr[:, 0, 2], intr[:, 1, 2], intr[:, 2, 2] = 64.0, 48.0, 1.0
    d = dev()
    out = _mod("camera").get_novel_calib({"intr": intr.to(d), "extr": extr.to(d)}, 128, 96)
    return {k: cpu(v) for k, v in out.items()}


@gpu
@pytest.mark.parametrize("byte", BYTES)
def test_deform(byte, monkeypatch):
    """The deformation field's input assembly and its apply step, forward and backward, and the MLP's bias + ReLU pass, at 257 rows."""
    poisoned_equals_clean("deform", _deform, byte, monkeypatch, False)


@gpu
@pytest.mark.parametrize("byte", BYTES)
def test_gaussian_epilogue(byte, monkeypatch):
    poisoned_equals_clean("gaussian_epilogue", _gaussian_epilogue, byte, monkeypatch, False)


@gpu
@pytest.mark.parametrize("byte", BYTES)
def test_point_latent(byte, monkeypatch):
    """Forward only: the backward allocates with torch.zeros and adds with float atomics, so it has neither a poisoned result nor bits to
    repeat."""
    poisoned_equals_clean("point_latent", _point_latent, byte, monkeypatch, False)


@gpu
@pytest.mark.parametrize("byte", BYTES)
def test_novel_calib(byte, monkeypatch):
    """257 cameras in one launch."""
    poisoned_equals_clean("novel_calib", _novel_calib, byte, monkeypatch, False)


# ---- ops that carve scratch out of a torch.empty buffer of their own ----------------------------------------------------------------
def _rendering_loss(case):
    c, d = lc.CASES[case], dev()
    inp, _ = lc.make_inputs(case)
    color, feature = inp["color"].to(d).requires_grad_(True), inp["feature"].to(d).requires_grad_(True)
    gt_rgb, gt_embed = lc.lay_out(inp["gt_rgb"], c["layout"][0]).to(d), lc.lay_out(inp["gt_embed"], c["layout"][1]).to(d)
    loss, terms = _mod("losses").rendering_loss(color, gt_rgb, feature, gt_embed, weights=c["weights"], embed_loss_fn=c["fn"])
    loss.backward()
    return dict(loss=cpu(loss), g_color=cpu(color.grad), g_feature=cpu(feature.grad), **{k: cpu(v) for k, v in terms.items()})


@gpu
@pytest.mark.parametrize("byte", BYTES)
@pytest.mark.parametrize("case", ["l2_norm_odd_f5", "odd_f8_last"])
def test_rendering_loss(case, byte, monkeypatch):
    """100 x 75 images (W no multiple of 4).  l2_norm_odd_f5 also goes through the min / max partials of the target embedding."""
    assert lc.CASES[case]["W"] % 4 and (lc.CASES[case]["fn"] == "l2_norm") == (case == "l2_norm_odd_f5")
    poisoned_equals_clean(("rendering_loss", case), lambda: _rendering_loss(case), byte, monkeypatch, False)


def _photometric_loss(case):
    c, d = phc.CASES[case], dev()
    inp = phc.make_inputs(case)
    color = inp["color"].to(d).requires_grad_(True)
    loss, terms = _mod("photometric").photometric_loss(color, phc.lay_out(inp["target"], c["layout"]).to(d), weights=c["weights"])
    loss.backward()
    return dict(loss=cpu(loss), g_color=cpu(color.grad), **{k: cpu(v) for k, v in terms.items()})


@gpu
@pytest.mark.parametrize("byte", BYTES)
@pytest.mark.parametrize("case", ["odd_37x23", "tiles_70x45"])
def test_photometric_loss(case, byte, monkeypatch):
    """odd_37x23: two views, partial tiles on both axes, W no multiple of 4; tiles_70x45: several tiles each way, so the gradient's halo
    reads maps that other workgroups wrote."""
    poisoned_equals_clean(("photometric_loss", case), lambda: _photometric_loss(case), byte, monkeypatch, False)


def _fused_lamb(steps=2):
    """The optimizer is built, and its layout with it, inside whatever context this runs in."""
    inp, d = lac.make_inputs("odd_sizes"), dev()
    ps = []
    for i, t in enumerate(inp["params"]):
        if i in inp["case"].get("offset_view", []):   # 4 bytes off a 16-byte boundary, as tests/test_optim.py lays it out
            v = torch.zeros(t.numel() + 1, device=d)[1:].view(t.shape)
            v.copy_(t)
            ps.append(v.requires_grad_(True))
        else:
            ps.append(t.to(d).requires_grad_(True))
    groups = [dict(params=[ps[i] for i in g["idx"]], lr=g["lr"], betas=g["betas"], eps=g["eps"], weight_decay=g["weight_decay"])
              for g in inp["groups"]]
    opt = _mod("optim").FusedLamb(groups, adam=inp["adam"])
    r = {}
    for k in range(steps):
        for p, g in zip(ps, lac.gradients(inp, k)):
            if p.grad is None:
                p.grad = g.to(d)
            else:
                p.grad.copy_(g.to(d))
        opt.step()
        for i, p in enumerate(ps):
            st = opt.state[p]
            r[f"step{k} stats{i}"] = cpu(torch.stack([st["weight_norm"], st["adam_norm"], st["trust_ratio"]]))
    for i, p in enumerate(ps):
        r[f"p{i}"], r[f"m{i}"], r[f"v{i}"] = cpu(p), cpu(opt.state[p]["exp_avg"]), cpu(opt.state[p]["exp_avg_sq"])
    return r


@gpu
@pytest.mark.parametrize("byte", BYTES)
def test_fused_lamb(byte, monkeypatch):
    """Two steps of odd_sizes (1, 3, 5, 4097, 262 145 and 13 x 79 elements, the last 4 bytes off a 16-byte boundary): p, m, v and the
    three statistics of both steps."""
    poisoned_equals_clean("fused_lamb", _fused_lamb, byte, monkeypatch, False)
