"""GPU parity tests (run with -m gpu on an MI355X): the HIP path, called through the public API and the C ABI,
against Oracle B on the same seeded inputs, against the committed golden vectors, and -- at BASELINE.json's
full sizes -- through size-independent properties.

Tolerances (BASELINE.json north_star): 1e-4 absolute on rendered RGB / feature maps; gradients within 1e-3 of
the tensor's largest gradient magnitude (the per-Gaussian sums are float atomics in arbitrary order, in the
reference as well: RAST/cuda_rasterizer/backward.cu:541-590)."""
import glob
import os
import types
import warnings

import numpy as np
import pytest
import torch

from child import run_graph_tool
import util
from manigaussian_amd import GaussianRasterizationSettings, GaussianRasterizer, _lib
from manigaussian_amd import synthetic as syn

pytestmark = pytest.mark.gpu

IMG_TOL = 1e-4
GRAD_TOL = 1e-3
GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "*.npz")))
REF_GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "ref", "*.npz")))


@pytest.fixture(autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need a HIP device"
    L = _lib.lib()
    assert os.path.samefile(L._name, os.path.join(os.path.dirname(_lib.__file__), "libmgsplat.so"))
    yield


def _check(case, tight_bins=None):
    if tight_bins is None:
        return _check_(case)
    old = _lib.get_option("tight_bins")
    try:  # a per-call option: only the default the shim copies into each call is switched, and put back
        _lib.set_option("tight_bins", tight_bins)
        return _check_(case)
    finally:
        _lib.set_option("tight_bins", old)


def _check_(case):
    case = dict(case)
    max_fragile = case.pop("max_fragile_gaussians", 0.05)
    sc, cam, kw, dC, dF = util.scene_case(**case)
    inc = case.get("include_feature", True)
    cr, fr, rr, gr, st = util.run_oracle_b(sc, kw, dC, dF)
    ch, fh, rh, gh = util.run_hip(sc, cam, dC, dF, case.get("sh_degree", 1), inc, case.get("bg", (0.1, 0.2, 0.3)))
    assert torch.equal(rh, rr), "radii differ"
    imgs = [("color", ch, cr)]
    if inc:
        assert fh.shape == fr.shape
        imgs.append(("feature", fh, fr))
    else:
        assert fh.shape == (1,)
    for nm, a, b in imgs:
        robust, fragile, frac = util.image_errors(a, b, st)
        assert robust <= IMG_TOL, f"{nm}: {robust:.3e} on threshold-robust pixels"
        assert fragile <= util.FRAGILE_TOL and frac <= util.FRAGILE_MAX_FRACTION, (nm, fragile, frac)
    errs, frac = util.grad_errors_split(gh, gr, st)
    assert frac <= max_fragile
    for k, (robust, fragile, mag) in errs.items():
        assert robust <= GRAD_TOL * mag + 1e-7, f"grad {k}: err {robust:.3e} vs max {mag:.3e}"
        assert fragile <= util.FRAGILE_GRAD_TOL * mag + 1e-7, f"grad {k} (threshold-fragile): {fragile:.3e} vs {mag:.3e}"
    return st


@pytest.mark.parametrize("F", [3, 32], ids=["valu_blend_f3", "mfma_blend_f32"])
def test_translucent_scene_walks_many_rounds(F):
    """Almost transparent Gaussians on a small image: no pixel terminates, so every 8x8 block walks its whole list --
    thousands of survivors, i.e. several fill steps and several rounds of the dense forward, partial last chunks, and as
    many chunk records in the backward."""
    sc, cam, kw, dC, dF = util.scene_case(P=30000, F=F, W=32, H=32)
    sc["opacities"] = (sc["opacities"] * 0.1).contiguous()
    cr, fr, rr, gr, st = util.run_oracle_b(sc, kw, dC, dF)
    assert st.num_rendered > 4 * 6000 and float(st.array("final_T").min()) > 1e-3  # long lists, nothing terminates
    ch, fh, rh, gh = util.run_hip(sc, cam, dC, dF, 1, True, (0.1, 0.2, 0.3))
    assert torch.equal(rh, rr)
    for a, b in ((ch, cr), (fh, fr)):
        robust, fragile, frac = util.image_errors(a, b, st)
        assert robust <= IMG_TOL and fragile <= util.FRAGILE_TOL
    errs, _ = util.grad_errors_split(gh, gr, st)
    for k, (robust, fragile, mag) in errs.items():
        assert robust <= GRAD_TOL * mag + 1e-7, f"grad {k}: err {robust:.3e} vs max {mag:.3e}"
        assert fragile <= util.FRAGILE_GRAD_TOL * mag + 1e-7, f"grad {k} (threshold-fragile): {fragile:.3e} vs {mag:.3e}"


def test_one_block_with_hundreds_of_chunks():
    """One 8x8 image = one block; 40 000 Gaussians whose opacity sits just above 1/255, so that each is blended at a pixel or
    two and nothing terminates: the block's list holds > 400 chunks of 64 survivors -- dozens of forward rounds (more than
    the 16 / 8 whose first records the kernels keep in LDS: the chunk-record lookups fall back to the table in memory) and
    more q values than fit the backward's LDS area (the sums behind a chunk then come from memory)."""
    sc, cam, kw, dC, dF = util.scene_case(P=40000, F=32, W=8, H=8)
    sc["opacities"] = torch.full_like(sc["opacities"], 0.0045)
    cr, fr, rr, gr, st = util.run_oracle_b(sc, kw, dC, dF)
    assert st.num_rendered > 26000 and float(st.array("final_T").min()) > 1e-3, (st.num_rendered, float(st.array("final_T").min()))
    ch, fh, rh, gh = util.run_hip(sc, cam, dC, dF, 1, True, (0.1, 0.2, 0.3))
    assert torch.equal(rh, rr)
    for a, b in ((ch, cr), (fh, fr)):
        robust, fragile, frac = util.image_errors(a, b, st)
        assert robust <= IMG_TOL and fragile <= util.FRAGILE_TOL
    errs, _ = util.grad_errors_split(gh, gr, st)
    for k, (robust, fragile, mag) in errs.items():
        assert robust <= GRAD_TOL * mag + 1e-7, f"grad {k}: err {robust:.3e} vs max {mag:.3e}"
        assert fragile <= util.FRAGILE_GRAD_TOL * mag + 1e-7, f"grad {k} (threshold-fragile): {fragile:.3e} vs {mag:.3e}"


def test_randomised_sweep_fixed_seed():
    """24 cases of tests/tools/fuzz_parity.py (random sizes, feature widths, colour sources, opacity scales, cameras)."""
    import importlib.util
    import random
    spec = importlib.util.spec_from_file_location(
        "fuzz_parity", os.path.join(os.path.dirname(__file__), "tools", "fuzz_parity.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    rng = random.Random(7)
    assert all([fz.one(rng, i) for i in range(24)])


def test_wave64_primitives_selftest():
    assert _lib.lib().mgs_selftest(None) == 0, _lib.last_error()


CASES = {
    "manigaussian_shape_16k_f3_negfocal": dict(P=16384, F=3),
    "f32_posfocal": dict(P=6000, F=32, neg=False),
    "precomp_rgb_only": dict(P=5000, F=3, colors_precomp=True, include_feature=False),
    "sh3_unnormalised_quat": dict(P=3000, F=3, M=16, sh_degree=3, unnormalized_rot=True),
    "sh2_f4_black_bg": dict(P=3000, F=4, M=9, sh_degree=2, bg=(0.0, 0.0, 0.0)),
    "cov3d_precomp_odd_size": dict(P=3000, F=3, cov3d=True, W=72, H=40),
    "padded_feature_width_f5": dict(P=2000, F=5),
    "f8": dict(P=2000, F=8), "f16": dict(P=2000, F=16), "f64": dict(P=1500, F=64),
    "image_256": dict(P=8000, F=32, W=256, H=256),
    "tiny_image_8x8": dict(P=500, F=3, W=8, H=8),
    "single_gaussian": dict(P=1, F=3, W=16, H=16),
    "odd_17x33_f64": dict(P=70, F=64, W=17, H=33),
    "image_512_1024_tiles": dict(P=6000, F=8, W=512, H=512),
    # few Gaussians with huge footprints: many of them own at least one threshold-fragile pixel pair
    "image_1080p_binning_tables_in_memory": dict(P=3000, F=3, W=1920, H=1080, max_fragile_gaussians=0.5),
    "other_view": dict(P=4000, F=3, cam_index=3),
}


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("tight", [0, 1])
def test_parity_with_oracle(name, tight):
    _check(CASES[name], tight_bins=tight)


_DEFAULTS = dict(gm_waves=12, bin_mode=2, seg=2048, exact_cull=1, fast_exp=0, tight_bins=1)
VARIANTS = {
    "binning_tables_in_memory": dict(bin_mode=0), "segment_sort_rank_merge": dict(bin_mode=1),
    "segments_512": dict(bin_mode=1, seg=512), "segments_1024": dict(bin_mode=1, seg=1024), "segments_4096": dict(bin_mode=1, seg=4096),
    "backward_8_waves": dict(gm_waves=8),
    "backward_16_waves_one_pixel_per_step": dict(gm_waves=16),
    "v_exp_f32_bbox_cull": dict(fast_exp=1, exact_cull=0), "v_exp_f32": dict(fast_exp=1),
}


@pytest.mark.parametrize("name", list(VARIANTS))
def test_kernel_variants_agree_with_oracle(name):
    """Every per-call switch (MgsOptions) selects another implementation of the same result contract."""
    try:
        for k, v in VARIANTS[name].items():
            _lib.set_option(k, v)
        _check(dict(P=6000, F=32))
        _check(dict(P=3000, F=3, cov3d=True, W=72, H=40))
    finally:
        for k, v in _DEFAULTS.items():
            _lib.set_option(k, v)


@pytest.mark.parametrize("P,F,view", [(20000, 32, 0), (20000, 32, 5), (30000, 3, 2), (100000, 32, 1)])
def test_backward_forms_take_the_forward_s_decisions(P, F, view):
    """The three forms of the render backward (12 waves / two pixels per step, 16 and 8 waves / one pixel per step) evaluate
    the pair exponent through the same function as the forward (mgs_render_common.h gauss_power / gauss_power2), so they skip
    exactly the pairs the forward skipped: their gradients differ by summation order only (<= 1e-5 of the tensor's max; one pair
    decided differently shows as ~1e-3).  Round 5 regression: the packed form once multiplied (cy dy) dx instead of (cy dx) dy,
    one ulp apart, and blended one pair of view 0 of the first scene that the forward had skipped -- 1.4e-3 of the max on one
    Gaussian, inside the 1e-3-of-max-away-from-fragile-pairs contract of every test against the oracles, caught only by
    test_view_batch_equals_per_view_calls."""
    sc = syn.make_scene(P, F=F, M=4, seed=2)
    cam = syn.circle_cameras(8, 128, 128, negative_focal=True)[view]
    g = torch.Generator().manual_seed(4 + view)
    dC, dF = torch.randn(3, 128, 128, generator=g), torch.randn(F, 128, 128, generator=g)
    res = {}
    try:
        for gw in (16, 12, 8):
            _lib.set_option("gm_waves", gw)
            res[gw] = util.run_hip(sc, cam, dC, dF, 1, True, (0.1, 0.2, 0.3))
    finally:
        _lib.set_option("gm_waves", _DEFAULTS["gm_waves"])
    for gw in (12, 8):
        assert torch.equal(res[gw][0], res[16][0]) and torch.equal(res[gw][1], res[16][1])
        for k, ref in res[16][3].items():
            d = (res[gw][3][k] - ref).abs().max().item()
            assert d <= 1e-5 * ref.abs().max().item() + 1e-9, (gw, k, d, ref.abs().max().item())


@pytest.mark.parametrize("seg,P", [(512, 520), (512, 700), (512, 1030), (512, 1300), (512, 1540), (512, 2100), (512, 2570),
                                   (512, 4100), (2048, 4200), (2048, 9000), (4096, 4200), (4096, 9000), (4096, 13000)])
def test_merge_rank_search_over_segment_lengths(seg, P):
    """One tile: its list is cut into 2..8 segments of many different lengths (powers of two, one more, one less, a short
    last segment), each sorted by the four-keys-per-lane bitonic network (LDS round trips at every segment size), and every
    key is ranked in the others by the bounded branch-free search of bin_merge_emit_kernel; the sorted order must be the
    oracle's (images and gradients follow from it)."""
    try:
        _lib.set_option("bin_mode", 1)  # (the default, bin_mode 2, ranks a tile's keys in one bucket pass: tests/test_binning.py)
        _lib.set_option("seg", seg)
        _check(dict(P=P, F=3, W=16, H=16, neg=False))
    finally:
        _lib.set_option("seg", _DEFAULTS["seg"])
        _lib.set_option("bin_mode", _DEFAULTS["bin_mode"])


def _raw_forward(d, kwd, P, F, W=128, H=128):
    from manigaussian_amd import _C
    e = torch.Tensor([])
    return _C.rasterize_gaussians(kwd["bg"], d["means3D"], e, d["language_feature"], d["opacities"], d["scales"],
                                  d["rotations"], 1.0, e, kwd["viewmatrix"], kwd["projmatrix"], kwd["tanfovx"],
                                  kwd["tanfovy"], H, W, d["shs"], 1, kwd["campos"], False, False, True)


import contextlib


@contextlib.contextmanager
def _marks_only():
    """The opt-in asynchronous mode with workspaces sized from the high-water marks even for shapes whose worst-case workspace
    is small enough to be allocated outright: the tests of the marks / overflow machinery need it."""
    import manigaussian_amd as mg
    from manigaussian_amd import _state
    old = _state._SAFE_BYTES  # (None: the default)
    mg.set_safe_workspace(0)
    old_mode = mg.set_forward_mode("async")
    try:
        yield
    finally:
        _state.set_safe_bytes(old)
        mg.set_forward_mode(old_mode)


@contextlib.contextmanager
def _forward_mode(mode):
    import manigaussian_amd as mg
    old = mg.set_forward_mode(mode)
    try:
        yield
    finally:
        mg.set_forward_mode(old)


def test_capacity_retry_and_two_call_path_match_fused_forward():
    with _marks_only():
        _impl_test_capacity_retry_and_two_call_path_match_fused_forward()


def _impl_test_capacity_retry_and_two_call_path_match_fused_forward():
    """The fused forward sizes the binning workspace from a guess; when the guess is too small it reports
    MGS_NEED_CAPACITY and the shim re-bins with the exact count.  The reference-shaped two-call path
    (preprocess -> host read-back -> render) must give the same images as both."""
    import ctypes
    from manigaussian_amd import _C, _state
    dev = torch.device("cuda:0")
    sc, cam, kw, dC, dF = util.scene_case(P=5000, F=32)
    d = {k: v.to(dev) for k, v in sc.items()}
    kwd = syn.camera_settings_kwargs(cam, 1, True, bg=(0.1, 0.2, 0.3), device=dev)
    e = torch.Tensor([])
    R0, c0, f0, r0 = _raw_forward(d, kwd, 5000, 32)[:4]
    st = _state.device_state(dev)
    key = (5000, 128, 128, 32, 1)
    import manigaussian_amd as mg
    mg.check_status(dev)                     # the marks are learned from the device's report: the instances actually BINNED
    assert 0 < st.marks[key][0] <= R0        # (R0 is the reference's 3-sigma-rect count: at least as many)
    binned = st.marks[key][0]
    st.marks[key] = [16, None]               # far too small: forces the retry (blocking entry point)
    R1, c1, f1, r1 = _raw_forward(d, kwd, 5000, 32)[:4]
    assert R1 == R0 and torch.equal(c1, c0) and torch.equal(f1, f0) and torch.equal(r1, r0)
    assert st.marks[key][0] == binned        # the high-water mark was learnt again: the BINNED count, not the returned
    #                                          3-sigma-rect integer (advisor r4: that one would inflate every later workspace)
    # two-call path through the C ABI
    L = _lib.lib()
    u8 = dict(dtype=torch.uint8, device=dev)
    geom = torch.empty(L.mgs_geom_bytes(5000, 4, 128, 128), **u8)
    img = torch.empty(L.mgs_img_bytes(128, 128), **u8)
    a = _lib.MgsRasterArgs()
    _C._fill_args(a, P=5000, D=1, M=4, F=32, W=128, H=128, tanfovx=kwd["tanfovx"], tanfovy=kwd["tanfovy"],
                  scale_modifier=1.0, prefiltered=False, debug=False, include_feature=True, background=kwd["bg"],
                  means3D=d["means3D"], sh=d["shs"], colors=e, language_feature=d["language_feature"],
                  opacity=d["opacities"], scales=d["scales"], rotations=d["rotations"], cov3D_precomp=e,
                  viewmatrix=kwd["viewmatrix"], projmatrix=kwd["projmatrix"], campos=kwd["campos"], geom=geom,
                  binning=None, img=img)   # a zero-initialised MgsOptions: all defaults
    radii = torch.empty(5000, dtype=torch.int32, device=dev)
    nr = ctypes.c_int32(0)
    _lib.check(L.mgs_rasterize_forward_preprocess(ctypes.byref(a), radii.data_ptr(), ctypes.byref(nr), None), "pre")
    assert nr.value == R0 and torch.equal(radii, r0)
    binning = torch.empty(L.mgs_binning_bytes(nr.value, 128, 128, 32), **u8)
    a.binning, a.binning_bytes = binning.data_ptr(), binning.numel()
    c2, f2 = torch.empty_like(c0), torch.empty_like(f0)
    _lib.check(L.mgs_rasterize_forward_render(ctypes.byref(a), nr.value, radii.data_ptr(), c2.data_ptr(), f2.data_ptr(),
                                              None), "render")
    torch.cuda.synchronize()
    assert torch.equal(c2, c0) and torch.equal(f2, f0)
    # a binning workspace that is too small is refused, not overrun
    a.binning_bytes = L.mgs_binning_bytes(nr.value // 2, 128, 128, 32)
    assert L.mgs_rasterize_forward_render(ctypes.byref(a), nr.value, radii.data_ptr(), c2.data_ptr(), f2.data_ptr(),
                                          None) == _lib.MGS_ERR_WORKSPACE
    # ... and so is an explicit (capacity, pool) pair that does not fit the buffer
    a.binning_bytes = binning.numel()
    a.binning_capacity, a.chunk_pool = nr.value * 4, 0
    assert L.mgs_rasterize_forward_render(ctypes.byref(a), nr.value, radii.data_ptr(), c2.data_ptr(), f2.data_ptr(),
                                          None) == _lib.MGS_ERR_WORKSPACE


def _train_step(d, rast, dC, dF, between=None):
    leaves = {k: v.detach().requires_grad_(True) for k, v in d.items()}
    c, f, r = rast(leaves["means3D"], torch.zeros_like(leaves["means3D"]), leaves["opacities"], shs=leaves["shs"],
                   language_feature_precomp=leaves["language_feature"], scales=leaves["scales"],
                   rotations=leaves["rotations"])
    if between is not None:
        between()
    grads = torch.autograd.grad([c, f], list(leaves.values()), [dC, dF])
    return c, f, r, grads


@pytest.mark.parametrize("bin_mode", [2, 1, 0], ids=["bucket_rank", "lds_tables", "tables_in_memory"])
def test_async_forward_equals_blocking_forward_and_never_synchronises(bin_mode):
    """(bin_mode 0: the table kernel of the in-memory scatter is the one that reports to the host.)"""
    _lib.set_option("bin_mode", bin_mode)
    try:
        with _marks_only():
            _impl_test_async_forward_equals_blocking_forward_and_never_synchronises()
    finally:
        _lib.set_option("bin_mode", _DEFAULTS["bin_mode"])


def _impl_test_async_forward_equals_blocking_forward_and_never_synchronises():
    """Steady state (third call of a shape onwards): the forward returns without reading anything back -- the workspace
    comes from the high-water marks, the chunk pool is a fraction of the worst case -- and images / gradients are bit
    for bit those of the blocking path (same kernels, same order; only the record indices differ)."""
    import manigaussian_amd as mg
    from manigaussian_amd import _state
    dev = torch.device("cuda:0")
    P, F, W = 30000, 32, 128
    sc, cam, kw, dC, dF = util.scene_case(P=P, F=F)
    d = {k: v.to(dev) for k, v in sc.items()}
    rast = GaussianRasterizer(GaussianRasterizationSettings(**syn.camera_settings_kwargs(cam, 1, True, device=dev)))
    dC, dF = dC.to(dev), dF.to(dev)
    _old_mode = mg.set_forward_mode("blocking")
    try:
        c0, f0, r0, g0 = _train_step(d, rast, dC, dF)
        torch.cuda.synchronize()
    finally:
        mg.set_forward_mode(_old_mode)
    st = _state.device_state(dev)
    key = (P, W, W, F, 1)
    for _ in range(3):  # learn both marks (the chunk-record mark arrives with the render's report)
        _train_step(d, rast, dC, dF)
        mg.check_status(dev)
    R_mark, chunk_mark = st.marks[key]
    assert chunk_mark is not None and 0 < chunk_mark <= _lib.lib().mgs_chunk_pool_max(R_mark, W, W) // 2
    # the asynchronous step: enqueue a long-running kernel first; the forward must return while it is still running
    spin = torch.empty(64 << 20, device=dev)
    ev = torch.cuda.Event()
    for _ in range(20):
        spin.add_(1.0)
    c1, f1, r1, g1 = _train_step(d, rast, dC, dF)
    ev.record()
    returned_early = not ev.query()   # fwd + bwd were enqueued behind ~20 big fills and we are already back
    torch.cuda.synchronize()
    mg.check_status(dev)
    assert returned_early, "the forward waited for the device"
    assert torch.equal(c1, c0) and torch.equal(f1, f0) and torch.equal(r1, r0)
    for a, b in zip(g1, g0):
        assert (a - b).abs().max().item() <= 2e-5 * b.abs().max().item() + 1e-12  # float atomics: order differs run to run


def test_async_overflow_is_reported_loudly_and_recovers():
    with _marks_only():
        _impl_test_async_overflow_is_reported_loudly_and_recovers()


def _impl_test_async_overflow_is_reported_loudly_and_recovers():
    """A scene that outgrows the marks of its shape (both kinds: too few instances, too few chunk records).
    (a) The training-loop case: by the time the backward is reached the forward has long finished (here: a synchronise
        stands in for the loss and the rest of the network) -- the overflow is known at backward entry, the forward is
        re-rendered on the blocking path into the same output tensors, NO exception, a RuntimeWarning, and images and
        gradients equal those of the blocking path.
    (b) The host-ahead case: forward and backward are both enqueued before the device has reported (they sit behind a
        long fill) -- the step is lost and the next call into the library raises, loudly.
    Either way the marks are raised and the shape renders correctly afterwards."""
    import warnings
    import manigaussian_amd as mg
    from manigaussian_amd import _state
    dev = torch.device("cuda:0")
    P, F, W = 8000, 3, 128
    sc, cam, kw, dC, dF = util.scene_case(P=P, F=F)
    d = {k: v.to(dev) for k, v in sc.items()}
    rast = GaussianRasterizer(GaussianRasterizationSettings(**syn.camera_settings_kwargs(cam, 1, True, device=dev)))
    dC, dF = dC.to(dev), dF.to(dev)
    _old_mode = mg.set_forward_mode("blocking")
    try:
        c0, f0, r0, g0 = _train_step(d, rast, dC, dF)
        torch.cuda.synchronize()
    finally:
        mg.set_forward_mode(_old_mode)
    for _ in range(3):
        _train_step(d, rast, dC, dF)
        mg.check_status(dev)
    st = _state.device_state(dev)
    key = (P, W, W, F, 1)
    good = list(st.marks[key])

    def same_as_blocking(c1, f1, r1, g1):
        assert torch.equal(c1, c0) and torch.equal(f1, f0) and torch.equal(r1, r0)
        for a, b in zip(g1, g0):
            assert (a - b).abs().max().item() <= 2e-5 * b.abs().max().item() + 1e-12  # float atomics: order differs

    for bad in ([64, good[1]], [good[0], 1]):   # too few instances / too few chunk records
        # (a) the report is in before the backward: repaired, not raised
        st.marks[key] = list(bad)
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            c1, f1, r1, g1 = _train_step(d, rast, dC, dF, between=torch.cuda.synchronize)
            torch.cuda.synchronize()
            mg.check_status(dev)               # nothing left to raise
        assert any("outgrew the workspace" in str(x.message) for x in w), [str(x.message) for x in w]
        same_as_blocking(c1, f1, r1, g1)
        assert st.marks[key][0] >= good[0]
        for _ in range(3):
            c1, f1, r1, g1 = _train_step(d, rast, dC, dF)
            mg.check_status(dev)
        same_as_blocking(c1, f1, r1, g1)
        assert st.marks[key][1] is not None and st.marks[key][1] >= good[1]
        # (b) forward AND backward enqueued before the device could report: loud, late
        st.marks[key] = list(bad)
        spin = torch.empty(64 << 20, device=dev)
        with pytest.raises(RuntimeError, match="outgrew the workspace"):
            for _ in range(20):
                spin.add_(1.0)
            _train_step(d, rast, dC, dF)
            mg.check_status(dev)
        for _ in range(3):
            c1, f1, r1, g1 = _train_step(d, rast, dC, dF)
            mg.check_status(dev)
        same_as_blocking(c1, f1, r1, g1)
        assert st.marks[key][0] >= good[0] and st.marks[key][1] is not None and st.marks[key][1] >= good[1]


def test_async_overflow_policy_raise_loses_the_step_instead_of_repairing_it():
    """set_overflow_policy("raise") (round-3 advisor finding: a repaired step still mixes a loss computed from incomplete images
    with gradients of the complete render): the overflow known at backward entry raises, nothing is repaired, no warning; the
    marks are raised and the next steps render like the blocking path."""
    import warnings
    import manigaussian_amd as mg
    from manigaussian_amd import _state
    dev = torch.device("cuda:0")
    P, F, W = 7000, 3, 128
    sc, cam, kw, dC, dF = util.scene_case(P=P, F=F)
    d = {k: v.to(dev) for k, v in sc.items()}
    rast = GaussianRasterizer(GaussianRasterizationSettings(**syn.camera_settings_kwargs(cam, 1, True, device=dev)))
    dC, dF = dC.to(dev), dF.to(dev)
    with _forward_mode("blocking"):
        c0, f0, r0, g0 = _train_step(d, rast, dC, dF)
        torch.cuda.synchronize()
    old_policy = mg.set_overflow_policy("raise")
    try:
        with _marks_only():
            for _ in range(3):
                _train_step(d, rast, dC, dF)
                mg.check_status(dev)
            st = _state.device_state(dev)
            key = (P, W, W, F, 1)
            good = list(st.marks[key])
            st.marks[key] = [64, good[1]]
            with warnings.catch_warnings(record=True) as w:
                warnings.simplefilter("always")
                with pytest.raises(RuntimeError, match="outgrew"):
                    _train_step(d, rast, dC, dF, between=torch.cuda.synchronize)
                    mg.check_status(dev)
            assert not any("re-renders" in str(x.message) for x in w)
            torch.cuda.synchronize()
            assert st.marks[key][0] >= good[0]
            for _ in range(3):
                c1, f1, r1, g1 = _train_step(d, rast, dC, dF)
                mg.check_status(dev)
            assert torch.equal(c1, c0) and torch.equal(f1, f0) and torch.equal(r1, r0)
    finally:
        mg.set_overflow_policy(old_policy)


def test_async_overflow_of_a_view_batch_is_repaired_at_backward_entry():
    """The same repair for GaussianRasterizerBatch (mgs_rasterize_forward_views): marks far too small, the report is in before
    the backward -> re-rendered on the blocking path, a warning, images and gradients of the blocking path."""
    import warnings
    import manigaussian_amd as mg
    from manigaussian_amd import GaussianRasterizerBatch, _state
    with _marks_only():
        dev = torch.device("cuda:0")
        P, F, V, W = 5000, 32, 3, 64
        sc, cams, dC, dF = _batch_case(P, F, V, W, W)
        sets = [GaussianRasterizationSettings(**syn.camera_settings_kwargs(c, 1, True, bg=(0.1, 0.2, 0.3), device=dev))
                for c in cams]
        rast = GaussianRasterizerBatch(sets)
        dCd, dFd = dC.to(dev), dF.to(dev)

        def step(between=None):
            d = {k: v.to(dev).clone().requires_grad_(True) for k, v in sc.items()}
            c, f, r = rast(d["means3D"], None, d["opacities"], shs=d["shs"], language_feature_precomp=d["language_feature"],
                           scales=d["scales"], rotations=d["rotations"])
            if between is not None:
                between()
            gs = torch.autograd.grad([c, f], list(d.values()), [dCd, dFd])
            return c, f, r, gs

        _old_mode = mg.set_forward_mode("blocking")
        try:
            c0, f0, r0, g0 = step()
            torch.cuda.synchronize()
        finally:
            mg.set_forward_mode(_old_mode)
        for _ in range(3):
            step()
            mg.check_status(dev)
        st = _state.device_state(dev)
        key = ("views", V, P, W, W, F, 1)
        good = list(st.marks[key])
        for bad in ([64, good[1]], [good[0], 1]):
            st.marks[key] = list(bad)
            with warnings.catch_warnings(record=True) as w:
                warnings.simplefilter("always")
                c1, f1, r1, g1 = step(between=torch.cuda.synchronize)
                torch.cuda.synchronize()
                mg.check_status(dev)
            assert any("outgrew the workspace" in str(x.message) for x in w)
            assert torch.equal(c1, c0) and torch.equal(f1, f0) and torch.equal(r1, r0)
            for a_, b_ in zip(g1, g0):
                assert (a_ - b_).abs().max().item() <= 2e-5 * b_.abs().max().item() + 1e-12
            for _ in range(3):
                step()
                mg.check_status(dev)


def test_raw_C_forward_backward_pair_agrees_with_the_autograd_path():
    """The reference-shaped pybind pair _C.rasterize_gaussians -> _C.rasterize_gaussians_backward(R: int, binningBuffer)
    (RAST/rasterize_points.cu:35-225): the backward is handed nothing but the three byte buffers and the count, so forward
    and backward must derive the same carving from the buffer sizes.  Called twice for one shape: the second forward's
    buffer is sized from the first one's count (an arbitrary number, not a multiple of 16)."""
    from manigaussian_amd import _C
    dev = torch.device("cuda:0")
    P, F = 7001, 32
    sc, cam, kw, dC, dF = util.scene_case(P=P, F=F)
    d = {k: v.to(dev) for k, v in sc.items()}
    kwd = syn.camera_settings_kwargs(cam, 1, True, bg=(0.1, 0.2, 0.3), device=dev)
    dCd, dFd = dC.to(dev), dF.to(dev)
    e = torch.Tensor([])
    ch, fh, rh, gh = util.run_hip(sc, cam, dC, dF, 1, True, (0.1, 0.2, 0.3))
    for rep in range(2):
        R, c, f, radii, geom, binning, img = _raw_forward(d, kwd, P, F)
        assert isinstance(R, int) and R > 0
        out = _C.rasterize_gaussians_backward(kwd["bg"], d["means3D"], radii, e, d["language_feature"], d["scales"],
                                              d["rotations"], 1.0, e, kwd["viewmatrix"], kwd["projmatrix"], kwd["tanfovx"],
                                              kwd["tanfovy"], dCd, dFd, d["shs"], 1, kwd["campos"], geom, R, binning, img,
                                              False, True)
        torch.cuda.synchronize()
        g_means2D, g_colors, g_feat, g_op, g_means3D, g_cov3D, g_sh, g_scales, g_rot = out
        assert torch.equal(c.cpu(), ch) and torch.equal(f.cpu(), fh) and torch.equal(radii.cpu(), rh)
        got = {"means3D": g_means3D, "means2D": g_means2D, "opacities": g_op, "scales": g_scales, "rotations": g_rot,
               "shs": g_sh, "language_feature": g_feat}
        for k, v in got.items():
            ref = gh[k]
            assert (v.cpu() - ref).abs().max().item() <= 2e-5 * ref.abs().max().item() + 1e-12, (rep, k)


def test_small_shapes_get_their_worst_case_workspace_and_cannot_overflow():
    """A shape whose worst-case workspace fits the budget (default 1 GB; ManiGaussian's 16 384 Gaussians need 206 MB) is given
    that workspace from the first call on: asynchronous immediately, no marks involved, and a scene that is 50 times denser
    than the previous one of its shape renders correctly (with the marks alone it would overflow and raise)."""
    import manigaussian_amd as mg
    from manigaussian_amd import _state
    dev = torch.device("cuda:0")
    P, F = 6001, 3  # a shape no other test uses: no marks exist
    sc, cam, kw, dC, dF = util.scene_case(P=P, F=F)
    rast = GaussianRasterizer(GaussianRasterizationSettings(**syn.camera_settings_kwargs(cam, 1, True, device=dev)))
    st = _state.device_state(dev)
    assert (P, 128, 128, F, 1) not in st.marks
    small = {k: v.to(dev) for k, v in sc.items()}
    small["scales"] = small["scales"] * 0.05
    big = {k: v.to(dev) for k, v in sc.items()}
    big["scales"] = big["scales"] * 4.0
    outs = {}
    for name, d in (("small", small), ("big", big)):
        c, f, r = rast(d["means3D"], torch.zeros(P, 3, device=dev), d["opacities"], shs=d["shs"],
                       language_feature_precomp=d["language_feature"], scales=d["scales"], rotations=d["rotations"])
        mg.check_status(dev)  # would raise if the second scene had outgrown a workspace sized from the first
        outs[name] = (c, f, r)
    with _marks_only():  # the same two scenes through the blocking path (exact sizes)
        _old_mode = mg.set_forward_mode("blocking")
        try:
            for name, d in (("small", small), ("big", big)):
                c, f, r = rast(d["means3D"], torch.zeros(P, 3, device=dev), d["opacities"], shs=d["shs"],
                               language_feature_precomp=d["language_feature"], scales=d["scales"], rotations=d["rotations"])
                assert torch.equal(c, outs[name][0]) and torch.equal(f, outs[name][1]) and torch.equal(r, outs[name][2])
        finally:
            mg.set_forward_mode(_old_mode)
    assert int((outs["big"][2] > 0).sum()) > 0


def test_default_mode_never_returns_incomplete_images_when_a_scene_grows():
    """under the DEFAULT options ("safe" forward mode) an abruptly growing scene of a shape whose
    worst-case workspace does NOT fit the budget (forced here with a 1 MB budget; BASELINE configs[2] needs 4 GB against the
    default 1 GB) yields the correct images and gradients in the very call that grew, with no warning and nothing to raise
    later -- the reference's behaviour (RAST/cuda_rasterizer/rasterizer_impl.cu:282-284 sizes the buffer from the count it
    waited for).  Three scenes of one shape in a row: sparse, 80 x denser, sparse again; single view and a 3-view batch."""
    import warnings
    import manigaussian_amd as mg
    from manigaussian_amd import GaussianRasterizerBatch, _state
    assert mg.forward_mode() == "safe", "the package default must be the mode that cannot return incomplete images"
    dev = torch.device("cuda:0")
    P, F, W = 9001, 32, 128
    sc, cam, kw, dC, dF = util.scene_case(P=P, F=F)
    cams = syn.circle_cameras(3, W, W, negative_focal=True)
    mk = lambda c: GaussianRasterizationSettings(**syn.camera_settings_kwargs(c, 1, True, bg=(0.1, 0.2, 0.3), device=dev))  # noqa: E731
    rast, rastV = GaussianRasterizer(mk(cam)), GaussianRasterizerBatch([mk(c) for c in cams])
    dCd, dFd = dC.to(dev), dF.to(dev)
    dCv, dFv = torch.stack([dCd] * 3), torch.stack([dFd] * 3)
    scenes = []
    for mult in (0.05, 4.0, 0.05):
        d = {k: v.to(dev) for k, v in sc.items()}
        d["scales"] = d["scales"] * mult
        scenes.append(d)

    def step(d, batched):
        leaves = {k: v.clone().requires_grad_(True) for k, v in d.items()}
        if batched:
            c, f, r = rastV(leaves["means3D"], None, leaves["opacities"], shs=leaves["shs"],
                            language_feature_precomp=leaves["language_feature"], scales=leaves["scales"],
                            rotations=leaves["rotations"])
            gs = torch.autograd.grad([c, f], list(leaves.values()), [dCv, dFv])
        else:
            c, f, r = rast(leaves["means3D"], torch.zeros(P, 3, device=dev), leaves["opacities"], shs=leaves["shs"],
                           language_feature_precomp=leaves["language_feature"], scales=leaves["scales"],
                           rotations=leaves["rotations"])
            gs = torch.autograd.grad([c, f], list(leaves.values()), [dCd, dFd])
        return c, f, r, gs

    old_budget = _state._SAFE_BYTES  # (None: the default)
    mg.set_safe_workspace(1)
    try:
        for batched in (False, True):
            with _forward_mode("blocking"):  # the expected values: every scene on the blocking path, on its own
                want = [step(d, batched) for d in scenes]
                torch.cuda.synchronize()
            with warnings.catch_warnings(record=True) as w:
                warnings.simplefilter("always")
                got = [step(d, batched) for d in scenes]
                torch.cuda.synchronize()
                mg.check_status(dev)  # nothing to raise
            assert not [x for x in w if issubclass(x.category, RuntimeWarning)], [str(x.message) for x in w]
            for (c1, f1, r1, g1), (c0, f0, r0, g0) in zip(got, want):
                assert torch.equal(c1, c0) and torch.equal(f1, f0) and torch.equal(r1, r0)
                for a, b in zip(g1, g0):
                    assert (a - b).abs().max().item() <= 2e-5 * b.abs().max().item() + 1e-12  # float atomics: order differs
    finally:
        _state.set_safe_bytes(old_budget)


def test_forward_backward_captured_into_a_hip_graph_replays_bit_identically():
    """fwd + bwd through the public autograd API captured with torch.cuda.graph (tests/tools/graph_capture_check.py, in a
    process of its own: stream capture is process-wide state): the capture succeeds because the library never
    synchronises, replays reproduce the eager images bit for bit and follow in-place parameter updates."""
    run_graph_tool("graph_capture_check.py", limit=170)


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[:-4] for p in GOLDEN])
def test_golden_vectors(path):
    z = np.load(path)
    case = eval(bytes(z["case"]).decode())
    sc = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("in_")}
    cam = {k[4:]: (torch.from_numpy(z[k]) if z[k].ndim else z[k].item()) for k in z.files if k.startswith("cam_")}
    inc = case.get("include_feature", True)
    dC = torch.from_numpy(z["d_color"])
    dF = torch.from_numpy(z["d_feat"]) if "d_feat" in z.files else None
    ch, fh, rh, gh = util.run_hip(sc, cam, dC, dF, case.get("sh_degree", 1), inc, case.get("bg", (0.1, 0.2, 0.3)))
    assert np.array_equal(rh.numpy(), z["radii"])
    pairs = [(ch.numpy(), z["out_color"])] + ([(fh.numpy(), z["out_feat"])] if inc else [])
    # the file carries Oracle B's own fragility masks (pixels / Gaussians with a pair within 2e-5 of a hard threshold):
    # everything unmarked must meet the contract, the marked ones the flipped-pair bound
    frag_px, frag_g = z["fragile_pixels"].astype(bool), z["fragile_gaussians"].astype(bool)
    assert frag_px.mean() <= util.FRAGILE_MAX_FRACTION
    for a, b in pairs:
        e = np.abs(a - b).max(0)
        assert (e[~frag_px].max() if (~frag_px).any() else 0.0) <= IMG_TOL and e.max() <= util.FRAGILE_TOL
    for k, v in gh.items():
        ref = z["grad_" + util.GRAD_KEYS[k]].reshape(v.shape)
        if ref.size:
            e = np.abs(v.numpy() - ref).reshape(ref.shape[0], -1).max(1)
            assert (e[~frag_g].max() if (~frag_g).any() else 0.0) <= GRAD_TOL * np.abs(ref).max() + 1e-7, k
            assert e.max() <= util.FRAGILE_GRAD_TOL * np.abs(ref).max() + 1e-7, k


def _check_against_reference(got, ref, inc, tag, state=None):
    """got / ref = (color, feat, radii, grads by Oracle-B name).  Both sides ran on gfx950: radii bit-exact, images 2e-5,
    gradients 1e-3 of the tensor max (measured: <= 2e-6 and <= 1e-4, profiles/r01_ref_compare.log).
    state (an Oracle-B run of the same scene): the library evaluates exp() with v_exp_f32 (relative error ~2e-7), the
    reference with ocml's expf, so a (pixel, Gaussian) pair within that distance of a hard threshold (alpha < 1/255,
    T < 1e-4) may be decided differently -- a handful of pairs among the 10^8..10^9 of the large cases.  The pixels /
    Gaussians Oracle B marks as sitting within 2e-5 (relative) of such a threshold get REF_FRAGILE_TOL (5e-4) /
    REF_FRAGILE_GRAD_TOL (3e-3 of the max) and at most REF_MAX_PIXELS_ABOVE_CONTRACT pixels of an image may exceed 1e-4;
    everything else the strict bound (2e-5 / 1e-3).  The measured values go to $MGS_PARITY_REPORT."""
    (ch, fh, rh, gh), (cr, fr, rr, gr) = got, ref
    assert np.array_equal(np.asarray(rh), np.asarray(rr)), tag
    frag_px = frag_g = None
    if state is not None:
        from oracle import oracle_b
        frag_px, frag_g = oracle_b.fragile_mask(state).numpy(), oracle_b.fragile_gaussians(state).numpy()
        assert frag_px.mean() <= util.FRAGILE_MAX_FRACTION, tag
    stats = {}
    for nm, a, b in [("color", ch, cr)] + ([("feature", fh, fr)] if inc else []):
        e = np.abs(np.asarray(a) - np.asarray(b)).max(0)
        above = int((e > IMG_TOL).sum())
        stats[nm] = dict(max=float(e.max()), pixels_above_1e_4=above,
                         max_unmarked=float(e[~frag_px].max()) if frag_px is not None and (~frag_px).any() else float(e.max()))
        if frag_px is None:
            assert e.max() <= 2e-5, (tag, nm, e.max())
        else:
            assert e[~frag_px].max() <= 2e-5, (tag, nm, e[~frag_px].max())
            assert e.max() <= util.REF_FRAGILE_TOL, (tag, nm, e.max())
            assert above <= util.REF_MAX_PIXELS_ABOVE_CONTRACT, (tag, nm, above)
    for k, v in gh.items():
        r = np.asarray(gr[util.GRAD_KEYS[k]])
        if k == "language_feature" and not inc:
            continue
        if r.size:
            e = np.abs(v.numpy() - r.reshape(v.shape)).reshape(v.shape[0], -1).max(1)
            mag = np.abs(r).max()
            stats["grad_" + k] = dict(max_rel=float(e.max() / (mag + 1e-30)))
            if frag_g is None:
                assert e.max() <= GRAD_TOL * mag + 1e-7, (tag, k)
            else:
                assert e[~frag_g].max() <= GRAD_TOL * mag + 1e-7, (tag, k)
                assert e.max() <= util.REF_FRAGILE_GRAD_TOL * mag + 1e-7, (tag, k, e.max() / mag)
    util.report(tag, against="reference kernels", **stats)


@pytest.mark.parametrize("path", REF_GOLDEN, ids=[os.path.basename(p)[:-4] for p in REF_GOLDEN])
def test_reference_kernel_golden_vectors(path):
    """The HIP path against outputs of the REFERENCE's own kernels (tests/golden/ref/*.npz, produced on an MI355X by
    tests/golden/make_golden_ref.py from oracle/_ref = the reference's forward.cu/backward.cu/rasterizer_impl.cu built
    with hipcc)."""
    z = np.load(path)
    case = eval(bytes(z["case"]).decode())
    sc, cam, kw, dC, dF = util.scene_case(**case)
    sc = util.stored_inputs(z, sc)
    inc = case.get("include_feature", True)
    got = util.run_hip(sc, cam, dC, dF, case.get("sh_degree", 1), inc, case.get("bg", (0.1, 0.2, 0.3)),
                       scale_modifier=case.get("scale_modifier", 1.0))
    ref = (z["out_color"], z["out_feat"], z["radii"], {k[5:]: z[k] for k in z.files if k.startswith("grad_")})
    _check_against_reference(got, ref, inc, os.path.basename(path))


@pytest.mark.parametrize("case", [
    dict(P=100000, F=32, W=128, H=128, neg=True, bg=(0.0, 0.0, 0.0), seed=0, cam_index=0),  # = BASELINE configs[2]
    dict(P=100000, F=3, W=128, H=128, neg=True, bg=(0.0, 0.0, 0.0), seed=12),               # = BASELINE configs[1]
    dict(P=20000, F=32, W=200, H=120, neg=False, bg=(0.2, 0.1, 0.0), seed=15, M=9, sh_degree=2),
    dict(P=30000, F=3, W=256, H=192, neg=False, bg=(0.3, 0.3, 0.3), seed=13, M=16, sh_degree=3),
    dict(P=50000, F=3, W=128, H=128, neg=True, colors_precomp=True, include_feature=False, seed=14),
    dict(P=500000, F=32, W=256, H=256, neg=True, bg=(0.0, 0.0, 0.0), seed=0),               # = BASELINE configs[4] shape
    dict(P=16384, F=3, W=128, H=128, neg=True, bg=(0.0, 0.0, 0.0), seed=16),                # ManiGaussian's own workload
    dict(P=40000, F=8, W=128, H=128, neg=True, bg=(0.1, 0.0, 0.2), seed=17),                # a third width (reference rebuilt)
    dict(P=30000, F=3, W=128, H=128, neg=True, bg=(0.0, 0.0, 0.0), seed=18, scale_modifier=0.5),
    dict(P=30000, F=32, W=128, H=128, neg=False, bg=(0.0, 0.0, 0.0), seed=19, scale_modifier=2.0),
], ids=["c3_p100k_f32", "c2_p100k_f3", "f32_sh2_200x120", "sh3_256x192", "precomp_rgb_only_50k", "c5_p500k_256_f32",
        "manigaussian_16k_f3", "f8_p40k", "scale_modifier_0p5_f3", "scale_modifier_2_f32"])
def test_live_reference(case):
    """The HIP path against the reference's own kernels run LIVE on this GPU (oracle/_ref/libmgs_ref.so, prebuilt in the
    development container from /root/reference; the GPU box never reads /root/reference; the F = 32 cases use the same
    sources rebuilt at that feature width).  Skipped where the library was not built."""
    from oracle import ref_cuda
    if not ref_cuda.available(case["F"]):
        pytest.skip("oracle/_ref/libmgs_ref*.so not built (needs /root/reference at build time)")
    sc, cam, kw, dC, dF = util.scene_case(**case)
    inc = case.get("include_feature", True)
    cr, fr, rr, gr, R = util.run_reference(sc, kw, dC, dF)
    got = util.run_hip(sc, cam, dC, dF, case.get("sh_degree", 1), inc, case.get("bg", (0.1, 0.2, 0.3)),
                       scale_modifier=case.get("scale_modifier", 1.0))
    state = util.run_oracle_b(sc, kw, dC, dF)[4]  # only to know which pixels sit on a hard threshold
    _check_against_reference(got, (cr, fr, rr, gr), inc, repr(case), state=state)
    # The integer the reference returns first (RAST/rasterize_points.cu:127 <- rasterizer_impl.cu:282-284):
    # _C.rasterize_gaussians()[0] IS that number under the default options (since round 4) and under tight_bins = 0 -- the
    # preprocess counts the reference's 3-sigma-rect instances beside the ones it bins (fewer under tight_bins = 1).
    R_ref, R_hip = int(R), {}
    for tight in (0, 1):
        R_hip[tight] = _num_rendered(sc, cam, case, tight)
    assert R_hip[0] == R_hip[1] == R_ref == int(state.num_rendered), (R_hip, R_ref, state.num_rendered)
    util.report(repr(case), num_rendered_reference=R_ref, num_rendered_tight0=R_hip[0], num_rendered_tight1=R_hip[1])


@pytest.mark.parametrize("case", [
    dict(P=100000, F=32, W=128, H=128, neg=True, bg=(0.0, 0.0, 0.0), seed=0, cam_index=0),  # = BASELINE configs[2]
    dict(P=500000, F=32, W=256, H=256, neg=True, bg=(0.0, 0.0, 0.0), seed=0),               # = BASELINE configs[4] shape
    dict(P=100000, F=3, W=128, H=128, neg=True, bg=(0.0, 0.0, 0.0), seed=12),               # = BASELINE configs[1]
], ids=["c3_p100k_f32", "c5_p500k_256_f32", "c2_p100k_f3"])
def test_live_reference_exact_exp_and_fast_exp(case):
    """is the exact-exp path exact, and what does v_exp_f32 cost in parity?
    With fast_exp = 0 -- the DEFAULT since round 4 -- the render kernels evaluate exp() with ocml's expf exactly as the
    reference's kernels, built by the same compiler, do (RAST/cuda_rasterizer/forward.cu:345-361; exp_ocml_unclamped, checked
    bit for bit against expf by mgs_selftest), and the preprocess hands them bit-identical inputs
    (test_preprocess_is_bit_identical_to_the_reference_kernels).  Asserted, at BASELINE configs[1], [2] and the configs[4]
    shape (500 000 Gaussians, 256^2, ~1e9 (pixel, Gaussian) pairs):
      * fast_exp = 0 (default): EVERY pixel within 2e-5 of the reference (measured <= 2.7e-6) and every gradient row within
        1e-5 of its tensor's max -- no fragile allowance, no pixel count: the three hard per-pair decisions fall the same way
        everywhere;
      * fast_exp = 1 (the option, 2.4 % faster): no pixel above the 1e-4 contract (measured: <= 9.5e-7 at 100 000 Gaussians;
        at 500 000 ONE pixel at 8.9e-5 -- a pair whose alpha sits within v_exp_f32's 2e-7 of 1/255; an alpha flip moves a
        pixel by up to T |c| / 255, so the option CAN exceed the contract on another scene), gradients within 1e-3."""
    from oracle import ref_cuda
    if not ref_cuda.available(case["F"]):
        pytest.skip("oracle/_ref/libmgs_ref*.so not built (needs /root/reference at build time)")
    sc, cam, kw, dC, dF = util.scene_case(**case)
    cr, fr, rr, gr, R = util.run_reference(sc, kw, dC, dF)
    old = _lib.get_option("fast_exp")
    for fe in (0, 1):
        try:
            _lib.set_option("fast_exp", fe)
            ch, fh, rh, gh = util.run_hip(sc, cam, dC, dF, 1, True, case.get("bg", (0.1, 0.2, 0.3)))
        finally:
            _lib.set_option("fast_exp", old)
        assert np.array_equal(np.asarray(rh), np.asarray(rr))
        stats = {}
        for nm, a, b in (("color", ch, cr), ("feature", fh, fr)):
            e = np.abs(np.asarray(a) - np.asarray(b)).max(0)
            stats[nm] = dict(max=float(e.max()), pixels_above_1e_4=int((e > IMG_TOL).sum()), pixels_above_2e_5=int((e > 2e-5).sum()))
        for k, v in gh.items():
            r = np.asarray(gr[util.GRAD_KEYS[k]])
            if r.size:
                e = np.abs(v.numpy() - r.reshape(v.shape)).reshape(v.shape[0], -1).max(1)
                stats["grad_" + k] = dict(max_rel=float(e.max() / (np.abs(r).max() + 1e-30)))
        util.report(repr(case), against=f"reference kernels, fast_exp = {fe}", **stats)
        for nm in ("color", "feature"):
            if fe == 0:
                assert stats[nm]["pixels_above_2e_5"] == 0, (fe, nm, stats[nm])
            else:
                assert stats[nm]["pixels_above_1e_4"] == 0, (fe, nm, stats[nm])
        for k, v in stats.items():
            if k.startswith("grad_"):
                assert v["max_rel"] <= (1e-5 if fe == 0 else GRAD_TOL), (fe, k, v)


@pytest.mark.parametrize("case", [
    dict(P=100000, F=32, W=128, H=128, neg=True, bg=(0.0, 0.0, 0.0), seed=0, cam_index=0),
    dict(P=500000, F=32, W=256, H=256, neg=True, bg=(0.0, 0.0, 0.0), seed=0),
    dict(P=100000, F=32, W=128, H=128, neg=True, bg=(0.0, 0.0, 0.0), seed=0, phase=0.37),
    dict(P=100000, F=32, W=128, H=128, neg=False, bg=(0.0, 0.0, 0.0), seed=7, phase=1.1),
], ids=["c3_100k", "c5_500k_256", "generic_camera_negfocal", "generic_camera_posfocal"])
def test_preprocess_is_bit_identical_to_the_reference_kernels(case):
    """What the forward preprocess hands to binning and compositing, against the reference kernels' GeometryState
    (RAST/cuda_rasterizer/rasterizer_impl.h:30-46, filled by forward.cu:156-257), BIT FOR BIT over every visible Gaussian:
    radii, view depth (the sort key), pixel mean, conic, opacity, SH colour, 3-D covariance -- also for cameras whose matrices
    hold no structural zeros (the other tests' cameras sit at multiples of 90 degrees, which hides how a 4-term dot product
    is rounded).  Round 4 found cov3D a few ulps apart on 90 % of the Gaussians and conics up to 85 ulps apart (same algebra,
    another fused-multiply-add pattern), and one pixel of the 500 000-Gaussian case 1.16e-4 off because of it; every rounding
    of the forward preprocess is now pinned in the kernel (mgs_preprocess.hip: cov3d_from_scale_rotation, view_cov,
    cov2d_from, cov2d_det, row_view_z / row_hom_w / row_hom_xy)."""
    import ctypes
    import types
    from oracle import ref_cuda
    from manigaussian_amd import _C
    if not ref_cuda.available(case["F"]):
        pytest.skip("oracle/_ref/libmgs_ref*.so not built (needs /root/reference at build time)")
    case = dict(case)
    phase = case.pop("phase", 0.0)
    sc, cam, kw, dC, dF = util.scene_case(**case)
    if phase:
        cam = syn.circle_cameras(4, case["W"], case["H"], negative_focal=case["neg"], phase=phase)[1]
        kw = syn.camera_settings_kwargs(cam, 1, True, bg=case["bg"])
    st = types.SimpleNamespace(**kw)
    ref = ref_cuda.forward_geometry(sc["means3D"], sc["opacities"], st, shs=sc["shs"], language_feature=sc["language_feature"],
                                    scales=sc["scales"], rotations=sc["rotations"])
    dev = torch.device("cuda:0")
    kwd = syn.camera_settings_kwargs(cam, 1, True, bg=case["bg"], device=dev)
    d = {k: v.to(dev) for k, v in sc.items()}
    e = torch.Tensor([])
    P, M, W, H = case["P"], 4, case["W"], case["H"]
    out = _C.rasterize_gaussians(kwd["bg"], d["means3D"], e, d["language_feature"], d["opacities"], d["scales"], d["rotations"],
                                 1.0, e, kwd["viewmatrix"], kwd["projmatrix"], kwd["tanfovx"], kwd["tanfovy"], H, W, d["shs"], 1,
                                 kwd["campos"], False, False, True)
    radii, geom = out[3].cpu().numpy(), out[4].cpu().numpy()
    offs = [ctypes.c_size_t(0) for _ in range(4)]
    _lib.check(_lib.lib().mgs_debug_geom_layout(P, M, W, H, *[ctypes.byref(o) for o in offs]), "geom layout")
    f = lambda o, n: np.frombuffer(geom, np.float32, n, int(o.value)).copy()  # noqa: E731
    rec = f(offs[1], 8 * P).reshape(P, 8)
    hip = dict(depths=f(offs[0], P), means2D=rec[:, 0:2], conic_opacity=rec[:, [2, 3, 4, 5]],
               rgb=f(offs[2], 3 * P).reshape(P, 3), cov3D=f(offs[3], 6 * P).reshape(P, 6))
    assert np.array_equal(radii, ref["radii"])
    vis = ref["radii"] > 0
    bits = lambda a: np.ascontiguousarray(a).view(np.int32)  # noqa: E731
    stats = {}
    for name, r_, h_ in (("depths", ref["depths"], hip["depths"]), ("means2D", ref["means2D"], hip["means2D"]),
                         ("rgb", ref["rgb"], hip["rgb"]), ("cov3D", ref["cov3D"], hip["cov3D"]),
                         ("conic_opacity", ref["conic_opacity"], hip["conic_opacity"])):
        differ = int((bits(r_[vis]) != bits(h_[vis])).sum())
        stats[name + "_values_that_differ"] = differ
    util.report(repr(case) + f" phase={phase}", against="reference kernels, GeometryState bits", visible=int(vis.sum()), **stats)
    assert not any(stats.values()), stats


def _num_rendered(sc, cam, case, tight):
    """_C.rasterize_gaussians(...)[0] -- the count as the reference's pybind entry point returns it -- under tight_bins."""
    from manigaussian_amd import _C
    dev = torch.device("cuda:0")
    inc = case.get("include_feature", True)
    kwd = syn.camera_settings_kwargs(cam, case.get("sh_degree", 1), inc, bg=case.get("bg", (0.1, 0.2, 0.3)), device=dev)
    d = {k: v.to(dev) for k, v in sc.items()}
    e = torch.Tensor([])
    old = _lib.get_option("tight_bins")
    try:
        _lib.set_option("tight_bins", tight)
        out = _C.rasterize_gaussians(kwd["bg"], d["means3D"], d.get("colors_precomp", e), d.get("language_feature", e),
                                     d["opacities"], d.get("scales", e), d.get("rotations", e),
                                     float(case.get("scale_modifier", 1.0)),
                                     d.get("cov3D_precomp", e), kwd["viewmatrix"], kwd["projmatrix"], kwd["tanfovx"],
                                     kwd["tanfovy"], kwd["image_height"], kwd["image_width"], d.get("shs", e),
                                     case.get("sh_degree", 1), kwd["campos"], False, False, inc)
    finally:
        _lib.set_option("tight_bins", old)
    assert isinstance(out[0], int)
    return out[0]


def test_edge_cases_empty_and_all_culled():
    dev = torch.device("cuda:0")
    sc, cam, kw, dC, dF = util.scene_case(P=50, F=3, W=32, H=32)
    st = GaussianRasterizationSettings(**syn.camera_settings_kwargs(cam, 1, True, bg=(0.1, 0.2, 0.3), device=dev))
    r = GaussianRasterizer(st)
    z = lambda *s: torch.zeros(*s, device=dev)
    # P == 0 (rasterize_points.cu:92): zero images, empty radii
    c, f, rad = r(z(0, 3), z(0, 3), z(0, 1), shs=z(0, 4, 3), language_feature_precomp=z(0, 3), scales=z(0, 3),
                  rotations=z(0, 4))
    assert c.shape == (3, 32, 32) and c.abs().max() == 0 and rad.numel() == 0
    # everything behind the camera: R == 0, image == background, all gradients zero
    fwd = cam["world_view_transform"].reshape(-1)[[2, 6, 10]]  # world direction of +view-z
    sc["means3D"] = sc["means3D"] * 0 + cam["camera_center"] - 3.0 * fwd
    ch, fh, rh, gh = util.run_hip(sc, cam, dC, dF, 1, True, (0.1, 0.2, 0.3))
    assert (rh == 0).all() and fh.abs().max() == 0
    assert torch.allclose(ch, torch.tensor([0.1, 0.2, 0.3]).reshape(3, 1, 1).expand_as(ch))
    assert all(v.abs().max() == 0 for v in gh.values())
    assert not r.markVisible(sc["means3D"].to(dev)).any()


def test_mark_visible_matches_oracle():
    from oracle import oracle_b
    sc, cam, kw, _, _ = util.scene_case(P=5000, F=3)
    pts = sc["means3D"] * 3.0 - 1.0
    dev = torch.device("cuda:0")
    r = GaussianRasterizer(GaussianRasterizationSettings(**syn.camera_settings_kwargs(cam, 1, True, device=dev)))
    got = r.markVisible(pts.to(dev)).cpu()
    assert got.dtype == torch.bool and torch.equal(got, oracle_b.mark_visible(pts, kw["viewmatrix"], kw["projmatrix"]))


def test_debug_mode_and_prefiltered_trap():
    sc, cam, kw, dC, dF = util.scene_case(P=800, F=3, W=32, H=32)
    util.run_hip(sc, cam, dC, dF, 1, True, (0, 0, 0), debug=True)  # stage-by-stage sync path
    dev = torch.device("cuda:0")
    k = syn.camera_settings_kwargs(cam, 1, True, device=dev)
    k["prefiltered"] = True
    fwd = cam["world_view_transform"].reshape(-1)[[2, 6, 10]]
    sc["means3D"][0] = cam["camera_center"] - 3.0 * fwd  # one culled point although prefiltered is claimed
    d = {n: v.to(dev) for n, v in sc.items()}
    with pytest.raises(RuntimeError, match="prefiltered"):
        GaussianRasterizer(GaussianRasterizationSettings(**k))(
            d["means3D"], torch.zeros_like(d["means3D"]), d["opacities"], shs=d["shs"],
            language_feature_precomp=d["language_feature"], scales=d["scales"], rotations=d["rotations"])


def test_render_wrapper_matches_direct_call():
    """manigaussian_amd.gaussian_renderer.render == MG/gaussian_renderer/__init__.py:render semantics."""
    from manigaussian_amd.gaussian_renderer import render
    dev = torch.device("cuda:0")
    sc, cam, kw, dC, dF = util.scene_case(P=3000, F=3)
    raw_feat = torch.randn(3000, 3, generator=torch.Generator().manual_seed(5))
    data = {"novel_view": {"FovX": [cam["FovX"]], "FovY": [cam["FovY"]], "width": [128], "height": [128],
                           "world_view_transform": cam["world_view_transform"][None].to(dev),
                           "full_proj_transform": cam["full_proj_transform"][None].to(dev),
                           "camera_center": cam["camera_center"][None].to(dev)}}
    d = {k: v.to(dev) for k, v in sc.items()}
    out = render(data, 0, d["means3D"], d["rotations"], d["scales"], d["opacities"], [0.1, 0.2, 0.3],
                 features_color=d["shs"], features_language=raw_feat.to(dev))
    sc["language_feature"] = raw_feat / (raw_feat.norm(dim=-1, keepdim=True) + 1e-12)
    cr, fr, rr, _, st = util.run_oracle_b(sc, kw, dC, dF)
    assert util.image_errors(out["render"].cpu(), cr, st)[0] <= IMG_TOL
    assert util.image_errors(out["render_embed"].cpu(), fr, st)[0] <= IMG_TOL
    assert torch.equal(out["radii"].cpu(), rr) and out["viewspace_points"].shape == (3000, 3)
    # no language features: zeros [N,3] placeholder, include_feature False -> [1] output
    out = render(data, 0, d["means3D"], d["rotations"], d["scales"], d["opacities"], [0.1, 0.2, 0.3],
                 pts_rgb=torch.rand(3000, 3, device=dev))
    assert out["render_embed"].shape == (1,)


# ---- full BASELINE sizes: properties that need no oracle run -------------------------------------------

def _full(P=100000, F=32, W=128, H=128, cam_index=1, bg=(0.0, 0.0, 0.0)):
    dev = torch.device("cuda:0")
    sc = syn.make_scene(P, F=F, M=4, seed=0)
    cam = syn.circle_cameras(4, W, H, negative_focal=True)[cam_index]
    st = GaussianRasterizationSettings(**syn.camera_settings_kwargs(cam, 1, True, bg=bg, device=dev))
    return {k: v.to(dev) for k, v in sc.items()}, GaussianRasterizer(st), cam


def _fwd_bwd(d, rast, dC, dF):
    leaves = {k: v.clone().requires_grad_(True) for k, v in d.items()}
    c, f, r = rast(leaves["means3D"], torch.zeros_like(leaves["means3D"]), leaves["opacities"], shs=leaves["shs"],
                   language_feature_precomp=leaves["language_feature"], scales=leaves["scales"],
                   rotations=leaves["rotations"])
    torch.autograd.backward([c, f], [dC, dF])
    return c.detach(), f.detach(), r, {k: v.grad for k, v in leaves.items()}


@pytest.mark.parametrize("P,W", [(100000, 128), (500000, 256)], ids=["C3_100k_128", "C5_500k_256"])
def test_full_size_properties(P, W):
    """(1) backward is linear in the cotangent; (2) forward is bit-deterministic; (3) a Gaussian permutation
    permutes radii and gradients and leaves the image unchanged up to equal-depth ties; (4) 0 <= image."""
    d, rast, cam = _full(P=P, W=W, H=W)
    dev = d["means3D"].device
    g = torch.Generator().manual_seed(7)
    dC1, dF1 = torch.randn(3, W, W, generator=g).to(dev), torch.randn(32, W, W, generator=g).to(dev)
    dC2, dF2 = torch.randn(3, W, W, generator=g).to(dev), torch.randn(32, W, W, generator=g).to(dev)
    c1, f1, r1, g1 = _fwd_bwd(d, rast, dC1, dF1)
    c2, f2, r2, g2 = _fwd_bwd(d, rast, dC2, dF2)
    assert torch.equal(c1, c2) and torch.equal(f1, f2) and torch.equal(r1, r2)
    assert c1.min() >= 0 and torch.isfinite(c1).all() and torch.isfinite(f1).all()
    _, _, _, g12 = _fwd_bwd(d, rast, 2.0 * dC1 - 3.0 * dC2, 2.0 * dF1 - 3.0 * dF2)
    for k in g1:
        ref = 2.0 * g1[k] - 3.0 * g2[k]
        scale = max(g1[k].abs().max().item(), g2[k].abs().max().item())
        assert (g12[k] - ref).abs().max().item() <= 2e-4 * scale, k
        assert torch.isfinite(g12[k]).all()
    perm = torch.randperm(P, generator=g).to(dev)
    dp = {k: v[perm].contiguous() for k, v in d.items()}
    cp, fp, rp, gp = _fwd_bwd(dp, rast, dC1, dF1)
    assert torch.equal(rp, r1[perm])
    assert (cp - c1).abs().max().item() <= IMG_TOL and (fp - f1).abs().max().item() <= IMG_TOL
    for k in g1:
        assert (gp[k] - g1[k][perm]).abs().max().item() <= GRAD_TOL * g1[k].abs().max().item(), k


def test_tight_bins_is_result_preserving_at_full_size():
    """Dropping the (Gaussian, tile) instances whose alpha >= 1/255 footprint misses the tile removes only pairs
    that every pixel of the tile skips: the same pairs are blended in the same order.  The chunk boundaries move with
    the list, so the partial sums are grouped differently and equality holds to float rounding."""
    d, rast, cam = _full()
    dev = d["means3D"].device
    g = torch.Generator().manual_seed(9)
    dC, dF = torch.randn(3, 128, 128, generator=g).to(dev), torch.randn(32, 128, 128, generator=g).to(dev)
    try:
        _lib.set_option("tight_bins", 0)
        c0, f0, r0, g0 = _fwd_bwd(d, rast, dC, dF)
        _lib.set_option("tight_bins", 1)
        c1, f1, r1, g1 = _fwd_bwd(d, rast, dC, dF)
    finally:
        _lib.set_option("tight_bins", 1)
    assert torch.equal(r0, r1)
    # regrouped products differ in the last bits; a pixel sitting on the T < 1e-4 stop rule may then keep or drop
    # ONE more Gaussian (weight <= alpha * 1e-4): bulk at rounding level, outliers bounded by that weight
    for x0, x1 in ((c0, c1), (f0, f1)):
        e = (x0 - x1).abs().flatten()
        assert torch.quantile(e[:: max(1, e.numel() // 1000000)], 0.999).item() <= 2e-6 and e.max().item() <= 1e-4
    for k in g0:
        assert (g0[k] - g1[k]).abs().max().item() <= 2e-5 * g0[k].abs().max().item() + 1e-9, k


def test_sharded_views_on_gpu_equal_sum_of_views():
    """render_sharded() with the HIP rasterizer, world=1: bucket == sum over views of per-view gradients."""
    from manigaussian_amd.parallel import GradBucket, render_sharded
    dev = torch.device("cuda:0")
    P, W, F, V = 20000, 128, 32, 4
    sc = syn.make_scene(P, F=F, M=4, seed=0)
    cams = syn.circle_cameras(V, W, W, negative_focal=True)
    items = []
    for v, cam in enumerate(cams):
        dC, dF = syn.make_cotangents(W, W, F, seed=20 + v)
        items.append((GaussianRasterizer(GaussianRasterizationSettings(
            **syn.camera_settings_kwargs(cam, 1, True, device=dev))), dC.to(dev), dF.to(dev)))

    def render_item(params, item):
        rast, dC, dF = item
        c, f, _ = rast(params["means3D"], torch.zeros_like(params["means3D"]), params["opacities"], shs=params["shs"],
                       language_feature_precomp=params["language_feature"], scales=params["scales"],
                       rotations=params["rotations"])
        return (c * dC).sum() + (f * dF).sum()

    params = {k: v.to(dev).requires_grad_(True) for k, v in sc.items()}
    bucket = GradBucket(params)
    render_sharded(params, items, render_item, bucket)
    total = {k: p.grad.clone() for k, p in params.items()}
    acc = {k: torch.zeros_like(v) for k, v in total.items()}
    for it in items:
        gs = torch.autograd.grad(render_item(params, it), list(params.values()))
        for k, g_ in zip(params, gs):
            acc[k] += g_
    for k in total:
        assert (total[k] - acc[k]).abs().max().item() <= 1e-4 * acc[k].abs().max().item() + 1e-9, k


# ---- multi-view batches ---------------------------------------------------------------

@pytest.mark.parametrize("case", [dict(P=6000, F=32, V=4, W=128, H=128), dict(P=3000, F=3, V=3, W=72, H=40),
                                  dict(P=2000, F=5, V=2, W=64, H=64, precomp=True),
                                  dict(P=20000, F=32, V=8, W=128, H=128),
                                  dict(P=3000, F=3, V=3, W=72, H=40, bin_mode=0),
                                  dict(P=2500, F=8, V=5, W=512, H=512)],
                         ids=["f32_4views", "odd_size_3views", "precomp_colors_padded_f5", "f32_8views",
                              "binning_tables_in_memory", "5120_tiles_batch_in_memory_vs_single_views_in_lds"])
def test_view_batch_equals_per_view_calls(case):
    """GaussianRasterizerBatch == V GaussianRasterizer calls: images and radii bit for bit (same kernels, same
    per-pixel arithmetic and order), per-view means2D gradients equal, parameter gradients = sum over the views.
    The last two cases take the bin scatter with its tables in memory (forced by bin_mode 0; 5 x 1024 tiles exceed the LDS
    tables while each single view fits them: both scatter forms must yield the same lists)."""
    from manigaussian_amd import GaussianRasterizerBatch
    if "bin_mode" in case:
        _lib.set_option("bin_mode", case["bin_mode"])
    try:
        _view_batch_equals_per_view_calls(case)
    finally:
        _lib.set_option("bin_mode", _DEFAULTS["bin_mode"])


def test_view_batch_randomised_sweep_fixed_seed():
    """24 cases of tests/tools/fuzz_views.py (random Gaussian counts, view counts, image sizes, feature widths)."""
    import random
    rng = random.Random(11)
    for _ in range(24):
        case = dict(P=int(10 ** rng.uniform(0.0, 4.8)), F=rng.choice([3, 3, 8, 32]), V=rng.choice([2, 3, 4, 5, 8]),
                    precomp=rng.random() < 0.2)
        case["W"], case["H"] = rng.choice([(8, 8), (17, 33), (32, 32), (40, 72), (64, 64), (100, 52), (128, 128), (200, 120)])
        _view_batch_equals_per_view_calls(case)


def _view_batch_equals_per_view_calls(case):
    from manigaussian_amd import GaussianRasterizerBatch
    dev = torch.device("cuda:0")
    P, F, V, W, H = case["P"], case["F"], case["V"], case["W"], case["H"]
    precomp = case.get("precomp", False)
    sc = syn.make_scene(P, F=F, M=4, seed=2, colors_precomp=precomp)
    cams = syn.circle_cameras(V, W, H, negative_focal=True)
    sets = [GaussianRasterizationSettings(**syn.camera_settings_kwargs(c, 1, True, bg=(0.1, 0.2, 0.3), device=dev))
            for c in cams]
    g = torch.Generator().manual_seed(4)
    dC, dF = torch.randn(V, 3, H, W, generator=g).to(dev), torch.randn(V, F, H, W, generator=g).to(dev)

    def leaves():
        return {k: v.to(dev).clone().requires_grad_(True) for k, v in sc.items()}

    def call(rast, d, m2d):
        kw = dict(colors_precomp=d["colors_precomp"]) if precomp else dict(shs=d["shs"])
        return rast(d["means3D"], m2d, d["opacities"], language_feature_precomp=d["language_feature"],
                    scales=d["scales"], rotations=d["rotations"], **kw)

    db = leaves()
    m2b = torch.zeros(V, P, 3, device=dev, requires_grad=True)
    cb, fb, rb = call(GaussianRasterizerBatch(sets), db, m2b)
    torch.autograd.backward([cb, fb], [dC, dF])
    ds = leaves()
    acc = None
    for v in range(V):
        m2 = torch.zeros(P, 3, device=dev, requires_grad=True)
        c, f, r = call(GaussianRasterizer(sets[v]), ds, m2)
        assert torch.equal(c, cb[v]) and torch.equal(f, fb[v]) and torch.equal(r, rb[v]), f"view {v}"
        torch.autograd.backward([c, f], [dC[v], dF[v]])
        assert (m2.grad - m2b.grad[v]).abs().max().item() <= 1e-5 * m2.grad.abs().max().item() + 1e-9
    for k in ds:
        ref, got = ds[k].grad, db[k].grad
        assert (got - ref).abs().max().item() <= 2e-5 * ref.abs().max().item() + 1e-9, k


class _GuardedTorch:
    """Stand-in for the `torch` module inside manigaussian_amd.views / ._C: every uint8 workspace gets a 64 KB guard band
    behind the size the library asked for; check() fails if a kernel wrote into one."""
    GUARD = 64 << 10

    def __init__(self):
        self.bases = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, size, *a, **kw):
        if kw.get("dtype") is torch.uint8:
            n = int(size[0]) if isinstance(size, (tuple, list)) else int(size)
            base = torch.empty((n + self.GUARD,), *a, **kw)
            base[n:] = 0xA5
            self.bases.append((base, n))
            return base[:n]
        return torch.empty(size, *a, **kw)

    def check(self):
        torch.cuda.synchronize()
        assert self.bases
        for base, n in self.bases:
            assert bool((base[n:] == 0xA5).all()), f"a kernel wrote past a {n}-byte workspace"


@pytest.mark.parametrize("P,V,W", [(1100, 4, 128), (1025, 16, 128), (20000, 8, 128), (2049, 3, 64), (1100, 5, 512)])
def test_view_batch_workspaces_are_not_overrun(P, V, W, monkeypatch):
    """Gaussian counts that are not a multiple of the preprocess workgroup (1024) with V > 1: the per-(workgroup, tile) table
    has one row per LAUNCHED workgroup, V * ceil(P / 1024), not ceil(V * P / 1024) (round-2 advisor finding: 2-60 KB were
    written past the geometry workspace).  Guard bands behind every workspace must stay intact, forward and backward."""
    from manigaussian_amd import views as views_mod, _C as C_mod
    gt = _GuardedTorch()
    monkeypatch.setattr(views_mod, "torch", gt)
    monkeypatch.setattr(C_mod, "torch", gt)
    monkeypatch.setattr(C_mod, "_SPLIT_WORKSPACES", True)  # three allocations instead of one arena: a guard band behind each
    F = 32
    sc, cams, dC, dF = _batch_case(P, F, V, W, W)
    cb, fb, rb, grads, m2g = _run_batch(sc, cams, dC, dF, (0.1, 0.2, 0.3))
    gt.check()
    n_ws = len(gt.bases)
    assert n_ws >= 3
    # ... and the single-view path on the same scene (its workspaces are guarded the same way; through the ctypes shim, whose
    # allocations this test can intercept -- the compiled binding carves the same three workspaces out of one arena)
    with C_mod.use_compiled(False):
        ch, fh, rh, gh = util.run_hip(sc, cams[0], dC[0], dF[0], 1, True, (0.1, 0.2, 0.3))
    gt.check()
    assert len(gt.bases) >= n_ws + 3
    assert torch.equal(ch, cb[0]) and torch.equal(rh, rb[0])


class _RefusingTorch:
    """Stand-in for the `torch` module inside manigaussian_amd._C whose allocator refuses uint8 requests of ONE size (the
    worst-case workspace of the shape under test) with OutOfMemoryError: a Python exception, nothing reaches the device."""

    def __init__(self, nbytes):
        self.nbytes, self.refused = nbytes, 0

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, size, *a, **kw):
        n = int(size[0]) if isinstance(size, (tuple, list)) else int(size)
        if kw.get("dtype") is torch.uint8 and n == self.nbytes:
            self.refused += 1
            raise torch.cuda.OutOfMemoryError("refused by the test")
        return torch.empty(size, *a, **kw)


@pytest.mark.parametrize("V", [0, 3], ids=["single_view", "3_views"])
def test_worst_case_workspace_the_allocator_refuses_falls_back_to_the_marks(V, monkeypatch):
    """A forward whose worst-case workspace the allocator refuses goes by the marks and waits for its preprocess, for a single
    view (ctypes shim) and a view batch alike: no warning, no error, the images and radii of a blocking-mode run bit for bit
    and its gradients to float-atomic order."""
    from manigaussian_amd import _C, _state
    dev = torch.device("cuda:0")
    P, F, W, n = 3000, 32, 64, max(V, 1)
    sc, cams, dC, dF = _batch_case(P, F, n, W, W)
    bg = (0.1, 0.2, 0.3)

    def run():
        if V:
            c, f, r, g, m2g = _run_batch(sc, cams, dC, dF, bg)
            return c, f, r, dict(g, means2D=m2g)
        with _C.use_compiled(False):
            return util.run_hip(sc, cams[0], dC[0], dF[0], 1, True, bg)

    gb, ib, ok, cap, pool, _ = _lib.plan_arena(P, 4, F, W, W, V, _state.safe_bytes(dev))
    assert ok, "the shape's worst case must fit the budget"
    refusing = _RefusingTorch(gb + ib + _lib.plan_binning_bytes(P, F, W, W, V, cap, pool, False))
    old_mode = _state.set_forward_mode("blocking")
    try:
        ref = run()
        _state.set_forward_mode("safe")
        monkeypatch.setattr(_C, "torch", refusing)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            got = run()
            _state.check_status(dev)
    finally:
        _state.set_forward_mode(old_mode)
    assert refusing.refused >= 1, "the forward did not ask for its worst-case workspace"
    (c0, f0, r0, g0), (c1, f1, r1, g1) = ref, got
    assert torch.equal(c1, c0) and torch.equal(f1, f0) and torch.equal(r1, r0)
    assert g1.keys() == g0.keys()
    for k in g0:
        assert (g1[k] - g0[k]).abs().max().item() <= 2e-5 * g0[k].abs().max().item() + 1e-12, k


def _batch_case(P, F, V, W, H, seed=2, precomp=False):
    sc = syn.make_scene(P, F=F, M=4, seed=seed, colors_precomp=precomp)
    cams = syn.circle_cameras(max(V, 4), W, H, negative_focal=True)[:V]
    g = torch.Generator().manual_seed(4)
    return sc, cams, torch.randn(V, 3, H, W, generator=g), torch.randn(V, F, H, W, generator=g)


def _run_batch(sc, cams, dC, dF, bg):
    from manigaussian_amd import GaussianRasterizerBatch
    dev = torch.device("cuda:0")
    V, P = len(cams), sc["means3D"].shape[0]
    sets = [GaussianRasterizationSettings(**syn.camera_settings_kwargs(c, 1, True, bg=bg, device=dev)) for c in cams]
    d = {k: v.to(dev).clone().requires_grad_(True) for k, v in sc.items()}
    m2 = torch.zeros(V, P, 3, device=dev, requires_grad=True)
    kw = dict(colors_precomp=d["colors_precomp"]) if "colors_precomp" in d else dict(shs=d["shs"])
    cb, fb, rb = GaussianRasterizerBatch(sets)(d["means3D"], m2, d["opacities"], scales=d["scales"],
                                               language_feature_precomp=d["language_feature"], rotations=d["rotations"],
                                               **kw)
    torch.autograd.backward([cb, fb], [dC.to(dev), dF.to(dev)])
    torch.cuda.synchronize()
    grads = {k: v.grad.cpu() for k, v in d.items()}
    return cb.detach().cpu(), fb.detach().cpu(), rb.cpu(), grads, m2.grad.cpu()


@pytest.mark.parametrize("case", [dict(P=20000, F=32, V=4, W=128, H=128), dict(P=100000, F=32, V=8, W=128, H=128),
                                  dict(P=16384, F=3, V=8, W=128, H=128), dict(P=16384, F=3, V=4, W=128, H=128)],
                         ids=["f32_4views_20k", "c3_f32_8views_100k", "manigaussian_f3_8views", "manigaussian_f3_4views"])
def test_view_batch_matches_reference_kernels(case):
    """GaussianRasterizerBatch (V views in one call) against V runs of the REFERENCE's own kernels (oracle/_ref, live on
    this GPU): every view's image <= 2e-5, radii bit-exact, per-view means2D gradients and the parameter gradients summed
    over the views <= 1e-3 of the tensor max.  (The comparison with per-view HIP calls below cannot see a
    wrong-but-consistent change in the shared kernels; this one can.)"""
    from oracle import ref_cuda
    if not ref_cuda.available(case["F"]):
        pytest.skip("oracle/_ref/libmgs_ref*.so not built (needs /root/reference at build time)")
    P, F, V, W, H = case["P"], case["F"], case["V"], case["W"], case["H"]
    bg = (0.1, 0.2, 0.3)
    sc, cams, dC, dF = _batch_case(P, F, V, W, H)
    cb, fb, rb, gb, m2b = _run_batch(sc, cams, dC, dF, bg)
    from oracle import oracle_b
    acc, fragile = None, torch.zeros(P, dtype=torch.bool)
    for v, cam in enumerate(cams):
        kw = syn.camera_settings_kwargs(cam, 1, True, bg=bg)
        cr, fr, rr, gr, _ = util.run_reference(sc, kw, dC[v], dF[v])
        state = util.run_oracle_b(sc, kw, dC[v], dF[v])[4]  # which pixels / Gaussians sit on a hard threshold in this view
        fpx, fg = oracle_b.fragile_mask(state), oracle_b.fragile_gaussians(state)
        fragile |= fg
        assert np.array_equal(rb[v].numpy(), rr.numpy()), f"radii, view {v}"
        for nm, a, b in (("color", cb[v], cr), ("feature", fb[v], fr)):
            e = (a - b).abs().max(0)[0]
            assert e[~fpx].max().item() <= 2e-5 and e.max().item() <= util.REF_FRAGILE_TOL, f"{nm}, view {v}"
            assert int((e > IMG_TOL).sum()) <= util.REF_MAX_PIXELS_ABOVE_CONTRACT, f"{nm}, view {v}"
        r2 = gr["means2D"]
        e2 = (m2b[v] - r2).abs().max(1)[0]
        assert e2[~fg].max().item() <= GRAD_TOL * r2.abs().max().item() + 1e-9, f"means2D, view {v}"
        assert e2.max().item() <= util.REF_FRAGILE_GRAD_TOL * r2.abs().max().item() + 1e-9, f"means2D, view {v}"
        acc = {k: t.clone() for k, t in gr.items()} if acc is None else {k: acc[k] + gr[k] for k in acc}
    for k, got in gb.items():
        ref = acc[util.GRAD_KEYS[k]].reshape(got.shape)
        d = (got - ref).abs().reshape(P, -1).max(1)[0]
        mag = ref.abs().max().item()
        assert d[~fragile].max().item() <= GRAD_TOL * mag + 1e-9, k
        assert d.max().item() <= util.REF_FRAGILE_GRAD_TOL * mag + 1e-9, k


@pytest.mark.parametrize("case", [dict(P=6000, F=32, V=4, W=128, H=128), dict(P=3000, F=3, V=3, W=72, H=40),
                                  dict(P=2000, F=8, V=2, W=64, H=64, precomp=True)],
                         ids=["f32_4views", "odd_size_3views", "precomp_colors_f8"])
def test_view_batch_matches_oracle_b(case):
    """The same against Oracle B (CPU restatement, runs without the reference build): robust pixels 1e-4, gradients summed
    over the views 1e-3 of the max away from threshold-fragile Gaussians."""
    P, F, V, W, H = case["P"], case["F"], case["V"], case["W"], case["H"]
    bg = (0.1, 0.2, 0.3)
    sc, cams, dC, dF = _batch_case(P, F, V, W, H, precomp=case.get("precomp", False))
    cb, fb, rb, gb, m2b = _run_batch(sc, cams, dC, dF, bg)
    from oracle import oracle_b
    acc, fragile = None, torch.zeros(P, dtype=torch.bool)
    for v, cam in enumerate(cams):
        kw = syn.camera_settings_kwargs(cam, 1, True, bg=bg)
        cr, fr, rr, gr, st = util.run_oracle_b(sc, kw, dC[v], dF[v])
        assert torch.equal(rb[v], rr), f"radii, view {v}"
        for a, b in ((cb[v], cr), (fb[v], fr)):
            robust, frag, frac = util.image_errors(a, b, st)
            assert robust <= IMG_TOL and frag <= util.FRAGILE_TOL and frac <= util.FRAGILE_MAX_FRACTION, f"view {v}"
        fragile |= oracle_b.fragile_gaussians(st)
        acc = {k: t.clone() for k, t in gr.items()} if acc is None else {k: acc[k] + gr[k] for k in acc}
    assert fragile.float().mean().item() <= 0.1
    for k, got in gb.items():
        ref = acc[util.GRAD_KEYS[k]].reshape(got.shape)
        d = (got - ref).abs().reshape(P, -1).max(1)[0]
        mag = ref.abs().max().item()
        assert d[~fragile].max().item() <= GRAD_TOL * mag + 1e-7, k
        assert d.max().item() <= util.FRAGILE_GRAD_TOL * mag + 1e-7, k


# ---- deformation-field kernels ---------------------------------------------------------------------

def test_deform_apply_and_assembly_match_torch():
    from manigaussian_amd.deform import DeformationField, assemble_deform_input, deform_apply
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    N = 16384
    rn = lambda *s: torch.randn(*s, generator=g).to(dev)
    lat, z = rn(N, 128).requires_grad_(True), rn(N, 39).requires_grad_(True)
    xyz, sh, rot, scale, op, feat, act = rn(N, 3), rn(N, 4, 3), rn(N, 4), rn(N, 3), rn(N, 1), rn(N, 3), rn(1, 8)
    for use_feat in (False, True):
        out = assemble_deform_input(lat, z, xyz, sh, rot, scale, op, feat if use_feat else None, act)
        parts = [lat, xyz, sh[:, 0], sh[:, 1:].reshape(N, 9), rot, scale, op] + ([feat] if use_feat else []) + \
                [z, act.repeat(N, 1)]                      # models_embed.py:258-287
        ref = torch.cat(parts, -1)
        assert out.shape == ref.shape == (N, 128 + (73 if use_feat else 70)) and torch.equal(out, ref)
        w = rn(*out.shape)
        g1 = torch.autograd.grad((out * w).sum(), [lat, z])
        g2 = torch.autograd.grad((ref * w).sum(), [lat, z])
        assert torch.equal(g1[0], g2[0]) and torch.equal(g1[1], g2[1])
    delta = rn(N, 7).requires_grad_(True)
    nx, nr = deform_apply(delta, xyz, rot)
    rx, rr = xyz + delta[:, :3], torch.nn.functional.normalize(rot + delta[:, 3:], dim=-1)  # models_embed.py:297-299
    assert torch.allclose(nx, rx, atol=1e-6) and torch.allclose(nr, rr, atol=1e-6)
    wx, wr = rn(N, 3), rn(N, 4)
    ga = torch.autograd.grad((nx * wx).sum() + (nr * wr).sum(), delta)[0]
    gb = torch.autograd.grad((rx * wx).sum() + (rr * wr).sum(), delta)[0]
    assert torch.allclose(ga, gb, atol=1e-5, rtol=1e-4)
    field = DeformationField().to(dev)
    nxt = field(lat, z, xyz, sh, rot, scale, op, action=act)
    assert nxt["xyz"].shape == (N, 3) and nxt["rot"].shape == (N, 4)
    assert torch.allclose(nxt["rot"].norm(dim=-1), torch.ones(N, device=dev), atol=1e-5)
    (nxt["xyz"].sum() + nxt["rot"].sum()).backward()
    assert lat.grad is not None and torch.isfinite(lat.grad).all()


def test_regressor_epilogue_matches_torch():
    """manigaussian_amd.regressor.gaussian_epilogue vs the reference's torch ops (models_embed.py:233-253,
    gaussian_renderer/__init__.py:66-68), forward and backward, including clamped scales and a zero feature row."""
    from manigaussian_amd.regressor import gaussian_epilogue
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    N = 16384
    raw0 = torch.randn(1, N, 26, generator=g)
    raw0[..., 4:7] = raw0[..., 4:7] * 1.5 - 3.5     # exp() on both sides of the 0.05 clamp
    raw0[0, 5, 14:17] = 0.0                          # zero feature vector
    xyz0 = torch.randn(1, N, 3, generator=g)
    raw = raw0.to(dev).requires_grad_(True)
    xyz_in = xyz0.to(dev).requires_grad_(True)
    out = gaussian_epilogue(raw, xyz_in)
    raw_r = raw0.to(dev).requires_grad_(True)
    xyz_r = xyz0.to(dev).requires_grad_(True)
    dxyz, op, sc, rt, fdc, feat, frest = raw_r.split([3, 1, 3, 4, 3, 3, 9], dim=-1)
    ref = dict(xyz=xyz_r + dxyz, opacity=torch.sigmoid(op), scale=torch.clamp_max(torch.exp(sc), 0.05),
               rot=torch.nn.functional.normalize(rt, dim=-1),
               sh=torch.cat([fdc.unsqueeze(2), frest.reshape(1, N, -1, 3)], dim=2), feature=feat,
               feature_normalized=feat / (feat.norm(dim=-1, keepdim=True) + 1e-12))
    ws = {}
    for k in ref:
        assert out[k].shape == ref[k].shape, k
        assert torch.allclose(out[k], ref[k], atol=1e-6, rtol=1e-5), k
        ws[k] = torch.randn(ref[k].shape, generator=g).to(dev)
    (sum((out[k] * ws[k]).sum() for k in ref)).backward()
    (sum((ref[k] * ws[k]).sum() for k in ref)).backward()
    assert torch.allclose(raw.grad, raw_r.grad, atol=1e-5, rtol=1e-4)
    assert torch.allclose(xyz_in.grad, xyz_r.grad)
    # only some outputs used: the unused ones arrive as None
    raw.grad = None
    gaussian_epilogue(raw, xyz_in)["scale"].sum().backward()
    assert raw.grad[..., :4].abs().max() == 0 and raw.grad[..., 7:].abs().max() == 0


def test_point_latent_pe_matches_grid_sample_and_positional_encoding():
    """manigaussian_amd.voxel.point_latent_pe vs the reference's torch ops (models_embed.py:147-215, utils.py:133-169):
    grid_sample(align_corners=True) incl. points outside the volume, the 39-wide positional code, and the gradient
    w.r.t. the voxel features."""
    import math
    from manigaussian_amd.voxel import point_latent_pe
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    C, G, N = 128, 20, 16384
    bounds = (-0.3, -0.5, 0.6, 0.7, 0.5, 1.6)
    vox0 = torch.randn(1, C, G, G + 1, G + 2, generator=g)
    lo, hi = torch.tensor(bounds[:3]), torch.tensor(bounds[3:])
    xyz0 = lo + (hi - lo) * (torch.rand(1, N, 3, generator=g) * 1.3 - 0.15)   # some points outside the box
    vox = vox0.to(dev).requires_grad_(True)
    out = point_latent_pe(vox, xyz0.to(dev), bounds)
    # reference ops
    vr = vox0.to(dev).requires_grad_(True)
    canon = (xyz0.to(dev) - lo.to(dev)) / (hi.to(dev) - lo.to(dev))
    grid = (canon * 2 - 1.0).unsqueeze(1).unsqueeze(1)
    pl = torch.nn.functional.grid_sample(vr, grid, align_corners=True, mode="bilinear").squeeze(2).squeeze(2).permute(0, 2, 1)
    x = canon.reshape(-1, 3)
    freqs = torch.repeat_interleave(math.pi * 2.0 ** torch.arange(0, 6), 2).view(1, -1, 1).to(dev)
    phases = torch.zeros(12, device=dev)
    phases[1::2] = math.pi * 0.5
    emb = torch.sin(torch.addcmul(phases.view(1, -1, 1), x.unsqueeze(1).repeat(1, 12, 1), freqs)).view(N, -1)
    ref = torch.cat((pl.reshape(-1, C), torch.cat((x, emb), dim=-1)), dim=-1)
    assert out.shape == ref.shape == (N, C + 39)
    assert torch.allclose(out[:, :C], ref[:, :C], atol=1e-5, rtol=1e-5)
    assert torch.allclose(out[:, C:C + 3], ref[:, C:C + 3], atol=1e-6)
    assert (out[:, C + 3:] - ref[:, C + 3:]).abs().max().item() <= 2e-5   # sin of arguments up to 32 pi
    w = torch.randn(ref.shape, generator=g).to(dev)
    (out * w).sum().backward()
    (ref * w).sum().backward()
    assert torch.allclose(vox.grad, vr.grad, atol=1e-4, rtol=1e-4)
