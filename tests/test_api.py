"""CPU tests of the drop-in boundary: the C-ABI library loads and exports every symbol include/mgsplat.h
declares, the Python surface matches the reference's (field order, signatures, exception messages), and the
product path refuses to run without a HIP device instead of falling back."""
import inspect
import os

import pytest
import torch

import conv_family
from manigaussian_amd import _C, _lib
import diff_gaussian_rasterization as dgr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    L = _lib.lib()  # binds every symbol in _lib._EXPORTS; raises if one is missing
    conv_family.check_abi()   # the names, and every entry point's argument count and size type, against include/mgsplat.h
    assert L.mgs_abi_version() == _lib.ABI_VERSION


def test_workspace_size_queries_and_options():
    L = _lib.lib()
    assert L.mgs_geom_bytes(1000, 4, 128, 128) > 1000 * 75
    assert L.mgs_geom_bytes(2000, 4, 128, 128) > L.mgs_geom_bytes(1000, 4, 128, 128)
    assert L.mgs_img_bytes(128, 128) >= 128 * 128 * 4
    assert L.mgs_binning_bytes2(5000, 64, 128, 128, 32) < L.mgs_binning_bytes(5000, 128, 128, 32)
    assert L.mgs_chunk_pool_max(5000, 128, 128) == 4 * ((5000 + 63) // 64 + 16 * 64)
    assert L.mgs_binning_bytes(5000, 128, 128, 32) > 5000 * 24
    assert L.mgs_binning_bytes(0, 128, 128, 0) > 0
    old = _lib.get_option("tight_bins")
    _lib.set_option("tight_bins", 1 - old)
    assert _lib.get_option("tight_bins") == 1 - old
    _lib.set_option("tight_bins", old)
    with pytest.raises(RuntimeError):
        _lib.set_option("no_such_option", 1)


def test_settings_fields_match_reference_order():
    # RAST/diff_gaussian_rasterization/__init__.py:166-179
    assert dgr.GaussianRasterizationSettings._fields == (
        "image_height", "image_width", "tanfovx", "tanfovy", "bg", "scale_modifier", "viewmatrix", "projmatrix",
        "sh_degree", "campos", "prefiltered", "debug", "include_feature")


def test_forward_signature_matches_reference():
    sig = inspect.signature(dgr.GaussianRasterizer.forward)
    assert list(sig.parameters) == ["self", "means3D", "means2D", "opacities", "shs", "colors_precomp",
                                    "language_feature_precomp", "scales", "rotations", "cov3D_precomp"]
    assert all(sig.parameters[p].default is None for p in list(sig.parameters)[4:])
    assert list(inspect.signature(_C.rasterize_gaussians).parameters) == [
        "background", "means3D", "colors", "language_feature", "opacity", "scales", "rotations", "scale_modifier",
        "cov3D_precomp", "viewmatrix", "projmatrix", "tan_fovx", "tan_fovy", "image_height", "image_width", "sh",
        "degree", "campos", "prefiltered", "debug", "include_feature"]  # RAST/rasterize_points.h:18-40
    assert len(inspect.signature(_C.rasterize_gaussians_backward).parameters) == 24  # rasterize_points.h:42-67


def _settings():
    z = torch.zeros
    return dgr.GaussianRasterizationSettings(32, 32, 0.5, 0.5, z(3), 1.0, torch.eye(4), torch.eye(4), 1, z(3), False,
                                             False, True)


def test_argument_exclusivity_messages():
    r = dgr.GaussianRasterizer(_settings())
    m, o = torch.zeros(4, 3), torch.zeros(4, 1)
    with pytest.raises(Exception, match="Please provide excatly one of either SHs or precomputed colors!"):
        r(m, m, o, scales=m, rotations=torch.zeros(4, 4))
    with pytest.raises(Exception, match="Please provide excatly one of either SHs or precomputed colors!"):
        r(m, m, o, shs=torch.zeros(4, 4, 3), colors_precomp=m, scales=m, rotations=torch.zeros(4, 4))
    msg = "Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!"
    with pytest.raises(Exception, match=msg):
        r(m, m, o, colors_precomp=m)
    with pytest.raises(Exception, match=msg):
        r(m, m, o, colors_precomp=m, scales=m)
    with pytest.raises(Exception, match=msg):
        r(m, m, o, colors_precomp=m, scales=m, rotations=torch.zeros(4, 4), cov3D_precomp=torch.zeros(4, 6))


def test_no_cpu_fallback_and_shape_check():
    r = dgr.GaussianRasterizer(_settings())
    m, o = torch.zeros(4, 3), torch.zeros(4, 1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        r(m, m, o, colors_precomp=m, scales=m, rotations=torch.zeros(4, 4))
    with pytest.raises(RuntimeError, match=r"means3D must have dimensions \(num_points, 3\)"):
        r(torch.zeros(4, 2), m, o, colors_precomp=m, scales=m, rotations=torch.zeros(4, 4))
    with pytest.raises(RuntimeError, match="no CPU path"):
        r.markVisible(m)


def test_product_path_does_not_import_the_oracle():
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r); import manigaussian_amd, diff_gaussian_rasterization; "
            "import manigaussian_amd.deform, manigaussian_amd.parallel, manigaussian_amd.gaussian_renderer; "
            "bad = [m for m in sys.modules if m == 'oracle' or m.startswith('oracle.')]; "
            "assert not bad, bad" % ROOT)
    subprocess.check_call([sys.executable, "-c", code])
    for root, _, files in os.walk(os.path.join(ROOT, "manigaussian_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                assert "oracle" not in open(os.path.join(root, f)).read().replace("the CPU oracle", ""), f


def test_feature_width_padding_table():
    assert [_C._padded_F(f) for f in (1, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64)] == [3, 3, 4, 8, 8, 16, 16, 32, 32, 64, 64]
    with pytest.raises(RuntimeError):
        _C._padded_F(65)


@pytest.mark.skipif(not os.path.isdir("/root/reference"), reason="reference tree not present on this box")
def test_reference_render_file_imports_against_this_module():
    """The unmodified call site agents/manigaussian_bc/gaussian_renderer/__init__.py resolves
    `from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer` here."""
    import importlib.util
    path = "/root/reference/agents/manigaussian_bc/gaussian_renderer/__init__.py"
    spec = importlib.util.spec_from_file_location("ref_gaussian_renderer", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.GaussianRasterizer is dgr.GaussianRasterizer
    assert list(inspect.signature(mod.render).parameters)[:7] == ["data", "idx", "pts_xyz", "rotations", "scales",
                                                                  "opacity", "bg_color"]


def test_async_workspace_guess_follows_the_marks_and_the_headroom():
    """Host logic of the asynchronous forward (no device): the workspace guess of a shape is its high-water marks times the
    configurable head-room; marks only grow; an unknown chunk pool means "no guess" (the blocking path is taken)."""
    from manigaussian_amd import _state
    import manigaussian_amd as mg
    st = _state.DeviceState.__new__(_state.DeviceState)  # no pinned memory needed for the marks
    st.marks = _state._Marks(9)  # (the ledger's marks of a device index nothing else uses)
    st.marks.clear()
    key = (1000, 64, 64, 3, 1)
    assert st.guess(key) is None
    st.learn(key, R=10000, chunks=None, pool_unknown=True)
    assert st.guess(key) is None
    st.learn(key, R=8000, chunks=400)
    assert st.marks[key] == [10000, 400]
    hi, hc = _state._HEADROOM["instances"], _state._HEADROOM["chunks"]
    assert (hi, hc) == (1.5, 2.0)  # the defaults (memory is cheap on a 288 GB part; an overflow costs a step)
    assert st.guess(key) == (int(10000 * hi) + 4096, int(400 * hc) + 64)
    mg.set_headroom(instances=2.0, chunks=3.0)
    try:
        assert st.guess(key) == (2 * 10000 + 4096, 3 * 400 + 64)
        with pytest.raises(ValueError):
            mg.set_headroom(instances=0.5)
    finally:
        mg.set_headroom(instances=hi, chunks=hc)


def test_split_k_weight_gradient_equals_the_plain_product():
    """deform._wgrad: the batched split-K form of g^T @ x used by the fused MLP backward (CPU tensors, float64)."""
    import torch
    from manigaussian_amd import deform
    g, x = torch.randn(4096, 24, dtype=torch.float64), torch.randn(4096, 40, dtype=torch.float64)
    old = deform._WGRAD_MIN_ROWS
    try:
        deform._WGRAD_MIN_ROWS = 64
        assert torch.allclose(deform._wgrad(g, x), g.t() @ x, rtol=1e-12, atol=1e-12)
        deform._WGRAD_MIN_ROWS = 10 ** 9
        assert torch.equal(deform._wgrad(g, x), g.t() @ x)
    finally:
        deform._WGRAD_MIN_ROWS = old


def test_forward_mode_and_overflow_policy_switches_validate_their_argument():
    """Host-side switches (no GPU): set_* return the previous value and reject unknown values."""
    import manigaussian_amd as mg
    old = mg.set_forward_mode("blocking")
    try:
        assert mg.forward_mode() == "blocking" and mg.set_forward_mode("async") == "blocking"
        with pytest.raises(ValueError):
            mg.set_forward_mode("lazy")
    finally:
        mg.set_forward_mode(old)
    oldp = mg.set_overflow_policy("raise")
    try:
        assert mg.overflow_policy() == "raise" and mg.set_overflow_policy("repair") == "raise"
        with pytest.raises(ValueError):
            mg.set_overflow_policy("ignore")
    finally:
        mg.set_overflow_policy(oldp)


def test_feature_tables_beyond_32_bit_offsets_are_refused_before_any_launch():
    """The render forward addresses feature rows by 32-bit byte offsets (buffer loads): P * F * 4 >= 4 GiB is an argument error,
    reported by the argument check that runs before the first HIP call (so this runs without a GPU; the pointers below are
    never dereferenced)."""
    import ctypes
    a = _lib.MgsRasterArgs()
    a.P, a.D, a.M, a.F, a.W, a.H = 40_000_000, 1, 4, 32, 128, 128
    a.tanfovx = a.tanfovy = 0.5
    a.scale_modifier = 1.0
    a.include_feature = 1
    fake = ctypes.c_void_p(0x10000)
    for n in ("background", "means3D", "shs", "language_feature", "opacities", "scales", "rotations", "viewmatrix",
              "projmatrix", "campos"):
        setattr(a, n, fake)
    nr = ctypes.c_int32(-7)
    L = _lib.lib()
    L.mgs_rasterize_forward_preprocess.restype = ctypes.c_int
    rc = L.mgs_rasterize_forward_preprocess(ctypes.byref(a), None, ctypes.byref(nr), None)
    assert rc == -1, rc  # MGS_ERR_INVALID_ARG
    assert "32-bit offsets" in _lib.last_error()
    a.P = 1000  # the same arguments at a legal size pass the argument check (and would go on to the device): not called here
