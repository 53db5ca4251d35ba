"""The compiled autograd binding (manigaussian_amd/csrc/mgs_torch.cpp -> _mgs_torch.so): what the reference's own binding is
(RAST/rasterize_points.cu:35-225, compiled, torch types in, rasterizer out), over this repository's C ABI.  CPU: it loads, it
shares the workspace marks with the ctypes shim, it declines what it does not handle.  GPU: it is the path an unmodified
caller takes, its results are those of the ctypes shim (same kernels: images bit for bit, gradients to float-atomic order),
its waiting / retry / overflow protocol, autograd corner cases."""
import gc
import os
import time
import warnings

import pytest
import torch

import manigaussian_amd as mg
from manigaussian_amd import GaussianRasterizationSettings, GaussianRasterizer, _C, _lib, _state
from manigaussian_amd import synthetic as syn

import util


def _ext():
    e = _C.compiled()
    assert e is not None, "manigaussian_amd/_mgs_torch.so is not built (make -C manigaussian_amd/csrc ext)"
    return e


def test_compiled_binding_loads_declines_cpu_calls_and_shares_the_marks():
    e = _ext()
    assert e.ABI_VERSION == _lib.ABI_VERSION and e.build_id() == _lib.build_id()
    t = torch.zeros(4, 3)
    before = e.counters()["declined"]
    assert e.rasterize(t, t, t, t, t, t, t, t, t, t, t, t, t, 8, 8, 1.0, 1.0, 1.0, 1, False, False, True) is None
    assert e.counters()["declined"] == before + 1
    m = _state._Marks(7)  # (device index 7: nothing else uses it; the one store of the library's ledger)
    key, vkey = (1000, 64, 64, 3, 1), ("views", 4, 1000, 64, 64, 3, 1)
    assert key not in m and m.get(key) is None
    m[key] = [10000, None]
    m[vkey] = [5, 6]
    assert m[key] == [10000, None] and m[vkey] == [5, 6] and set(m) == {key, vkey} and len(m) == 2
    st = _state.DeviceState.__new__(_state.DeviceState)
    st.marks = m
    assert st.guess(key) is None             # chunk pool unknown: no guess
    st.learn(key, R=8000, chunks=400)        # marks only grow
    assert m[key] == [10000, 400] and st.guess(key) == (int(10000 * 1.5) + 4096, int(400 * 2.0) + 64)
    del m[key], m[vkey]
    assert len(m) == 0


def _step(d, rast, dC, dF, between=None, retain=False):
    leaves = {k: v.detach().requires_grad_(True) for k, v in d.items()}
    m2 = torch.zeros_like(leaves["means3D"]).requires_grad_(True)
    c, f, r = rast(leaves["means3D"], m2, leaves["opacities"], shs=leaves["shs"],
                   language_feature_precomp=leaves["language_feature"], scales=leaves["scales"], rotations=leaves["rotations"])
    if between is not None:
        between()
    inputs = list(leaves.values()) + [m2]
    grads = torch.autograd.grad([c, f], inputs, [dC, dF], retain_graph=retain)
    return c, f, r, grads, (leaves, m2, inputs)


def _setup(P, F, W=128):
    dev = torch.device("cuda:0")
    sc, cam, kw, dC, dF = util.scene_case(P=P, F=F, W=W, H=W)
    d = {k: v.to(dev) for k, v in sc.items()}
    rast = GaussianRasterizer(GaussianRasterizationSettings(**syn.camera_settings_kwargs(cam, 1, True, bg=(0.1, 0.2, 0.3),
                                                                                        device=dev)))
    return dev, d, rast, dC.to(dev), dF.to(dev)


def _same(a, b):
    (c0, f0, r0, g0), (c1, f1, r1, g1) = a[:4], b[:4]
    assert torch.equal(c1, c0) and torch.equal(f1, f0) and torch.equal(r1, r0)
    for x, y in zip(g1, g0):
        assert x.shape == y.shape
        assert (x - y).abs().max().item() <= 2e-5 * y.abs().max().item() + 1e-12  # float atomics: order differs run to run


@pytest.mark.gpu
@pytest.mark.parametrize("mode,budget_mb", [("safe", None), ("safe", 0), ("async", 0)],
                         ids=["safe-cannot-overflow", "safe-waits-for-the-preprocess", "async-marks"])
def test_compiled_path_is_what_runs_and_equals_the_ctypes_shim(mode, budget_mb):
    e = _ext()
    dev, d, rast, dC, dF = _setup(20000, 32)
    old_mode, old_budget = mg.set_forward_mode(mode), _state._SAFE_BYTES
    if budget_mb is not None:
        mg.set_safe_workspace(budget_mb)
    try:
        with _C.use_compiled(False):
            for _ in range(3):
                ref = _step(d, rast, dC, dF)
                mg.check_status(dev)
        e.counters(True)
        for _ in range(3):
            got = _step(d, rast, dC, dF)
            mg.check_status(dev)
        n = e.counters()
        assert n["forwards"] == 3 and n["backwards"] == 3 and n["declined"] == 0, n
        assert n["waited"] == (3 if (mode == "safe" and budget_mb == 0) else 0), n
        assert got[0].grad_fn.name() == "MgsRasterizeBackward" and got[2].grad_fn is None
        _same(ref, got)
    finally:
        mg.set_forward_mode(old_mode)
        _state.set_safe_bytes(old_budget)


@pytest.mark.gpu
def test_compiled_wait_path_retries_when_the_scene_outgrew_its_marks_and_never_returns_incomplete_images():
    e = _ext()
    dev, d, rast, dC, dF = _setup(15000, 3)
    old_mode, old_budget = mg.set_forward_mode("safe"), _state._SAFE_BYTES
    mg.set_safe_workspace(0)
    try:
        with _C.use_compiled(False), util_forward_mode("blocking"):
            ref = _step(d, rast, dC, dF)
        st = _state.device_state(dev)
        key = (15000, 128, 128, 3, 1)
        mg.check_status(dev)
        good = st.marks[key][0]
        st.marks[key] = [16, None]   # far too small: the preprocess's report says so, the call bins + renders again
        e.counters(True)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            got = _step(d, rast, dC, dF)
            mg.check_status(dev)
        n = e.counters()
        assert n["forwards"] == 1 and n["waited"] == 1 and n["retried"] == 1, n
        _same(ref, got)
        assert st.marks[key][0] >= good  # learnt again: the BINNED count
        got2 = _step(d, rast, dC, dF)
        mg.check_status(dev)
        assert e.counters()["retried"] == 1
        _same(ref, got2)
    finally:
        mg.set_forward_mode(old_mode)
        _state.set_safe_bytes(old_budget)


import contextlib


@contextlib.contextmanager
def util_forward_mode(mode):
    old = mg.set_forward_mode(mode)
    try:
        yield
    finally:
        mg.set_forward_mode(old)


@pytest.mark.gpu
def test_compiled_autograd_corner_cases():
    """retain_graph (a second backward allocates and fills its accumulators), no_grad, a saved input modified in place,
    an unused output, and no leak: the node holds its images weakly."""
    e = _ext()
    dev, d, rast, dC, dF = _setup(6000, 32)
    with _C.use_compiled(False):
        ref = _step(d, rast, dC, dF)
    e.counters(True)
    c, f, r, g1, (leaves, m2, inputs) = _step(d, rast, dC, dF, retain=True)
    g2 = torch.autograd.grad([c, f], inputs, [dC, dF])
    _same(ref, (c, f, r, g1))
    _same(ref, (c, f, r, g2))
    with pytest.raises(RuntimeError, match="second time"):
        torch.autograd.grad([c, f], inputs, [dC, dF])
    # only the colour image is differentiated: the feature cotangent is absent
    c, f, r, _, (leaves, m2, inputs) = _step(d, rast, dC, dF, retain=True)
    gc_only = torch.autograd.grad([c], inputs, [dC], allow_unused=True)
    with _C.use_compiled(False):
        c_, f_, r_, _, (lv_, m2_, in_) = _step(d, rast, dC, dF, retain=True)
        gc_ref = torch.autograd.grad([c_], in_, [dC], allow_unused=True)
    for x, y in zip(gc_only, gc_ref):
        assert (x is None) == (y is None)
        if x is not None:
            assert (x - y).abs().max().item() <= 2e-5 * y.abs().max().item() + 1e-12
    with torch.no_grad():
        c, f, r = rast(d["means3D"], torch.zeros_like(d["means3D"]), d["opacities"], shs=d["shs"],
                       language_feature_precomp=d["language_feature"], scales=d["scales"], rotations=d["rotations"])
    assert c.grad_fn is None and not c.requires_grad and torch.equal(c, ref[0])
    # a saved input modified in place between forward and backward: autograd's own error
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in d.items()}
    sc_ = leaves["scales"] * 1.0  # (non-leaf, so that an in-place op is legal)
    c, f, r = rast(leaves["means3D"], torch.zeros_like(leaves["means3D"]), leaves["opacities"], shs=leaves["shs"],
                   language_feature_precomp=leaves["language_feature"], scales=sc_, rotations=leaves["rotations"])
    assert c.grad_fn.name() == "MgsRasterizeBackward"
    sc_.mul_(2.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        (c.sum() + f.sum()).backward()
    del c, f, r
    mg.check_status(dev)
    gc.collect()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(dev)
    for _ in range(40):
        _step(d, rast, dC, dF)
    mg.check_status(dev)
    gc.collect()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(dev) - base < (8 << 20), "a forward's workspaces are not being released"


@pytest.mark.gpu
def test_num_rendered_is_the_reference_integer_on_every_path():
    """blocking entry points returned the reference's 3-sigma-rect count, asynchronous handles the binned count.
    The device now reports both (status words 0 and 2): int(handle) is the reference's integer on every path, binned() the
    other one."""
    dev, d, rast, dC, dF = _setup(20000, 32)
    e_ = torch.Tensor([])
    s = rast.raster_settings
    R_block = _C.rasterize_gaussians(s.bg, d["means3D"], e_, d["language_feature"], d["opacities"], d["scales"], d["rotations"],
                                     1.0, e_, s.viewmatrix, s.projmatrix, s.tanfovx, s.tanfovy, 128, 128, d["shs"], 1,
                                     s.campos, False, False, True)[0]
    old = mg.set_forward_mode("async")
    try:
        with _C.use_compiled(False):
            for _ in range(3):
                c, f, r, g, _ = _step(d, rast, dC, dF, retain=True)
                mg.check_status(dev)
            h = c.grad_fn.num_rendered
            assert h.pending is not None and int(h) == R_block and 0 < h.binned() <= R_block
    finally:
        mg.set_forward_mode(old)


@pytest.mark.gpu
def test_tile_tables_zeroed_by_a_launch_of_their_own_and_a_delayed_table_workgroup():
    """VERDICT r4 item 8.  table_init = 1: a zero-fill launch ahead of the preprocess, no workgroup waits for another (what
    debug = 1 selects by itself).  dbg = 512: workgroup 0 of the default preprocess sleeps ~0.3 ms before it zeroes the tables --
    every working workgroup has long finished its Gaussians and waits; bins, images and gradients must be the default's, bit
    for bit (images) -- and no MGS_ERR_HIP."""
    dev, d, rast, dC, dF = _setup(30000, 32)
    ref = _step(d, rast, dC, dF)
    mg.check_status(dev)
    for key, val in (("table_init", 1), ("dbg", 512)):
        old = _lib.get_option(key)
        _lib.set_option(key, val)
        try:
            for compiled in (True, False):
                with _C.use_compiled(compiled):
                    got = _step(d, rast, dC, dF)
                    mg.check_status(dev)
                    _same(ref, got)
            with _C.use_compiled(False), util_forward_mode("blocking"):
                got = _step(d, rast, dC, dF)
                _same(ref, got)
        finally:
            _lib.set_option(key, old)


@pytest.mark.gpu
def test_hand_shake_that_gives_up_is_retried_by_a_waiting_forward_and_repaired_behind_a_lazy_one():
    """the preprocess launch's table hand-shake assumes that workgroup 0 makes progress.  dbg = 1024 makes it never
    publish: the workers give up after ~1 s and nothing is binned.  A forward that waits for the preprocess runs itself again
    with the tables zeroed by a launch of their own (inside the call); a LAZY forward (the default `safe` mode with its
    worst-case workspace, or `async`) cannot -- its report says MGS_RETRY_TABLE_INIT, its backward re-renders on the same
    workspace with table_init = 1 and warns, and without a backward the next drain raises with that message (round 5: a generic
    "rasterizer forward failed")."""
    e = _ext()
    dev, d, rast, dC, dF = _setup(20000, 32)
    ref = _step(d, rast, dC, dF)
    mg.check_status(dev)
    old_dbg, old_budget = _lib.get_option("dbg"), _state._SAFE_BYTES
    _lib.set_option("dbg", 1024)
    try:
        for compiled in (True, False):
            with _C.use_compiled(compiled):
                # lazy: the images are repaired at backward entry (the report has arrived: the synchronise in between)
                with warnings.catch_warnings(record=True) as w:
                    warnings.simplefilter("always")
                    got = _step(d, rast, dC, dF, between=torch.cuda.synchronize)
                    mg.check_status(dev)
                assert any("zeroed tile tables" in str(x.message) for x in w), [str(x.message) for x in w]
                _same(ref, got)
                # lazy, no backward: loud at the next drain, with the reason
                with torch.no_grad():
                    rast(d["means3D"], torch.zeros_like(d["means3D"]), d["opacities"], shs=d["shs"],
                         language_feature_precomp=d["language_feature"], scales=d["scales"], rotations=d["rotations"])
                with pytest.raises(RuntimeError, match="zeroed tile tables"):
                    mg.check_status(dev)
                # waiting for the preprocess (no worst-case workspace): the call repairs itself
                mg.set_safe_workspace(0)
                with warnings.catch_warnings():
                    warnings.simplefilter("error")
                    got = _step(d, rast, dC, dF)
                    mg.check_status(dev)
                _same(ref, got)
                _state.set_safe_bytes(old_budget)
    finally:
        _lib.set_option("dbg", old_dbg)
        _state.set_safe_bytes(old_budget)
    assert e.counters()["recovered"] >= 1


@pytest.mark.gpu
def test_hand_shake_that_gives_up_is_retried_by_a_waiting_view_batch():
    """The same give-up (dbg = 1024) for GaussianRasterizerBatch (mgs_rasterize_forward_views): without a worst-case workspace
    the batch waits for its preprocess and runs itself again with the tables zeroed by a launch of their own, inside the call
    -- no warning, no error (round 6: "rasterize views: the forward preprocess gave up waiting for its zeroed tile tables").
    Images and radii are the default run's bit for bit, gradients equal to float-atomic order."""
    from manigaussian_amd import GaussianRasterizerBatch
    dev = torch.device("cuda:0")
    P, F, V, W = 20000, 32, 3, 64
    sc = syn.make_scene(P, F=F, M=4, seed=2)
    cams = syn.circle_cameras(4, W, W, negative_focal=True)[:V]
    rast = GaussianRasterizerBatch([GaussianRasterizationSettings(**syn.camera_settings_kwargs(c, 1, True, bg=(0.1, 0.2, 0.3),
                                                                                             device=dev)) for c in cams])
    g = torch.Generator().manual_seed(4)
    dC, dF = torch.randn(V, 3, W, W, generator=g).to(dev), torch.randn(V, F, W, W, generator=g).to(dev)

    def step():
        d = {k: v.to(dev).clone().requires_grad_(True) for k, v in sc.items()}
        c, f, r = rast(d["means3D"], None, d["opacities"], shs=d["shs"], language_feature_precomp=d["language_feature"],
                       scales=d["scales"], rotations=d["rotations"])
        return c, f, r, torch.autograd.grad([c, f], list(d.values()), [dC, dF])

    ref = step()
    mg.check_status(dev)
    old_dbg, old_budget = _lib.get_option("dbg"), _state._SAFE_BYTES
    try:
        _lib.set_option("dbg", 1024)
        mg.set_safe_workspace(0)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            got = step()
            mg.check_status(dev)
        _same(ref, got)
    finally:
        _lib.set_option("dbg", old_dbg)
        _state.set_safe_bytes(old_budget)


@pytest.mark.gpu
def test_two_python_threads_render_on_one_device_while_a_third_reads_the_status():
    """VERDICT r5 item 4a / ADVICE r5 (medium): drain() held the device's mutex while it released and re-took the GIL around
    hipDeviceSynchronize(); a second Python thread on the same device (GIL -> mutex) then dead-locked with it.  Two threads run
    1 000 forward + backward steps each through the compiled binding on ONE device while a third calls check_status(wait=True /
    False) in a loop; everybody finishes, and every thread's last step equals the single-threaded one."""
    import threading
    _ext()
    dev, d, rast, dC, dF = _setup(16384, 3)
    ref = _step(d, rast, dC, dF)
    mg.check_status(dev)
    errors, done = [], threading.Event()

    def worker(n):
        try:
            torch.cuda.set_device(dev)
            got = None
            for i in range(n):
                got = _step(d, rast, dC, dF)
                if i % 97 == 0:
                    mg.check_status(dev, wait=True)
            torch.cuda.synchronize()
            _same(ref, got)
        except Exception as ex:  # noqa: BLE001
            errors.append(ex)

    def checker():
        try:
            i = 0
            while not done.is_set():
                mg.check_status(dev, wait=(i % 2 == 0))
                i += 1
                time.sleep(2e-4)  # (a reader that spins takes the GIL from the renderers: the test then lasts minutes)
        except Exception as ex:  # noqa: BLE001
            errors.append(ex)

    ts = [threading.Thread(target=worker, args=(1000,), daemon=True) for _ in range(2)]
    tc = threading.Thread(target=checker, daemon=True)
    for t in ts + [tc]:
        t.start()
    for t in ts:
        t.join(timeout=300)
    done.set()
    tc.join(timeout=60)
    assert not any(t.is_alive() for t in ts + [tc]), "dead-lock: a thread did not finish"
    assert not errors, errors
    mg.check_status(dev)


@pytest.mark.gpu
@pytest.mark.parametrize("compiled", [True, False], ids=["compiled", "ctypes"])
def test_safe_budget_is_charged_against_the_workspaces_live_forwards_hold(compiled):
    """VERDICT r5 item 4b / ADVICE r5: `safe` mode gives a shape its WORST-CASE workspace (4.0 GB at BASELINE configs[2]) so that a
    forward never waits and never overflows -- but the budget was tested per call, so 16 forwards before the first backward
    pinned 64 GB.  The budget is now charged against what live forwards still hold: the first forwards that fit take the worst
    case, the rest size their workspace from the marks and wait for the preprocess's report (still never incomplete).  The
    reference sizes every buffer from the count (RAST/rasterize_points.cu:27-33,84-89)."""
    e = _ext()
    dev, d, rast, dC, dF = _setup(100000, 32)
    budget = _state.safe_bytes(dev)
    with _C.use_compiled(compiled):
        ref = _step(d, rast, dC, dF)  # (the shape's marks: the forwards that do not get the worst case size from them)
        mg.check_status(dev)
        ref = None
        ref = _step(d, rast, dC, dF)[:4]
        gc.collect()
        torch.cuda.synchronize()
        assert _state.held_bytes(dev.index) == 0
        e.counters(True)
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        outs = []
        for _ in range(16):
            leaves = {k: v.detach().requires_grad_(True) for k, v in d.items()}
            m2 = torch.zeros_like(leaves["means3D"]).requires_grad_(True)
            c, f, r = rast(leaves["means3D"], m2, leaves["opacities"], shs=leaves["shs"],
                           language_feature_precomp=leaves["language_feature"], scales=leaves["scales"],
                           rotations=leaves["rotations"])
            outs.append((c, f, list(leaves.values()) + [m2]))
            assert _state.held_bytes(dev.index) <= budget
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated(dev) - base
        held = _state.held_bytes(dev.index)
        assert 0 < held <= budget, (held, budget)
        assert peak <= 2 * budget, f"16 forwards in flight hold {peak / 2**30:.1f} GB, budget {budget / 2**30:.1f} GB"
        if compiled:
            n = e.counters()
            assert n["forwards"] == 16 and n["budget_fallbacks"] >= 8 and n["waited"] == n["budget_fallbacks"], n
        for c, f, inputs in outs:  # every forward is complete, every backward runs on its own state
            assert torch.equal(c, ref[0]) and torch.equal(f, ref[1])
            g = torch.autograd.grad([c, f], inputs, [dC, dF])
            for x, y in zip(g, ref[3]):
                assert (x - y).abs().max().item() <= 2e-5 * y.abs().max().item() + 1e-12
        mg.check_status(dev)
        del outs, c, f, inputs, g, leaves, m2, r
        gc.collect()
        torch.cuda.synchronize()
        assert _state.held_bytes(dev.index) == 0


@pytest.mark.gpu
def test_both_bindings_ask_one_ledger():
    """The marks and the outstanding reports are the library's (csrc/mgs_ledger.hip), not a binding's: a shape the ctypes shim
    warmed up is known to the compiled binding -- its FIRST forward of the shape is lazy --, and an overflow behind the compiled
    path is reported by the shim's check_status()."""
    e = _ext()
    dev, d, rast, dC, dF = _setup(2000, 3, W=64)
    key = (2000, 64, 64, 3, 1)
    old_mode, old_budget = mg.set_forward_mode("async"), _state._SAFE_BYTES
    mg.set_safe_workspace(0)
    try:
        mg.check_status(dev)
        st = _state.device_state(dev)
        st.marks.pop(key, None)  # (whoever warms the shape below is the shim)
        with _C.use_compiled(False):
            for _ in range(3):
                ref = _step(d, rast, dC, dF)
                mg.check_status(dev)
        good = list(st.marks[key])
        assert good[0] > 0 and good[1] is not None
        e.counters(True)
        got = _step(d, rast, dC, dF)
        n = e.counters()
        assert n["forwards"] == 1 and n["backwards"] == 1 and n["declined"] == 0 and n["waited"] == 0, n
        mg.check_status(dev)
        _same(ref, got)
        # too few chunk records (the shape bins fewer instances than the 4096 every guess adds: an instance mark cannot be too low)
        st.marks[key] = [good[0], 1]
        assert st.guess(key)[1] < good[1]
        with torch.no_grad():          # (no backward will follow: nobody can repair it)
            rast(d["means3D"], torch.zeros_like(d["means3D"]), d["opacities"], shs=d["shs"],
                 language_feature_precomp=d["language_feature"], scales=d["scales"], rotations=d["rotations"])
        assert e.counters()["forwards"] == 2 and e.counters()["declined"] == 0
        with pytest.raises(RuntimeError, match="outgrew the workspace"):
            _state.check_status(dev)
        assert st.marks[key][0] >= good[0]
        _same(ref, _step(d, rast, dC, dF))
        mg.check_status(dev)
    finally:
        mg.set_forward_mode(old_mode)
        _state.set_safe_bytes(old_budget)


@pytest.mark.gpu
@pytest.mark.parametrize("compiled", [True, False], ids=["compiled", "ctypes"])
@pytest.mark.parametrize("mode,budget_mb", [("safe", None), ("async", 0)], ids=["safe-worst-case-workspace", "async-mark-sized-workspace"])
def test_default_paths_bin_without_a_scatter_launch(compiled, mode, budget_mb):
    """Direct binning (csrc/mgs_common.h): on the package-default path (a worst-case workspace: its key arrays have the room) and on
    the mark-sized workspaces of the asynchronous mode (the bindings add mgs_binning_direct_extra bytes) the forward preprocess
    writes the tile keys itself -- the stage profile counts no bin scatter launch; with MgsOptions.dbg & 32768 it counts one per
    forward, and the results are the same bits either way."""
    dev, d, rast, dC, dF = _setup(16384, 3)
    old_mode, old_budget, old_dbg = mg.set_forward_mode(mode), _state._SAFE_BYTES, _lib.get_option("dbg")
    if budget_mb is not None:
        mg.set_safe_workspace(budget_mb)
    try:
        with _C.use_compiled(compiled):
            out = {}
            for dbg in (0, 32768):
                _lib.set_option("dbg", dbg)
                for _ in range(3):  # (asynchronous mode: the first calls of a shape learn its marks on the waiting path)
                    _step(d, rast, dC, dF)
                    mg.check_status(dev)
                torch.cuda.synchronize()
                _lib.profile_read(reset=True)
                _lib.set_option("profile", 2)
                out[dbg] = _step(d, rast, dC, dF)
                torch.cuda.synchronize()
                _lib.set_option("profile", 0)
                prof = _lib.profile_read(reset=True)
                mg.check_status(dev)
                assert prof["preprocess_fwd"][1] == 1 and prof["bin_segsort"][1] == 1, prof
                assert prof["bin_scatter"][1] == (1 if dbg else 0), (dbg, prof)
            _same(out[0], out[32768])
    finally:
        _lib.set_option("profile", 0)
        _lib.set_option("dbg", old_dbg)
        mg.set_forward_mode(old_mode)
        _state.set_safe_bytes(old_budget)
