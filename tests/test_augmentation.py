"""The fused SE(3) augmentation (manigaussian_amd/augmentation.py, csrc/mgs_augment.hip) against ManiGaussian's
voxel/augmentation.py.

Truth: the reference itself, executed on the CPU with the draws of a table (tests/se3_cases.py says how and with which
stand-ins), committed as tests/golden/se3/*.npz by tests/golden/make_golden_se3.py.  The GPU box has no reference: there the
fixtures are the truth.  With a fixture's draws injected the actions and the chosen attempt must be EXACTLY the fixture's --
the generator kept only cases whose every discretisation decision is at least 1e-4 bins from its boundary, far more than the
fp32 rounding by which the kernel (and the real pytorch3d) differ from the float64 stand-in -- and every cloud and camera pose
within 2e-5 absolute.

The 2e-5: for coordinates |p| <= 4 the reference's fp32 chain -- a subtract, a three-term dot product and an add -- rounds by at
most about 4e-6 whatever the order of its sums and whether or not they are fused; rotation entries that differ by one ulp
(6e-8) from the stand-in's, times three terms of at most 4 + 4, add about 1.5e-6.  The tolerance is 4 x the sum.
"""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from child import run_graph_tool
import se3_cases as sc

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [c[0] for c in sc.CASES]
TOL = 2e-5


def _spec(name):
    return next(c for c in sc.CASES if c[0] == name)


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
def test_every_case_has_its_fixture_and_the_fixtures_are_small():
    cases = sc.load_cases()
    assert sorted(cases) == sorted(NAMES)
    for name in NAMES:
        assert os.path.getsize(os.path.join(sc.GOLDEN, name + ".npz")) <= 64 * 1024, name
        c = cases[name]
        assert float(c["margin"]) >= sc.MARGIN, name
        n = int(c["n_cams"])
        assert max(float(np.abs(c[f"{k}{i}"]).max()) for k in ("pcd", "pose", "exp_pcd", "exp_pose") for i in range(n)) <= 4.0, name
    attempts = {name: int(cases[name]["exp_attempt"]) for name in NAMES}
    assert 0 in attempts.values() and -1 in attempts.values() and max(attempts.values()) >= 2, attempts
    assert {cases[n]["gripper"].shape[0] for n in NAMES} == {1, 3, 8}


@pytest.mark.skipif(not sc.have_reference(), reason="no copy of the reference on this machine")
@pytest.mark.parametrize("name", NAMES)
def test_fixtures_match_the_reference(name):
    """The generator's computation, re-run: the committed files are what the reference gives today."""
    c = sc.load_cases()[name]
    live = sc.build_case(_spec(name), int(c["seed"]))
    assert sorted(live) == sorted(c)
    for k in live:
        assert np.array_equal(np.asarray(live[k]), c[k]), (name, k)


def test_workspace_bytes():
    from manigaussian_amd import _lib, augmentation
    L = _lib.lib()
    assert L.mgs_se3_workspace_bytes(0) == 0 and L.mgs_se3_workspace_bytes(_lib.SE3_MAX_BATCH + 1) == 0
    assert L.mgs_se3_workspace_bytes(1) >= 64 and L.mgs_se3_workspace_bytes(_lib.SE3_MAX_BATCH) >= 64 * _lib.SE3_MAX_BATCH
    assert L.mgs_se3_workspace_bytes(8) % 256 == 0
    assert augmentation.workspace_bytes(8) == L.mgs_se3_workspace_bytes(8)
    assert L.mgs_abi_version() == 17  # additive exports


def test_the_library_refuses_bad_arguments_before_any_launch():
    """No device needed: the argument checks return before the first HIP call (the pointers are never dereferenced)."""
    from manigaussian_amd import _lib
    L = _lib.lib()
    fake = ctypes.c_void_p(0x10000)

    def args(**kw):
        a = _lib.MgsSe3Args()
        a.B, a.attempts, a.voxel_size, a.bounds_rows, a.rot_bins, a.rot_resolution = 2, 10, 100, 1, 72, 5.0
        for n in ("gripper_pose", "action_trans", "action_rot_grip", "bounds", "rng_state"):
            setattr(a, n, fake)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def select(a, ws_bytes=1 << 20):
        return L.mgs_se3_select(ctypes.byref(a), fake, fake, fake, fake, ws_bytes, None)

    for kw, word in ((dict(B=0), "B = 0"), (dict(B=_lib.SE3_MAX_BATCH + 1), "B = 4097"), (dict(attempts=0), "attempts = 0"),
                     (dict(attempts=_lib.SE3_MAX_ATTEMPTS + 1), "attempts = 33"), (dict(voxel_size=0), "voxel_size = 0"),
                     (dict(bounds_rows=3), "bounds_rows = 3"), (dict(retry=2), "retry = 2"), (dict(bounds=None), "NULL"),
                     (dict(rng_state=None), "rng_state")):
        assert select(args(**kw)) == _lib.MGS_ERR_INVALID_ARG, kw
        assert word in _lib.last_error(), (kw, _lib.last_error())
    a = args()
    a.rot_steps[1] = -1
    assert select(a) == _lib.MGS_ERR_INVALID_ARG and "rot_steps" in _lib.last_error()
    assert select(args(), ws_bytes=16) == _lib.MGS_ERR_WORKSPACE
    a = args(n_sources=_lib.SE3_MAX_SOURCES + 1)
    assert L.mgs_se3_apply(ctypes.byref(a), fake, 1 << 20, None) == _lib.MGS_ERR_INVALID_ARG and "9 sources" in _lib.last_error()
    a = args(n_sources=1)
    a.src[0], a.dst[0], a.n_points[0], a.stride_c[0] = 0x10000, 0x20000, 0, 16
    assert L.mgs_se3_apply(ctypes.byref(a), fake, 1 << 20, None) == _lib.MGS_ERR_INVALID_ARG and "0 points" in _lib.last_error()
    a.n_points[0], a.stride_c[0] = 16, 8
    assert L.mgs_se3_apply(ctypes.byref(a), fake, 1 << 20, None) == _lib.MGS_ERR_INVALID_ARG and "plane stride 8" in _lib.last_error()
    assert L.mgs_se3_draws(ctypes.byref(args()), None, None) == _lib.MGS_ERR_INVALID_ARG


def _cpu_call(B=2, cams=1, **kw):
    import manigaussian_amd as mg
    a = dict(pcd=[torch.zeros(B, 3, 2, 2) for _ in range(cams)], camera_pose=[torch.eye(4).repeat(B, 1, 1) for _ in range(cams)],
             action_gripper_pose=torch.tensor([[0.0, 0, 1, 0, 0, 0, 1]]).repeat(B, 1),
             action_trans=torch.zeros(B, 3, dtype=torch.int32), action_rot_grip=torch.zeros(B, 4, dtype=torch.int32),
             bounds=torch.tensor([sc.SCENE_BOUNDS]))
    a.update(kw)
    return mg.apply_se3_augmentation_with_camera_pose(
        a["pcd"], a["camera_pose"], a["action_gripper_pose"], a["action_trans"], a["action_rot_grip"], a["bounds"], 0,
        sc.trans_aug_tensor(0.125), [0.0, 0.0, 45.0], 5, 100, 5, "cpu")


def test_the_drop_in_refuses_what_it_cannot_run():
    from manigaussian_amd import augmentation
    with pytest.raises(RuntimeError, match="no CPU path"):
        _cpu_call()
    with pytest.raises(ValueError, match=r"\(3, 7\)"):
        _cpu_call(action_gripper_pose=torch.zeros(3, 7))
    with pytest.raises(ValueError, match="one batch size"):
        _cpu_call(pcd=[torch.zeros(2, 3, 2, 2), torch.zeros(3, 3, 2, 2)], camera_pose=[])
    with pytest.raises(ValueError, match="one batch size"):
        _cpu_call(action_trans=torch.zeros(2, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match="9 and 9"):
        _cpu_call(cams=9)
    with pytest.raises(ValueError, match="4097"):
        _cpu_call(B=augmentation.MAX_BATCH + 1, pcd=[torch.zeros(augmentation.MAX_BATCH + 1, 3, 1, 1)])
    with pytest.raises(ValueError, match="3 rows for a batch of 2"):
        _cpu_call(bounds=torch.tensor([sc.SCENE_BOUNDS] * 3))
    with pytest.raises(ValueError, match="retry"):
        augmentation.Se3Augmentation(0.125, [0, 0, 45], 5, 100, 5, retry="each")
    with pytest.raises(ValueError, match="attempts"):
        augmentation.Se3Augmentation(0.125, [0, 0, 45], 5, 100, 5, attempts=33)
    m = augmentation.Se3Augmentation(sc.trans_aug_tensor(0.125), [10.0, 15.0, 45.0], 5, 100, 5)
    assert m.rot_steps == (2, 3, 9) and m.trans_f64 and m.state_dict() == {} and m.rng_state.dtype == torch.int64
    assert list(m.parameters()) == []


def test_the_signatures_are_the_references():
    import inspect
    import manigaussian_amd as mg
    assert list(inspect.signature(mg.apply_se3_augmentation_with_camera_pose).parameters) == [
        "pcd", "camera_pose", "action_gripper_pose", "action_trans", "action_rot_grip", "bounds", "layer", "trans_aug_range",
        "rot_aug_range", "rot_aug_resolution", "voxel_size", "rot_resolution", "device"]  # voxel/augmentation.py:256-268
    assert list(inspect.signature(mg.apply_se3_augmentation).parameters) == [
        "pcd", "action_gripper_pose", "action_trans", "action_rot_grip", "bounds", "layer", "trans_aug_range", "rot_aug_range",
        "rot_aug_resolution", "voxel_size", "rot_resolution", "device"]  # voxel/augmentation.py:134-145
    assert list(inspect.signature(mg.Se3Augmentation.__init__).parameters)[1:] == [
        "trans_aug_range", "rot_aug_range", "rot_aug_resolution", "voxel_size", "rot_resolution", "layer", "attempts", "retry"]


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
def _module(c, retry="batch"):
    from manigaussian_amd import Se3Augmentation
    return Se3Augmentation(sc.trans_aug_tensor(float(c["trans_aug_range"])), [float(v) for v in c["rot_aug_range"]],
                           sc.ROT_AUG_RESOLUTION, sc.VOXEL_SIZE, sc.ROT_RESOLUTION, layer=int(c["layer"]), attempts=sc.ATTEMPTS,
                           retry=retry)


def _device_inputs(c, dev):
    n = int(c["n_cams"])
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    return dict(pcd=[t(c[f"pcd{i}"]) for i in range(n)], pose=[t(c[f"pose{i}"]) for i in range(n)], gripper=t(c["gripper"]),
                action_trans=t(c["action_trans"]), action_rot_grip=t(c["action_rot_grip"]), bounds=t(c["bounds"]),
                draws=t(c["draws"]))


def _call(m, d, draws=True, pcd=None):
    return m(pcd if pcd is not None else d["pcd"], d["pose"], d["gripper"], d["action_trans"], d["action_rot_grip"], d["bounds"],
             draws=d["draws"] if draws else None)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _check_fields(name, c, got, prefix, attempts):
    """actions exact, clouds and poses within TOL (identity samples: the inputs' bits); prints each figure before it asserts."""
    trans, rot, pcd, pose = got
    exp_t, exp_r = c["exp_trans" if prefix == "exp" else "s_trans"], c["exp_rot_grip" if prefix == "exp" else "s_rot_grip"]
    assert trans.dtype == torch.int64 and rot.dtype == torch.int64
    worst = 0.0
    for i in range(int(c["n_cams"])):
        for kind, g in (("pcd", pcd[i]), ("pose", pose[i])):
            e = torch.from_numpy(c[f"{prefix}_{kind}{i}"])
            assert g.shape == e.shape and g.dtype == torch.float32
            worst = max(worst, float((g.cpu() - e).abs().max()))
            for b in range(e.shape[0]):
                if attempts[b] < 0:
                    assert torch.equal(_bits(g[b]), _bits(torch.from_numpy(c[f"{kind}{i}"][b]))), (name, kind, i, b)
    print(f"{name} [{prefix}]: attempts {list(attempts)}, trans equal {np.array_equal(trans.cpu().numpy(), exp_t)}, rot equal "
          f"{np.array_equal(rot.cpu().numpy(), exp_r)}, worst cloud / pose error {worst:.3e}")
    assert np.array_equal(trans.cpu().numpy(), exp_t), (name, trans.cpu().numpy(), exp_t)
    assert np.array_equal(rot.cpu().numpy(), exp_r), (name, rot.cpu().numpy(), exp_r)
    assert worst <= TOL, (name, worst)


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_fixture_draws_give_the_fixture(name):
    dev = torch.device("cuda:0")
    c = sc.load_cases()[name]
    d = _device_inputs(c, dev)
    before = {k: ([t.clone() for t in v] if isinstance(v, list) else v.clone()) for k, v in d.items()}
    m = _module(c)
    got = _call(m, d)
    B = c["gripper"].shape[0]
    info = m.last_info.cpu().numpy()
    assert m.last_info.is_cuda and info.dtype == np.int32 and info.shape == (1 + B,)
    assert info[0] == int(c["exp_attempt"]) and (info[1:] == int(c["exp_attempt"])).all(), (name, info)
    _check_fields(name, c, got, "exp", info[1:])
    for k, v in d.items():  # inputs untouched
        for x, y in zip(v if isinstance(v, list) else [v], before[k] if isinstance(v, list) else [before[k]]):
            assert torch.equal(x, y), (name, k)
    assert all(g.data_ptr() != s.data_ptr() for g, s in zip(got[2] + got[3], d["pcd"] + d["pose"]))


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_per_sample_retry_is_the_single_sample_reference(name):
    dev = torch.device("cuda:0")
    c = sc.load_cases()[name]
    m = _module(c, retry="sample")
    got = _call(m, _device_inputs(c, dev))
    info = m.last_info.cpu().numpy()
    assert (info[1:] == c["s_attempt"]).all(), (name, info, c["s_attempt"])
    assert info[0] == int(c["exp_attempt"]), (name, info)  # the first attempt valid for the whole batch, as in "batch"
    _check_fields(name, c, got, "s", info[1:])


@gpu
@pytest.mark.parametrize("name", ["b3_5x7_c2", "b8_4x4_c3", "b3_4x4_c3_never"])
def test_strided_clouds_give_the_bits_of_their_contiguous_copies(name):
    dev = torch.device("cuda:0")
    c = sc.load_cases()[name]
    d = _device_inputs(c, dev)
    m = _module(c)
    base = _call(m, d)
    sliced, last = [], []
    for p in d["pcd"]:
        wide = torch.full((p.size(0) + 1, 8, p.size(2), p.size(3)), float("nan"), device=dev)
        wide[1:, 2:5] = p
        sliced.append(wide[1:, 2:5])
        last.append(p.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2))
    assert not sliced[0].is_contiguous() and (not last[0].is_contiguous() or last[0].size(0) == 1)
    for pcd in (sliced, last):
        got = _call(m, d, pcd=pcd)
        for g, e in zip(got[2] + got[3], base[2] + base[3]):
            assert g.is_contiguous() and torch.equal(_bits(g), _bits(e)), name
        assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1])


@gpu
def test_int64_actions_fp32_range_and_the_cloud_only_function():
    """The same values through the other input forms: int64 actions, the drop-in function without cameras (draws from the
    stream: only shapes, types and the untouched inputs are checked), and a float32 trans_aug_range (the fp32 chain) at
    trans_aug_range = 0, where both chains give the same translation."""
    import manigaussian_amd as mg
    dev = torch.device("cuda:0")
    c = sc.load_cases()["b3_4x4_c2_notrans"]
    d = _device_inputs(c, dev)
    base = _call(_module(c), d)
    d64 = dict(d, action_trans=d["action_trans"].long(), action_rot_grip=d["action_rot_grip"].long())
    m32 = mg.Se3Augmentation(torch.zeros(3), [0.0, 0.0, 45.0], 5, 100, 5)
    assert not m32.trans_f64
    for got in (_call(_module(c), d64), _call(m32, d)):
        assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1])
        assert all(torch.equal(_bits(g), _bits(e)) for g, e in zip(got[2] + got[3], base[2] + base[3]))
    t, r, pcd = mg.apply_se3_augmentation(d["pcd"], d["gripper"], d["action_trans"], d["action_rot_grip"], d["bounds"], 0,
                                          sc.trans_aug_tensor(0.125), [0.0, 0.0, 45.0], 5, 100, 5, dev)
    assert t.dtype == torch.int64 and t.shape == (3, 3) and r.shape == (3, 4) and len(pcd) == 2 and pcd[0].shape == d["pcd"][0].shape
    assert int(t.min()) >= 0 and int(t.max()) < 100 and int(r[:, :3].min()) >= 0 and int(r[:, :3].max()) < 72
    assert torch.equal(r[:, 3].cpu(), torch.from_numpy(c["action_rot_grip"][:, 3]).long())


@gpu
def test_the_generator():
    from manigaussian_amd.augmentation import se3_draws
    dev = torch.device("cuda:0")
    A, B = 32, 128  # 4096 draws
    state = torch.tensor([2024, 5], dtype=torch.int64, device=dev)
    for steps in ((2, 3, 9), (0, 1, 0)):
        t = se3_draws(A, B, steps, state)
        assert t.shape == (A, B, 6) and t.dtype == torch.float32
        assert torch.equal(t, se3_draws(A, B, steps, state)), "not the same from run to run"
        assert not torch.equal(t, se3_draws(A, B, steps, state + torch.tensor([0, 1], device=dev))), "offset + 1 draws the same"
        t = t.cpu().double().reshape(-1, 6)
        u = t[:, :3]
        assert float(u.min()) >= -1.0 and float(u.max()) < 1.0
        assert abs(float(u.mean())) < 4.0 * (1.0 / math.sqrt(3.0)) / math.sqrt(u.numel())  # (a uniform on [-1,1): sigma 1/sqrt 3)
        n = t.size(0)
        for i, k in enumerate(steps):
            s = t[:, 3 + i]
            assert torch.equal(s, s.round()) and float(s.min()) == -k and float(s.max()) == k
            p = 1.0 / (2 * k + 1)
            sigma = math.sqrt(n * p * (1.0 - p))
            for v in range(-k, k + 1):
                count = int((s == v).sum())
                print(f"steps {steps} axis {i} value {v}: {count} of {n}, expected {n * p:.1f} +- {sigma:.1f}")
                assert abs(count - n * p) <= 4.0 * sigma + 1e-9


@gpu
def test_the_module_draws_what_se3_draws_names_and_advances_by_one_per_call():
    from manigaussian_amd.augmentation import se3_draws
    dev = torch.device("cuda:0")
    c = sc.load_cases()["b8_4x4_c3"]
    d = _device_inputs(c, dev)
    m = _module(c).to(dev).manual_seed(1234, 7)
    assert m.rng_state.tolist() == [1234, 7]
    table = se3_draws(sc.ATTEMPTS, 8, m.rot_steps, m.rng_state.clone())
    own = _call(m, d, draws=False)
    assert m.rng_state.tolist() == [1234, 8]
    given = _call(m, dict(d, draws=table))
    assert m.rng_state.tolist() == [1234, 8], "a call with injected draws consumed the stream"
    assert torch.equal(own[0], given[0]) and torch.equal(own[1], given[1])
    assert all(torch.equal(_bits(g), _bits(e)) for g, e in zip(own[2] + own[3], given[2] + given[3]))
    again = _call(m, d, draws=False)
    assert m.rng_state.tolist() == [1234, 9]
    assert not all(torch.equal(_bits(g), _bits(e)) for g, e in zip(own[2], again[2])), "two calls drew the same perturbation"
    fresh = _module(c)  # seeded from torch's seed at first use, then advanced
    torch.manual_seed(99)
    _call(fresh, d, draws=False)
    _call(fresh, d, draws=False)
    assert fresh.rng_state.tolist() == [99, 2] and fresh.rng_state.is_cuda and fresh.state_dict() == {}


@gpu
def test_augmentation_then_voxelizer_captured_into_a_hip_graph():
    """In a child process: stream capture is process-wide state (tests/tools/se3_graph_capture_check.py)."""
    run_graph_tool("se3_graph_capture_check.py")
