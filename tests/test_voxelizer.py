"""The fused voxelizer (manigaussian_amd/voxelizer.py, csrc/mgs_voxelize.hip) against ManiGaussian's voxel/voxel_grid.py.

The contract is BIT EQUALITY with the reference module run on a CPU, not a tolerance: the kernels perform the reference's fp32
operations (the index arithmetic step by step, correctly rounded divisions, every voxel's points added in ascending point
index from 0.0f, one division by the count), so there is nothing to round differently.  The GPU box has no reference: the
committed fixtures (tests/golden/voxelize/, what the reference gave where it exists) and voxelize_cases.restate (checked
against every fixture bit for bit on the CPU) stand in.
"""
import os

import pytest
import torch

from child import run_graph_tool
import voxelize_cases as vc

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEMORY = ("channels_first", "channels_last")


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(vc.CASES))
def test_the_restatement_reproduces_every_fixture(case):
    f = vc.load_fixture(case)
    vc.assert_case_is_what_it_claims(case, f["coords"], f["bounds"], f["V"])
    coords, features, bounds, V = vc.make_inputs(case)
    assert vc.same_bits(coords, f["coords"]) and vc.same_bits(bounds, f["bounds"]) and V == f["V"], "the input makers moved"
    assert (features is None) == (f["features"] is None) and (features is None or vc.same_bits(features, f["features"]))
    got = vc.restate(f["coords"], f["features"], f["bounds"], f["V"])
    assert vc.same_bits(got, vc.grid_of_fixture(f)), case


@pytest.mark.skipif(not vc.have_reference(), reason="no copy of the reference on this machine")
def test_fixtures_match_the_reference():
    """The generator's computation, re-run: the committed files are what the reference's VoxelGrid gives today."""
    for case in vc.CASES:
        f = vc.load_fixture(case)
        grid = vc.reference_run(f["coords"], f["features"], f["bounds"], f["V"])
        assert vc.same_bits(grid, vc.grid_of_fixture(f)), case


def test_fixtures_are_small():
    for case in vc.CASES:
        assert os.path.getsize(os.path.join(vc.GOLDEN_DIR, case + ".npz")) <= 1_000_000, case


def test_the_library_refuses_bad_arguments_before_any_launch():
    from manigaussian_amd import _lib
    L = _lib.lib()
    fake = 0x10000
    ws = L.mgs_voxelize_workspace_bytes(1, 16384, 100)
    INV, WS = _lib.MGS_ERR_INVALID_ARG, _lib.MGS_ERR_WORKSPACE

    def call(B=1, N=16384, V=100, Fc=3, cf=1, coords=fake, features=fake, bounds=fake, grid=fake, workspace=fake, nbytes=ws):
        return L.mgs_voxelize_forward(B, N, V, Fc, cf, coords, features, bounds, grid, workspace, nbytes, None)

    for kw, word in ((dict(B=0), "B = 0"), (dict(N=-1), "N = -1"), (dict(V=0), "V = 0"), (dict(N=(1 << 24) + 1), "2^24"),
                     (dict(B=3000, V=100), "2^31"), (dict(Fc=-1), "feature width"), (dict(Fc=65), "feature width 65"),
                     (dict(coords=None), "NULL"), (dict(features=None), "NULL"), (dict(bounds=None), "NULL"),
                     (dict(grid=None), "NULL"), (dict(workspace=None), "NULL"), (dict(Fc=0), "Fc = 0"),
                     (dict(grid=fake + 4), "16-byte aligned"), (dict(workspace=fake + 8), "16-byte aligned")):
        assert call(**kw) == INV, kw
        assert word in _lib.last_error(), (kw, _lib.last_error())
    assert call(nbytes=ws - 1) == WS and "needed" in _lib.last_error()
    assert call(nbytes=0) == WS
    ptrs = (_lib.c_fp * 2)(fake, fake)
    img = lambda **kw: L.mgs_voxelize_forward_images(kw.get("B", 1), kw.get("n", 2), kw.get("HW", 8192), 100, 3, 1, ptrs, ptrs, fake,
                                                     kw.get("grid", fake), fake, kw.get("nbytes", ws), None)
    assert img(n=0) == INV and img(n=9) == INV and img(HW=0) == INV and img(grid=fake + 4) == INV
    assert img(nbytes=ws - 1) == WS
    assert L.mgs_voxelize_forward_images(1, 2, 8192, 100, 3, 1, (_lib.c_fp * 2)(fake, None), ptrs, fake, fake, fake, ws, None) == INV
    assert "image 1" in _lib.last_error()


def test_the_workspace_size_is_monotone_and_aligned():
    from manigaussian_amd import _lib
    W = _lib.lib().mgs_voxelize_workspace_bytes
    base = W(1, 16384, 100)
    assert base >= 4 * 100 ** 3 + 8 * 16384 and base % 16 == 0
    assert W(4, 65536, 100) > 0, "the limits must admit B = 4, N = 65 536, V = 100"
    last = 0
    for B, N, V in ((1, 0, 1), (1, 0, 8), (1, 1000, 8), (1, 1000, 37), (1, 16384, 37), (1, 16384, 100), (1, 49152, 100),
                    (2, 49152, 100), (4, 65536, 100), (4, 65536, 128)):
        n = W(B, N, V)
        assert n > last and n % 16 == 0, (B, N, V, n, last)
        last = n
    assert W(0, 10, 10) == 0 and W(1, -1, 10) == 0 and W(1, 10, 0) == 0 and W(3000, 10, 100) == 0


def test_voxelgrid_refuses_cpu_tensors_a_wrong_feature_width_and_too_many_points():
    from manigaussian_amd import VoxelGrid, voxelize_images
    vg = VoxelGrid(list(vc.SCENE_BOUNDS), 10, "cpu", 1, 3, 100)
    assert len(vg.state_dict()) == 0 and not list(vg.parameters())
    xyz, rgb = torch.zeros(1, 50, 3), torch.zeros(1, 50, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        vg.coords_to_bounding_voxel_grid(xyz, coord_features=rgb)
    with pytest.raises(RuntimeError, match="no CPU path"):
        voxelize_images([torch.zeros(1, 3, 4, 4)], [torch.zeros(1, 3, 4, 4)], torch.tensor([vc.SCENE_BOUNDS]), 10)
    with pytest.raises(ValueError, match="memory"):
        VoxelGrid(list(vc.SCENE_BOUNDS), 10, "cpu", 1, 3, 100, memory="nhwc")
    with pytest.raises(ValueError, match="4 wide.*feature_size 3"):
        vg.coords_to_bounding_voxel_grid(xyz, coord_features=torch.zeros(1, 50, 4))
    with pytest.raises(ValueError, match="0 wide.*feature_size 3"):
        vg.coords_to_bounding_voxel_grid(xyz)
    with pytest.raises(ValueError, match="101 points.*max_num_coords 100"):
        vg.coords_to_bounding_voxel_grid(torch.zeros(1, 101, 3), coord_features=torch.zeros(1, 101, 3))


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
def _grid(f, dev, memory, **kw):
    from manigaussian_amd import VoxelGrid
    B, N = f["coords"].shape[:2]
    vg = VoxelGrid(list(vc.SCENE_BOUNDS), f["V"], dev, B, f["Fc"], N, memory=memory)
    feats = f["features"].to(dev) if f["features"] is not None else None
    return vg.coords_to_bounding_voxel_grid(f["coords"].to(dev), coord_features=feats, coord_bounds=f["bounds"].to(dev), **kw)


def _report(name, got, exp):
    """Print the figures before asserting: how many floats differ in their bits, and by how much."""
    g, e = got.detach().cpu(), exp
    diff = vc.bits(g) != vc.bits(e) if g.shape == e.shape else None
    n = int(diff.sum()) if diff is not None else -1
    err = float((torch.nan_to_num(g) - torch.nan_to_num(e)).abs().max()) if diff is not None and n else 0.0
    print(f"{name}: shape {tuple(g.shape)} vs {tuple(e.shape)}, {n} of {e.numel()} floats differ in bits, max abs {err:.3g}")
    return n


@gpu
@pytest.mark.parametrize("memory", MEMORY)
@pytest.mark.parametrize("case", list(vc.CASES))
def test_every_fixture_bit_for_bit(case, memory):
    dev = torch.device("cuda:0")
    f = vc.load_fixture(case)
    exp = vc.grid_of_fixture(f)
    B, V, Fc = exp.shape[0], f["V"], f["Fc"]
    vox = _grid(f, dev, memory)
    assert _report(f"{case}/{memory}", vox, exp) == 0
    assert vox.shape == (B, V, V, V, Fc + 7) and vox.dtype == torch.float32 and not vox.requires_grad
    if memory == "channels_first":
        assert vox.permute(0, 4, 1, 2, 3).is_contiguous(), "the caller's permute must give Conv3d a contiguous tensor"
    else:
        assert vox.is_contiguous()
    c = vox.cpu()
    assert torch.equal(vc.bits(c[..., Fc + 3:Fc + 6]), vc.bits(exp[..., Fc + 3:Fc + 6])), "index channels"
    assert torch.equal(c[..., -1], exp[..., -1]) and set(c[..., -1].unique().tolist()) <= {0.0, 1.0}, "occupancy"
    vox2, occ = _grid(f, dev, memory, return_density=True)
    assert occ.shape == (B, V, V, V, 1) and vc.same_bits(occ.cpu(), exp[..., -1:]) and vc.same_bits(vox2.cpu(), exp)
    only = _grid(f, dev, memory, only_features=True)
    assert only.shape == (B, V, V, V, Fc) and vc.same_bits(only.cpu(), exp[..., :Fc])


FULL = {
    "three_cameras": dict(B=1, N=49152, V=100, Fc=3, kind="depth", bounds="scene", seed=21),
    "batch_of_four": dict(B=4, N=16384, V=100, Fc=3, kind="depth", bounds="four", seed=22),
    "fc64_long_lists": dict(B=2, N=3000, V=6, Fc=64, kind="uniform", bounds="two", seed=23),
}


def _full_inputs(name):
    spec = dict(FULL[name])
    four = spec["bounds"] == "four"
    if four:
        spec["bounds"] = "scene"
    coords, features, bounds, V = vc.make_inputs(**spec)
    if four:  # per-item bounds: crops of the scene, as the agent's bounds_offset augmentation passes them
        for b in range(1, 4):
            bounds[b] += torch.tensor([0.03 * b, -0.02 * b, 0.01 * b, -0.05 * b, 0.02 * b, -0.03 * b])
    return coords, features, bounds, V


@gpu
@pytest.mark.parametrize("memory", MEMORY)
@pytest.mark.parametrize("name", list(FULL))
def test_the_restatement_at_full_size_bit_for_bit(name, memory):
    from manigaussian_amd.voxelizer import voxelize
    dev = torch.device("cuda:0")
    coords, features, bounds, V = _full_inputs(name)
    kept, voxels, most = vc.census(coords, bounds, V)
    print(f"{name}: {kept} points kept, {voxels} voxels, at most {most} in one")
    assert kept > 0 and (name != "fc64_long_lists" or most > 8)
    exp = vc.restate(coords, features, bounds, V)
    got = voxelize(coords.to(dev), features.to(dev), bounds.to(dev), V, memory)
    assert _report(f"{name}/{memory}", got, exp) == 0


@gpu
def test_two_calls_are_bit_identical_and_a_call_leaves_nothing_behind():
    """The same inputs twice; then other inputs of the same sizes (the same cached workspace), an empty cloud, and the first
    again: no voxel of an earlier call survives and none goes missing."""
    from manigaussian_amd.voxelizer import voxelize
    dev = torch.device("cuda:0")
    f = vc.load_fixture("mani_16384_v100")
    exp = vc.grid_of_fixture(f)
    a = [t.to(dev) for t in (f["coords"], f["features"], f["bounds"])]
    for memory in MEMORY:
        one = voxelize(*a, f["V"], memory)
        two = voxelize(*a, f["V"], memory)
        assert one.data_ptr() != two.data_ptr() and vc.same_bits(one.cpu(), two.cpu())
        other = vc.make_inputs(B=1, N=16384, V=100, Fc=3, kind="one_voxel", bounds="scene", seed=31)
        got = voxelize(other[0].to(dev), other[1].to(dev), other[2].to(dev), 100, memory)
        assert _report(f"after another call/{memory}", got, vc.restate(*other)) == 0
        far = torch.full((1, 16384, 3), 50.0, device=dev)
        got = voxelize(far, a[1], a[2], 100, memory)
        assert _report(f"empty cloud/{memory}", got, vc.background(1, 100, 3)) == 0
        assert _report(f"the first again/{memory}", voxelize(*a, f["V"], memory), exp) == 0
    none = voxelize(torch.zeros(1, 0, 3, device=dev), torch.zeros(1, 0, 3, device=dev), a[2], 100)
    assert _report("N = 0", none, vc.background(1, 100, 3)) == 0


@gpu
@pytest.mark.parametrize("memory", MEMORY)
def test_voxelize_images_equals_the_flattened_call(memory):
    from manigaussian_amd import voxelize_images
    from manigaussian_amd.voxelizer import voxelize
    dev = torch.device("cuda:0")
    B, H, W, V = 2, 64, 96, 50
    g = torch.Generator().manual_seed(41)
    bounds = vc.make_bounds("two", B).to(dev)
    pcds, rgbs = [], []
    for cam in range(3):
        cloud = vc.depth_cloud(g, B, H * W)
        pcds.append(cloud.view(B, H, W, 3).permute(0, 3, 1, 2).contiguous().to(dev))
        rgbs.append((torch.randint(0, 256, (B, 3, H, W), generator=g).float() / 255.0 * 2 - 1).to(dev))
    # ...agent.py:205-214: camera after camera, row-major pixels
    flat_pcd = torch.cat([p.permute(0, 2, 3, 1).reshape(B, -1, 3) for p in pcds], 1)
    flat_rgb = torch.cat([p.permute(0, 2, 3, 1).reshape(B, -1, 3) for p in rgbs], 1)
    exp = vc.restate(flat_pcd.cpu(), flat_rgb.cpu(), bounds.cpu(), V)
    assert _report(f"flattened/{memory}", voxelize(flat_pcd, flat_rgb, bounds, V, memory), exp) == 0
    assert _report(f"images/{memory}", voxelize_images(pcds, rgbs, bounds, V, memory), exp) == 0
    none = voxelize_images(pcds, None, bounds, V, memory)
    assert _report(f"images, no features/{memory}", none, vc.restate(flat_pcd.cpu(), None, bounds.cpu(), V)) == 0


@gpu
def test_the_output_is_detached_and_a_side_stream_works():
    from manigaussian_amd import VoxelGrid
    dev = torch.device("cuda:0")
    f = vc.load_fixture("odd_v37_n1000")
    exp = vc.grid_of_fixture(f)
    coords = f["coords"].to(dev).requires_grad_(True)
    feats = f["features"].to(dev).requires_grad_(True)
    vg = VoxelGrid(f["bounds"][0].tolist(), f["V"], dev, 1, 3, 1000)  # (the constructor's bounds, kept on the device)
    vox = vg.coords_to_bounding_voxel_grid(coords, coord_features=feats)
    assert not vox.requires_grad and vox.grad_fn is None and vc.same_bits(vox.cpu(), exp)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = vg.coords_to_bounding_voxel_grid(coords, coord_features=feats)
    side.synchronize()
    assert vc.same_bits(on_side.cpu(), exp)
    torch.cuda.synchronize()


@gpu
def test_voxelize_then_point_latent_captured_into_a_hip_graph():
    """In a child process: stream capture is process-wide state (tests/tools/voxelize_graph_capture_check.py)."""
    run_graph_tool("voxelize_graph_capture_check.py")
