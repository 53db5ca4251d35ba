"""Cases, seeded inputs, fixtures and a plain-torch restatement for tests/test_voxelizer.py -- TEST INFRASTRUCTURE, shared with
tests/golden/make_golden_voxelize.py (which records what `reference_run()` returns).

The reference is ManiGaussian's voxel/voxel_grid.py, executed unmodified on the CPU.  It exists only where a development copy
of the reference does (tests/ref_import.py's first candidate, $MGS_REFERENCE_ROOT); everywhere else the fixtures under
tests/golden/voxelize/ stand in.  A fixture holds the inputs (coords, features, bounds, V) and the reference's grid SPARSELY:
occ_index [K,4] int32 (b, x, y, z) of the occupied voxels, sorted, and occ_values [K,Fc+3] fp32, their mean channels; the
rest of the grid is the closed-form background (0, index / V, occupancy 0).  `dense_v8` stores the reference's whole grid, so
that the background itself is pinned by the reference and not by this file.

`restate()` is the voxelizer written once more for this repository, in torch on the CPU: the index arithmetic step by step in
fp32, index_add_ in point order, one division.  It is checked against every fixture BIT FOR BIT, and then serves as the truth
at sizes the fixtures cannot hold.
"""
import importlib.util
import os

import numpy as np
import torch

import ref_import
from numerics import bits, same_bits  # noqa: F401  (re-exported: the tests and the tools reach them through this module)

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_DIR = os.path.join(HERE, "golden", "voxelize")
SCENE_BOUNDS = (-0.3, -0.5, 0.6, 0.7, 0.5, 1.6)  # conf/config.yaml:21
REF_FILE = os.path.join(ref_import._CANDIDATES[0], "voxel", "voxel_grid.py")

# name: B, N, V, Fc, the cloud's kind and the bounds ("scene": SCENE_BOUNDS for every item; "two": the second item's are shifted)
CASES = {
    "mani_16384_v100": dict(B=1, N=16384, V=100, Fc=3, kind="depth", bounds="scene", seed=1),
    "b2_v20":          dict(B=2, N=8192, V=20, Fc=3, kind="depth", bounds="two", seed=2),
    "one_voxel":       dict(B=1, N=4096, V=10, Fc=3, kind="one_voxel", bounds="scene", seed=3),
    "all_outside":     dict(B=1, N=1000, V=10, Fc=3, kind="outside", bounds="scene", seed=4),
    "edges_nonfinite": dict(B=1, N=600, V=10, Fc=3, kind="edges", bounds="scene", seed=5),
    "fc0":             dict(B=1, N=2000, V=16, Fc=0, kind="uniform", bounds="scene", seed=6),
    "fc8":             dict(B=1, N=2000, V=16, Fc=8, kind="uniform", bounds="scene", seed=7),
    "odd_v37_n1000":   dict(B=1, N=1000, V=37, Fc=3, kind="uniform", bounds="scene", seed=8),
    "dense_v8":        dict(B=2, N=500, V=8, Fc=3, kind="uniform", bounds="two", seed=9, dense=True),
}


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def make_bounds(kind, B):
    b = torch.tensor([SCENE_BOUNDS] * B, dtype=torch.float32)
    if kind == "two" and B > 1:
        b[1] += torch.tensor([0.05, -0.02, 0.01, 0.07, -0.03, 0.02])
    return b


def _colours(g, B, N, Fc):
    """8-bit colours scaled to [-1, 1] like the agent's (they also compress well in a fixture); other widths: random normal."""
    if Fc == 0:
        return None
    if Fc == 3:
        return torch.randint(0, 256, (B, N, 3), generator=g).float() / 255.0 * 2.0 - 1.0
    return torch.randn(B, N, Fc, generator=g)


def depth_cloud(g, B, N):
    """A depth-map-like cloud: a tilted, noisy surface seen pixel by pixel that overhangs the scene bounds in x and y, so that
    about 30 % of the points lie outside."""
    u = torch.rand(B, N, 2, generator=g)
    z = 0.8 + 0.3 * u[..., :1] + 0.02 * torch.randn(B, N, 1, generator=g)
    return torch.cat([-0.4 + 1.2 * u[..., :1], -0.6 + 1.2 * u[..., 1:], z], -1).float()


def make_inputs(case=None, **spec):
    """(coords [B,N,3], features [B,N,Fc] or None, bounds [B,6], V) of a named case or of a spec like the entries of CASES."""
    c = dict(CASES[case]) if case is not None else spec
    B, N, V, Fc = c["B"], c["N"], c["V"], c["Fc"]
    g = torch.Generator().manual_seed(c["seed"])
    bounds = make_bounds(c["bounds"], B)
    lo, hi = bounds[:, None, :3], bounds[:, None, 3:]
    kind = c["kind"]
    if kind == "depth":
        xyz = depth_cloud(g, B, N)
    elif kind == "uniform":  # the box grown by 10 % on every side
        xyz = lo - 0.1 * (hi - lo) + 1.2 * (hi - lo) * torch.rand(B, N, 3, generator=g)
    elif kind == "one_voxel":  # well inside voxel (3, 4, 5): its centre +- 0.3 of a voxel
        res = (hi - lo) / V
        xyz = lo + res * (torch.tensor([3.5, 4.5, 5.5]) + 0.6 * (torch.rand(B, N, 3, generator=g) - 0.5))
    elif kind == "outside":  # beyond the upper or below the lower bound on at least the x axis
        xyz = lo + (hi - lo) * torch.rand(B, N, 3, generator=g)
        side = torch.rand(B, N, generator=g) < 0.5
        xyz[..., 0] = torch.where(side, hi[..., 0] + 0.01 + torch.rand(B, N, generator=g), lo[..., 0] - 0.01 - torch.rand(B, N, generator=g))
    elif kind == "edges":
        xyz = lo + (hi - lo) * torch.rand(B, N, 3, generator=g)
        res = ((hi - lo) / (torch.tensor(float(V)) + 1e-12))[0, 0]
        lo0, hi0 = lo[0, 0], hi[0, 0]
        i = 0
        for ax in range(3):  # exactly on the lower and the upper bound, and on every k res boundary computed two ways
            xyz[0, i, ax] = lo0[ax]; i += 1
            xyz[0, i, ax] = hi0[ax]; i += 1
            for k in range(V + 1):
                xyz[0, i, ax] = lo0[ax] + k * res[ax]; i += 1
                xyz[0, i, ax] = hi0[ax] - k * res[ax]; i += 1
                xyz[0, i, ax] = torch.nextafter(lo0[ax] + k * res[ax], hi0[ax]); i += 1
                xyz[0, i, ax] = torch.nextafter(lo0[ax] + k * res[ax], lo0[ax] - 1); i += 1
        for bad in (float("nan"), float("inf"), float("-inf"), 1e30, -1e30, 3e38, -3e38, 2.2e9, -2.2e9):
            for ax in range(3):
                xyz[0, i, ax] = bad; i += 1
        xyz[0, i] = float("nan"); i += 1
        assert i <= N
    else:
        raise KeyError(kind)
    return xyz.float().contiguous(), _colours(g, B, N, Fc), bounds, V


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def background(B, V, Fc):
    """The grid of an empty cloud: zeros, index / V in channels Fc + 3 .. Fc + 5 (voxel_grid.py:219-221), occupancy 0."""
    g = torch.zeros(B, V, V, V, Fc + 7, dtype=torch.float32)
    ar = torch.arange(V, dtype=torch.float32) / float(V)
    g[..., Fc + 3] = ar.view(1, V, 1, 1)
    g[..., Fc + 4] = ar.view(1, 1, V, 1)
    g[..., Fc + 5] = ar.view(1, 1, 1, V)
    return g


def voxel_indices(coords, bounds, V):
    """(keep [B,N] bool, lin [B,N] int64 = the voxel inside the whole batch's grid, of kept points).  Every step is one fp32
    operation, as in voxel_grid.py:170-183.  Index 0 or V + 1 (after the reference's clamp) is the cropped shell: dropped,
    with everything that is not finite."""
    B = coords.shape[0]
    bounds = bounds.reshape(-1, 6).float().expand(B, 6)
    mn, mx = bounds[:, None, :3], bounds[:, None, 3:]
    res = (mx - mn) / (torch.tensor(float(V), dtype=torch.float32) + 1e-12)
    den = res + 1e-12
    shift = mn - res
    f = torch.floor((coords.float() - shift) / den)
    keep = ((f >= 1) & (f <= V)).all(-1)
    i = torch.where(keep[..., None], f, torch.ones_like(f)).long() - 1
    b = torch.arange(B).view(B, 1)
    lin = ((b * V + i[..., 0]) * V + i[..., 1]) * V + i[..., 2]
    return keep, lin


def restate(coords, features, bounds, V):
    """[B,V,V,V,Fc+7] fp32, the reference's values: per voxel the sum of [features | xyz] of its points in point order from 0,
    divided once by the count."""
    B, N, _ = coords.shape
    Fc = 0 if features is None else features.shape[-1]
    keep, lin = voxel_indices(coords, bounds, V)
    vals = coords.float() if Fc == 0 else torch.cat([features.float(), coords.float()], -1)
    sums = torch.zeros(B * V ** 3, Fc + 3, dtype=torch.float32)
    count = torch.zeros(B * V ** 3, dtype=torch.float32)
    sel = lin[keep]
    src = vals[keep]
    for c in range(Fc + 3):  # one channel at a time: a 1-D index_add_ on the CPU walks the index in order
        sums[:, c].index_add_(0, sel, src[:, c].contiguous())
    count.index_add_(0, sel, torch.ones(sel.numel()))
    grid = background(B, V, Fc)
    flat = grid.view(B * V ** 3, Fc + 7)
    flat[:, :Fc + 3] = sums / count.clamp(min=1)[:, None]
    flat[:, Fc + 6] = (count > 0).float()
    return grid


# ---- the reference -------------------------------------------------------------------------------------------------------------
def have_reference() -> bool:
    return os.path.isfile(REF_FILE)


def reference_run(coords, features, bounds, V):
    """voxel/voxel_grid.py, unmodified, on the CPU (it imports only torch)."""
    spec = importlib.util.spec_from_file_location("_mgs_reference_voxel_grid", REF_FILE)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    B, N, _ = coords.shape
    Fc = 0 if features is None else features.shape[-1]
    vg = mod.VoxelGrid(list(SCENE_BOUNDS), V, "cpu", B, Fc, N)
    with torch.no_grad():
        vox, occ = vg.coords_to_bounding_voxel_grid(coords, coord_features=features, coord_bounds=bounds, return_density=True)
    assert torch.equal(occ[..., 0], vox[..., -1])
    return vox.contiguous()


# ---- fixtures ------------------------------------------------------------------------------------------------------------------
def fixture_of_grid(case, coords, features, bounds, V, grid):
    Fc = 0 if features is None else features.shape[-1]
    occ = grid[..., -1] > 0
    index = occ.nonzero().int()  # row-major: sorted by (b, x, y, z)
    out = dict(coords=coords.numpy(), features=(features.numpy() if features is not None else np.zeros((0,), np.float32)),
               bounds=bounds.numpy(), V=np.int32(V), Fc=np.int32(Fc), occ_index=index.numpy(),
               occ_values=grid[occ][:, :Fc + 3].numpy())
    sparse = grid_of_fixture({k: torch.from_numpy(np.asarray(v)) for k, v in out.items()})
    assert same_bits(sparse, grid), f"{case}: the grid is not its occupied voxels over the closed-form background"
    if CASES[case].get("dense"):
        out["grid"] = grid.numpy()
    return out


def load_fixture(case):
    with np.load(os.path.join(GOLDEN_DIR, case + ".npz")) as z:
        f = {k: torch.from_numpy(z[k]) for k in z.files}
    f["V"], f["Fc"] = int(f["V"]), int(f["Fc"])
    f["features"] = f["features"] if f["Fc"] > 0 else None
    return f


def grid_of_fixture(f):
    """The reference's dense grid: the stored one, or the occupied voxels over the closed-form background."""
    if "grid" in f:
        return f["grid"]
    B, V, Fc = f["coords"].shape[0], int(f["V"]), int(f["Fc"])
    g = background(B, V, Fc)
    i = f["occ_index"].long()
    g[i[:, 0], i[:, 1], i[:, 2], i[:, 3], :Fc + 3] = f["occ_values"]
    g[i[:, 0], i[:, 1], i[:, 2], i[:, 3], Fc + 6] = 1.0
    return g


def census(coords, bounds, V):
    """(points kept, occupied voxels, most points in one voxel)."""
    keep, lin = voxel_indices(coords, bounds, V)
    if not keep.any():
        return 0, 0, 0
    n = torch.bincount(lin[keep])
    return int(keep.sum()), int((n > 0).sum()), int(n.max())


def assert_case_is_what_it_claims(case, coords, bounds, V):
    """A fixture that lost its point (no long lists, nothing outside) would pass and test nothing."""
    kept, voxels, most = census(coords, bounds, V)
    N = coords.shape[0] * coords.shape[1]
    if case == "mani_16384_v100":
        assert 0.6 * N < kept < 0.8 * N and voxels > 5000 and 2 <= most <= 8, (kept, voxels, most)
    elif case == "b2_v20":
        assert most >= 20 and len({tuple(r) for r in bounds.tolist()}) == 2, most
    elif case == "one_voxel":
        assert kept == N and voxels == 1
    elif case == "all_outside":
        assert kept == 0
    elif case == "edges_nonfinite":
        assert not torch.isfinite(coords).all() and 0 < kept < N
    else:
        assert 0 < kept < N and voxels > 1
