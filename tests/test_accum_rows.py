"""The render backward's hand-over rows (mgs_render_bwd_gm.hip): with SH colours the nine scalar sums of a (view, Gaussian)
leave as one 64-byte row of acc16 (geometry in slots 0-5, dR dG dB in 6-8, copied to dL_dcolors by the preprocess backward);
with colors_precomp the geometry goes to acc16 and the colours to the caller's [P,3] table.  Small scenes that still reach
every path of the hand-over: a ragged 4-Gaussians-per-instruction tail (P = 2 999), blocks with more than 64 survivors (both
groups of a chunk, at least two chunks) and Gaussians blended from several blocks (rows that several workgroups add into).

Everything is compared with Oracle B through the helpers and tolerances test_gpu_parity.py uses."""
import numpy as np
import pytest
import torch

import util
from manigaussian_amd import GaussianRasterizationSettings, GaussianRasterizerBatch, _C, _lib
from manigaussian_amd import synthetic as syn
from test_gpu_parity import GRAD_TOL, IMG_TOL

pytestmark = pytest.mark.gpu

P, W, H, V = 2999, 64, 64, 3
BG = (0.1, 0.2, 0.3)
SH_C0 = 0.28209479177387814  # the degree-0 basis function (the reference's SH_C0)


@pytest.fixture(autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need a HIP device"
    _lib.lib()
    yield


def block_incidence(st):
    """(most Gaussians blended by one 8x8 block, most blocks one Gaussian is blended from), from the oracle's own lists: pair
    (pixel, entry j of its tile's list) is blended iff j < n_contrib[pixel], power <= 0 and alpha >= 1/255.  A block's survivors
    in the HIP kernels are a superset of the Gaussians it blends."""
    m2, co = st.array("means2D"), st.array("conic_opacity")
    pl, rg = st.array("point_list").astype(np.int64), st.array("ranges").astype(np.int64)
    nc = st.array("n_contrib").reshape(st.H, st.W).astype(np.int64)
    tiles_x = (st.W + 15) // 16
    most, blocks_of = 0, np.zeros(st.P, np.int64)
    for t in range(rg.shape[0]):
        ids = pl[rg[t, 0]:rg[t, 1]]
        if ids.size == 0:
            continue
        x0, y0 = (t % tiles_x) * 16, (t // tiles_x) * 16
        for by in (0, 8):
            for bx in (0, 8):
                ys, xs = np.arange(y0 + by, min(y0 + by + 8, st.H)), np.arange(x0 + bx, min(x0 + bx + 8, st.W))
                if ys.size == 0 or xs.size == 0:
                    continue
                px, py = [a.ravel() for a in np.meshgrid(xs, ys)]
                n = nc[py, px]
                k = int(n.max())
                if k == 0:
                    continue
                g = ids[:k]
                dx = m2[g, 0][None, :] - px[:, None].astype(np.float32)
                dy = m2[g, 1][None, :] - py[:, None].astype(np.float32)
                power = -0.5 * (co[g, 0] * dx * dx + co[g, 2] * dy * dy) - co[g, 1] * dx * dy
                alpha = np.minimum(0.99, co[g, 3] * np.exp(np.minimum(power, 0.0)))
                hit = ((np.arange(k)[None, :] < n[:, None]) & (power <= 0) & (alpha >= 1.0 / 255.0)).any(0)
                most = max(most, int(hit.sum()))
                np.add.at(blocks_of, g[hit], 1)
    return most, int(blocks_of.max())


_REF = {}


def reference(F=32, inc=True, deg=1, precomp=False, view=1):
    """(scene, camera, settings, cotangents, Oracle B's results) of one view, computed once per module and not modified."""
    key = (F, inc, deg, precomp, view)
    if key not in _REF:
        sc, cam, kw, dC, dF = util.scene_case(P=P, F=F, W=W, H=H, sh_degree=deg, include_feature=inc, cam_index=view)
        if precomp:  # the colours the SH scene has at degree 0 (the same in every view), as precomputed colours
            rgb = SH_C0 * sc.pop("shs")[:, 0] + 0.5
            assert float(rgb.min()) > 0.0  # (nothing clamped)
            sc["colors_precomp"] = rgb.contiguous()
        _REF[key] = (sc, cam, kw, dC, dF, util.run_oracle_b(sc, kw, dC, dF))
    return _REF[key]


def assert_matches_oracle(got, ref, inc=True):
    """test_gpu_parity._check_'s comparison."""
    ch, fh, rh, gh = got
    cr, fr, rr, gr, st = ref
    assert torch.equal(rh, rr), "radii differ"
    for nm, a, b in [("color", ch, cr)] + ([("feature", fh, fr)] if inc else []):
        robust, fragile, frac = util.image_errors(a, b, st)
        assert robust <= IMG_TOL, f"{nm}: {robust:.3e} on threshold-robust pixels"
        assert fragile <= util.FRAGILE_TOL and frac <= util.FRAGILE_MAX_FRACTION, (nm, fragile, frac)
    errs, frac = util.grad_errors_split(gh, gr, st)
    assert frac <= 0.05
    for k, (robust, fragile, mag) in errs.items():
        assert robust <= GRAD_TOL * mag + 1e-7, f"grad {k}: err {robust:.3e} vs max {mag:.3e}"
        assert fragile <= util.FRAGILE_GRAD_TOL * mag + 1e-7, f"grad {k} (threshold-fragile): {fragile:.3e} vs {mag:.3e}"


def assert_same_sums(got, ref, keys, what):
    """Two runs of the same sums in another atomic order (the bound of test_view_batch_equals_per_view_calls)."""
    for k in keys:
        d, mag = (got[k] - ref[k]).abs().max().item(), ref[k].abs().max().item()
        assert d <= 2e-5 * mag + 1e-9, (what, k, d, mag)


def run_single(F=32, inc=True, deg=1, precomp=False, compiled=True):
    sc, cam, kw, dC, dF, ref = reference(F, inc, deg, precomp)
    if compiled:
        assert _C.compiled() is not None
    with _C.use_compiled(compiled):
        return util.run_hip(sc, cam, dC, dF, deg, inc, BG), ref


def test_the_scene_reaches_both_groups_two_chunks_and_shared_rows():
    """Oracle B's data: some 8x8 block blends more than 64 Gaussians (its survivor list is at least as long: two chunks, both
    32-entry groups of the first), and some Gaussian is blended from several blocks (its row is added to by several waves)."""
    most, shared = block_incidence(reference()[5][4])
    assert most > 64 and shared > 1, (most, shared)


@pytest.mark.parametrize("F,inc", [(32, True), (3, True), (3, False)], ids=["f32", "f3", "rgb_only"])
def test_sh_colours_ragged_tail_matches_oracle(F, inc):
    """P = 2 999: the last merged-row instruction of the last group covers fewer than four Gaussians."""
    got, ref = run_single(F, inc)
    assert_matches_oracle(got, ref, inc)


def test_ctypes_shim_sizes_the_rows_like_the_compiled_binding():
    """The two host paths size and zero the accumulator block separately."""
    got_c, ref = run_single(compiled=True)
    got_p, _ = run_single(compiled=False)
    assert_matches_oracle(got_c, ref)
    assert_matches_oracle(got_p, ref)
    assert torch.equal(got_c[0], got_p[0]) and torch.equal(got_c[1], got_p[1])
    assert_same_sums(got_p[3], got_c[3], got_c[3].keys(), "ctypes vs compiled")


@pytest.mark.parametrize("compiled", [True, False], ids=["compiled", "ctypes"])
def test_second_step_finds_every_slot_zeroed(compiled):
    """Forward, backward, forward, backward: the second forward's preprocess zeroes the block the first backward added into
    (the allocator hands the same memory out again), slots 6-8 of every row included."""
    first, ref = run_single(compiled=compiled)
    second, _ = run_single(compiled=compiled)
    assert_matches_oracle(second, ref)
    assert_same_sums(second[3], first[3], first[3].keys(), "second step")


def run_batch(sc, cams, dC, dF, deg):
    dev = torch.device("cuda:0")
    sets = [GaussianRasterizationSettings(**syn.camera_settings_kwargs(c, deg, True, bg=BG, device=dev)) for c in cams]
    d = {k: v.to(dev).clone().requires_grad_(True) for k, v in sc.items()}
    m2 = torch.zeros(len(cams), P, 3, device=dev, requires_grad=True)
    kw = dict(colors_precomp=d["colors_precomp"]) if "colors_precomp" in d else dict(shs=d["shs"])
    cb, fb, rb = GaussianRasterizerBatch(sets)(d["means3D"], m2, d["opacities"], scales=d["scales"],
                                               language_feature_precomp=d["language_feature"], rotations=d["rotations"], **kw)
    torch.autograd.backward([cb, fb], [dC.to(dev), dF.to(dev)])
    torch.cuda.synchronize()
    grads = {k: v.grad.cpu() for k, v in d.items()}
    grads["means2D"] = m2.grad.cpu()
    return cb.detach().cpu(), fb.detach().cpu(), rb.cpu(), grads


def batch_case(deg=1, precomp=False):
    """V views of the scene: per-view references (shared with the single-view tests where the view is theirs), stacked
    cotangents, and the batched HIP run compared with Oracle B as test_view_batch_matches_oracle_b does."""
    refs = [reference(deg=deg, precomp=precomp, view=v) for v in range(V)]
    sc = refs[0][0]
    dC, dF = torch.stack([r[3] for r in refs]), torch.stack([r[4] for r in refs])
    cb, fb, rb, gb = run_batch(sc, [r[1] for r in refs], dC, dF, deg)
    from oracle import oracle_b
    acc, fragile = None, torch.zeros(P, dtype=torch.bool)
    for v, r in enumerate(refs):
        cr, fr, rr, gr, st = r[5]
        assert torch.equal(rb[v], rr), f"radii, view {v}"
        for a, b in ((cb[v], cr), (fb[v], fr)):
            robust, frag, frac = util.image_errors(a, b, st)
            assert robust <= IMG_TOL and frag <= util.FRAGILE_TOL and frac <= util.FRAGILE_MAX_FRACTION, f"view {v}"
        fg = oracle_b.fragile_gaussians(st)
        fragile |= fg
        r2 = gr["means2D"]
        e2 = (gb["means2D"][v] - r2).abs().max(1)[0]  # per view: rows of the batch are indexed by the virtual id
        assert e2[~fg].max().item() <= GRAD_TOL * r2.abs().max().item() + 1e-7, f"means2D, view {v}"
        assert e2.max().item() <= util.FRAGILE_GRAD_TOL * r2.abs().max().item() + 1e-7, f"means2D, view {v}"
        acc = {k: t.clone() for k, t in gr.items()} if acc is None else {k: acc[k] + gr[k] for k in acc}
    assert fragile.float().mean().item() <= 0.1
    for k, got in gb.items():
        if k == "means2D":
            continue
        ref = acc[util.GRAD_KEYS[k]].reshape(got.shape)
        d = (got - ref).abs().reshape(P, -1).max(1)[0]
        mag = ref.abs().max().item()
        assert d[~fragile].max().item() <= GRAD_TOL * mag + 1e-7, k
        assert d.max().item() <= util.FRAGILE_GRAD_TOL * mag + 1e-7, k
    return (cb, fb, rb, gb)


def test_view_batch_with_sh_colours_matches_oracle():
    """Three views in one call: the merged rows are indexed by the virtual id v * P + i, the SH gradient sums the views."""
    batch_case(deg=1)


SHARED = ("means3D", "means2D", "opacities", "scales", "rotations", "language_feature")


def test_precomputed_colours_keep_the_two_table_path_single_view():
    """colors_precomp = the degree-0 SH colours: the same images and the same geometry sums as the SH run, the colour sums in
    the caller's [P,3] table instead of slots 6-8 (dL_dsh[:, 0] = SH_C0 dL_dcolour)."""
    sh, ref_sh = run_single(deg=0)
    pre, ref_pre = run_single(deg=0, precomp=True)
    assert_matches_oracle(sh, ref_sh)
    assert_matches_oracle(pre, ref_pre)
    assert torch.equal(pre[2], sh[2])
    assert_same_sums(pre[3], sh[3], SHARED, "precomp vs SH")
    assert_same_sums({"c": SH_C0 * pre[3]["colors_precomp"]}, {"c": sh[3]["shs"][:, 0]}, ["c"], "colour sums")


def test_precomputed_colours_keep_the_two_table_path_view_batch():
    """The same for the 3-view batch: [V P] merged rows with SH colours, one [P,3] colour table summed over the views with
    colors_precomp."""
    sh = batch_case(deg=0)
    pre = batch_case(deg=0, precomp=True)
    assert torch.equal(pre[2], sh[2])
    assert_same_sums(pre[3], sh[3], SHARED, "precomp vs SH, batch")
    assert_same_sums({"c": SH_C0 * pre[3]["colors_precomp"]}, {"c": sh[3]["shs"][:, 0]}, ["c"], "colour sums, batch")
