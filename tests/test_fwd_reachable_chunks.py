"""GPU tests of the render forward's second chunk slot (csrc/mgs_render_dense.hip): a round evaluates the chunks of its
second slot only as far as some pixel of the block is alive entering them; MgsOptions.dbg & 1 << 17 selects the earlier,
eager form that evaluates every chunk of a round ahead of its one barrier.  The two forms must agree bit for bit in
everything the forward hands out, and both must be the reference's render.

The scenes (tests/reachable_chunks_cases.py) are stacks of large, low-opacity Gaussians over a 16 x 16 image -- one tile,
four blocks, every list entry a survivor of every block -- whose opacity chooses how many chunks a block visits.  What a scene
reaches is decided on the CPU by a model of the chunk walk over Oracle B's lists (`reach` below) and then read back from the
GPU through mgs_forward_stats: the three counts must be the model's wherever the model sits further than 1e-3 (relative)
from every alive / dead decision -- a product of <= 2400 factors differs between two association orders by far less."""
import ctypes

import numpy as np
import pytest
import torch

from child import run_graph_tool
import reachable_chunks_cases as rc
import util
from manigaussian_amd import _C, _lib
from manigaussian_amd import GaussianRasterizationSettings, GaussianRasterizer
from manigaussian_amd import synthetic as syn

pytestmark = pytest.mark.gpu

EAGER = 1 << 17   # MgsOptions.dbg: every chunk of a round evaluated ahead of its one barrier (include/mgsplat.h)
NP16 = 8          # chunks per slot of the 16-wave form (one per wave pair); the 8-wave form's slot holds 4
ROBUST = 1e-3     # the model's counts bind the GPU where no decision of the model is closer than this to its threshold


def _near_threshold_opacities(pick):
    """Two neighbouring float32 opacities of the uniform 1100-stack between which the pixel `pick` chooses (np.min: the least
    transparent one, np.max: the most transparent one) changes sides entering chunk 8: alive with the lower opacity, dead with
    the higher one -- its transmittance there a few ulps either side of 1e-4."""
    def least(o):
        sc, cam, kw, dC, dF = rc.stack_scene(n=1100, opacity=float(o), F=3)
        return pick(rc.chunk_model(rc.oracle_forward(sc, kw)[3]).enter[0][NP16])
    lo, hi = np.float32(0.017), np.float32(0.019)
    assert least(lo) >= np.float32(rc.T_STOP) > least(hi)
    while np.nextafter(lo, np.float32(1)) < hi:
        mid = np.float32((np.float64(lo) + np.float64(hi)) / 2)
        if least(mid) >= np.float32(rc.T_STOP):
            lo = mid
        else:
            hi = mid
    return float(lo), float(hi)


def _all(m, lo, hi):
    return all(lo <= v <= hi for v in m.block_vis.values())


# name: (stack_scene arguments, what the model must show the scene to reach)
CASES = {
    # (a) the fill delivers 16 chunks, every pixel is dead before chunk 8: no second slot at all
    "a_16_filled_5_visited_second_slot_skipped": (
        dict(n=1100, opacity=rc.die_after(300)), lambda m: m.n[0] >= 1024 and _all(m, 1, NP16 - 1)),
    # (b) the list ends after 540 survivors: 8 full chunks and a short ninth, all visited
    "b_540_survivors_short_ninth_chunk": (
        dict(n=540, opacity=0.012), lambda m: 513 <= m.n[0] <= 575 and _all(m, 9, 9)),
    # (c) 9 or 10 chunks visited: the second slot's first group only
    "c_10_visited_first_group_only": (
        dict(n=1100, opacity=rc.die_after(600)), lambda m: m.n[0] >= 1024 and _all(m, 9, 10)),
    # (d) 11..16 visited: both groups
    "d_14_visited_both_groups": (
        dict(n=1100, opacity=rc.die_after(850)), lambda m: m.n[0] >= 1024 and _all(m, 11, 16)),
    # (e) a second round, whose second slot nobody reaches / somebody reaches
    "e_24_visited_round_1_skips_its_second_slot": (
        dict(n=2400, opacity=rc.die_after(1500)), lambda m: m.n[0] >= 2048 and _all(m, 17, 24)),
    "e_27_visited_round_1_needs_its_second_slot": (
        dict(n=2400, opacity=rc.die_after(1690)), lambda m: m.n[0] >= 2048 and _all(m, 25, 32)),
    # (f) entering chunk 8 the rows 0..3 of the upper blocks are alive and their rows 4..7 dead (a wave blends one half block);
    #     the lower blocks are dead altogether
    "f_one_half_block_alive_entering_chunk_8": (
        dict(n=1100, opacity=0.0200, sigma_px=(600.0, 12.0), centre_px=(0.0, -2.0)),
        lambda m: (m.enter[0][NP16][0:4, :] >= 1e-4).all() and (m.enter[0][NP16][4:16, :] < 1e-4).all()),
}
# (h) 288 blocks: the 8-wave form (two workgroups per CU), whose second slot starts at chunk 4; 6 and 7 chunks visited, i.e.
#     blocks that stop in the first group (chunks 4, 5) and blocks that need the second (6, 7)
WIDE = dict(n=700, opacity=rc.die_after(340), W=144, H=128, sigma_px=(150.0, 150.0))


def _forward_backward(sc, cam, dC, dF, F, dbg):
    """One forward + backward on the GPU under MgsOptions.dbg = dbg -> (color, feat, radii, grads, the three stats counts)."""
    dev = torch.device("cuda:0")
    old = _lib.get_option("dbg")
    try:
        _lib.set_option("dbg", dbg)
        kw = syn.camera_settings_kwargs(cam, 1, F > 0, bg=(0.1, 0.2, 0.3), device=dev)
        leaves = {k: v.to(dev).requires_grad_(True) for k, v in sc.items()}
        m2 = torch.zeros(sc["means3D"].shape[0], 3, device=dev, requires_grad=True)
        with _C.use_compiled(False):  # (the ctypes shim: its autograd node exposes the forward's handle, which the statistics need)
            color, feat, radii = GaussianRasterizer(GaussianRasterizationSettings(**kw))(
                means3D=leaves["means3D"], means2D=m2, opacities=leaves["opacities"], shs=leaves["shs"],
                language_feature_precomp=leaves.get("language_feature"), scales=leaves["scales"], rotations=leaves["rotations"])
            torch.cuda.synchronize()
            counts = [ctypes.c_int64(0) for _ in range(3)]
            _lib.check(_lib.lib().mgs_forward_stats(ctypes.byref(color.grad_fn.num_rendered.a), 0, *map(ctypes.byref, counts), None),
                       "mgs_forward_stats")
            loss = (color * dC.to(dev)).sum() + ((feat * dF.to(dev)).sum() if F > 0 else 0.0)
            loss.backward()
        torch.cuda.synchronize()
        grads = {k: v.grad.detach().cpu() for k, v in leaves.items()}
        grads["means2D"] = m2.grad.detach().cpu()
        return color.detach().cpu(), feat.detach().cpu(), radii.cpu(), grads, tuple(int(c.value) for c in counts)
    finally:
        _lib.set_option("dbg", old)


def _check(args, F, reach=None):
    sc, cam, kw, dC, dF = rc.stack_scene(F=F, **args)
    c_ref, f_ref, r_ref, g_ref, state = util.run_oracle_b(sc, kw, dC, dF)
    m = rc.chunk_model(state)
    if reach is not None:
        assert reach(m), (m.n, m.block_vis)
    lazy = _forward_backward(sc, cam, dC, dF, F, 0)
    eager = _forward_backward(sc, cam, dC, dF, F, EAGER)
    print(f"model: blocks visit {sorted(set(m.block_vis.values()))} chunks, margin {m.margin:.3g} (blocks {m.block_margin:.3g}); "
          f"stats lazy {lazy[4]} eager {eager[4]} model {(m.incidences, m.chunks, m.pixel_chunks)}")
    # the two forms: bit-equal in everything the forward hands out
    assert torch.equal(lazy[0], eager[0]) and torch.equal(lazy[1], eager[1]), "images differ between the two forms"
    assert torch.equal(lazy[2], eager[2]) and lazy[4] == eager[4], "radii or the state's counts differ between the two forms"
    # ... and what the model says the scene reaches is what the GPU did
    if m.block_margin > ROBUST:
        assert lazy[4][:2] == (m.incidences, m.chunks), (lazy[4], m.incidences, m.chunks)
    if m.margin > ROBUST:
        assert lazy[4][2] == m.pixel_chunks, (lazy[4], m.pixel_chunks)
    # both are the reference's render (the existing Oracle-B comparison and tolerances)
    for got in (lazy, eager):
        assert (got[2] == r_ref).all(), "radii"
        for img, ref in ((got[0], c_ref), (got[1], f_ref)) if F > 0 else ((got[0], c_ref),):
            robust, fragile, frac = util.image_errors(img, ref, state)
            assert robust < 1e-4 and fragile < util.FRAGILE_TOL and frac < util.FRAGILE_MAX_FRACTION, (robust, fragile, frac)
        errs, _ = util.grad_errors_split(got[3], g_ref, state)
        for k, (rob, fra, mag) in errs.items():
            assert rob <= 1e-3 * mag + 1e-7 and fra <= util.FRAGILE_GRAD_TOL * mag + 1e-7, (k, rob, fra, mag)
    # gradients of the two forms: the same state, another order of the float atomics (the bound between backward forms)
    for k in lazy[3]:
        a, b = lazy[3][k], eager[3][k]
        assert (a - b).abs().max().item() <= 1e-5 * b.abs().max().item() + 1e-12, k
    return m


@pytest.mark.parametrize("F", [32, 3])
@pytest.mark.parametrize("name", list(CASES))
def test_second_slot_is_evaluated_only_as_far_as_a_pixel_reaches_it(name, F):
    args, reach = CASES[name]
    m = _check(args, F, reach)
    assert m.block_margin > ROBUST and m.margin > ROBUST, "the scene was chosen away from every decision: its counts bind the GPU"


@pytest.mark.parametrize("F", [32, 3])
@pytest.mark.parametrize("pick", [np.min, np.max], ids=["least_transparent_pixel", "most_transparent_pixel"])
def test_a_pixel_within_a_few_ulps_of_the_threshold_entering_chunk_8(pick, F):
    """(g) Two neighbouring opacities: the chosen pixel enters chunk 8 with a transmittance a few ulps above 1e-4 with one and a
    few ulps below with the other (CPU model; which side the GPU's own product lands on is its business -- both forms form
    it with the same arithmetic, so they must still agree bit for bit).  The least transparent pixel: one pixel's own
    decision, every block still needs its second slot.  The most transparent pixel: the workgroup's decision itself -- with
    the higher opacity no pixel of any block reaches chunk 8 and the slot is skipped, with the lower one a single pixel does."""
    lo, hi = _near_threshold_opacities(pick)
    sides = []
    for o in (lo, hi):
        m = _check(dict(n=1100, opacity=o), F)
        e = m.enter[0][NP16]
        ulps = int(pick(e).view(np.int32)) - int(np.float32(rc.T_STOP).view(np.int32))
        # (one ulp of the opacity moves the product of 512 factors by 512 ulp(o) / (1 - o) ~ 1e-6 of it, about 14 ulps of a
        #  float next to 1e-4: the bracket is that wide, and each side lies within it -- twice that as the bound)
        assert abs(ulps) <= 32, ulps
        sides.append(ulps >= 0)
    assert sides == [True, False]


@pytest.mark.parametrize("F", [32, 3])
def test_eight_wave_form_whose_second_slot_starts_at_chunk_4(F):
    """(h) 144 x 128: 288 blocks, more than the 256 up to which a block gets 16 waves."""
    m = _check(WIDE, F, lambda m: len(m.block_vis) == 288 and set(m.block_vis.values()) == {6, 7})
    assert m.block_margin > ROBUST


def test_skip_path_replays_bit_identically_from_a_captured_graph():
    """(a) under graph capture (tests/tools/reachable_chunks_graph_check.py, in a process of its own: stream capture is
    process-wide state): the replayed forward + backward reproduces the eager images bit for bit."""
    run_graph_tool("reachable_chunks_graph_check.py", limit=170)
