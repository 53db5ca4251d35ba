"""mgs_debug_workspace_regions: the region map of the rasterizer's three workspaces, on the shapes that
tests/test_rasterizer_dirty_workspace.py dirties.  Host code only: no device, no pointer is read.

The map is what decides which bytes a test may poison (FLOAT) and which it may only replace by words of the same layout (INDEX),
so it has to BE the carving: every region inside its workspace, in carving order, disjoint, with nothing but alignment between
them, ending where the workspace plan says the workspace ends, and in agreement with the three older debug calls."""
import ctypes

import pytest

import dirty_workspace as dw
from manigaussian_amd import _lib

ALIGN = 256
# (P, M, F as the library sees it, W, H, V): the cases of the GPU file -- partial_blocks_17x33_f64, padded_width_f5 (F padded to 8),
# black_background_posfocal_f32, translucent_long_lists_f3, the batch 3_views_f3_72x40, the two-set batch (2 views of 2000)
SHAPES = {
    "partial_blocks_17x33_f64": (70, 4, 64, 17, 33, 0),
    "padded_width_f5": (2000, 4, 8, 64, 64, 0),
    "black_background_posfocal_f32": (1200, 4, 32, 48, 48, 0),
    "translucent_long_lists_f3": (30000, 4, 3, 32, 32, 0),
    "3_views_f3_72x40": (3000, 4, 3, 72, 40, 3),
    "two_sets_f3_64": (2000, 4, 3, 64, 64, 2),
    "no_feature_precomp": (1000, 0, 0, 64, 64, 0),
}
# how the binning workspace is sized: the worst case of the default forward mode; a capacity and pool from the marks, named in the
# struct (with the room for the direct keys behind the carved arrays); the same bytes unnamed (the raw pair: the library derives the
# carving from the byte count -- single views only, a batch always names its capacity)
SIZINGS = ("worst_named", "marks_named", "marks_unnamed", "worst_unnamed")

GEOM = ["depths", "rec", "rect", "rgb", "cov3D", "clamped", "blk_base"]
IMG = ["final_T", "ranges", "tables", "ready", "cursor"]
BINNING = ["keys_unsorted", "keys", "point_list", "seg_desc", "round_base", "last_chunk", "nsurv", "surv", "T_end", "T_mid", "last_pos",
           "q", "partial"]
FLOAT_REGIONS = {"rgb", "cov3D", "final_T", "T_end", "T_mid", "q", "partial"}


def _args(shape, sizing):
    P, M, F, W, H, V = shape
    if sizing.startswith("worst"):
        return dw.raster_args(P, M, F, W, H, V, named=sizing.endswith("_named"))
    cap, pool = _lib.plan_capacity(_lib.SIZE_HEADROOM, P, V, 3 * P + 17, 301, 1.5, 1.5)   # counts as marks hold them: arbitrary, odd
    named = sizing.endswith("_named")   # (a byte count alone says nothing about a pool: unnamed means the worst-case pool)
    return dw.raster_args(P, M, F, W, H, V, named=named, capacity=cap, pool=pool if named else 0)


CASES = [(n, s) for n in SHAPES for s in SIZINGS if not (SHAPES[n][5] and s.endswith("unnamed"))]


@pytest.mark.parametrize("name,sizing", CASES, ids=[f"{n}-{s}" for n, s in CASES])
def test_regions_are_the_carving(name, sizing):
    shape = SHAPES[name]
    P, M, F, W, H, V = shape
    a, gb, ib = _args(shape, sizing)
    regs = _lib.workspace_regions(a, V)
    total = {"geom": gb, "img": ib, "binning": int(a.binning_bytes)}
    by_ws = {ws: [r for r in regs if r[0] == ws and not r[5]] for ws in total}
    carved = [r[1] for r in by_ws["binning"] if r[1] != "direct_keys"]
    assert [r[1] for r in by_ws["geom"]] == GEOM and [r[1] for r in by_ws["img"]] == IMG and carved == BINNING
    assert {r[1] for r in regs if r[4] == _lib.REGION_FLOAT} == FLOAT_REGIONS        # everything else, direct keys included: INDEX
    for ws, rs in by_ws.items():
        end = 0
        for _, nm, off, n, kind, alias in rs:
            assert n > 0 and off % ALIGN == 0, (ws, nm)
            assert off >= end, f"{ws}.{nm} overlaps the region before it or is out of carving order"
            # (the room for the direct keys lies behind the carved arrays' own trailing ALIGN)
            gap = off - end - (ALIGN if nm == "direct_keys" else 0)
            assert 0 <= gap < ALIGN, f"{ws}.{nm}: a gap of {off - end} bytes is more than alignment"
            end = off + n
        # ... and the workspace ends where the plan says: the last region, rounded up, plus the trailing ALIGN
        tail = total[ws] - (end + ALIGN - 1) // ALIGN * ALIGN
        if ws == "binning" and sizing == "marks_named" and by_ws[ws][-1][1] != "direct_keys":
            # (the plan grants the room for the direct keys whenever the capacity is named below the worst case; where the two key
            #  arrays already hold T x P keys the preprocess writes them there and the room stays unused: nobody reads or writes it)
            assert tail == ALIGN + _lib.lib().mgs_binning_direct_extra(P, V, W, H) > 2 * ALIGN, (ws, end, total[ws])
        elif rs[-1][1] == "direct_keys":   # (T x P keys, not rounded up, and the room's own 256 bytes)
            assert total[ws] - end == ALIGN, (ws, end, total[ws])
        else:
            assert tail == ALIGN, (ws, end, total[ws])
    # sizes the kernels' host code takes for granted
    size = {r[1]: r[3] for r in regs}
    Pv, T = P * max(V, 1), ((W + 15) // 16) * ((H + 15) // 16) * max(V, 1)
    assert size["depths"] == 4 * Pv and size["rec"] == 32 * Pv and size["rect"] == 8 * Pv and size["cov3D"] == 24 * Pv
    assert size["ranges"] == 8 * T and size["last_chunk"] == 4 * 256 * T and size["nsurv"] == 8 * 4 * T
    assert size["T_end"] == size["T_mid"] == size["last_pos"] == size["q"] and size["partial"] == size["q"] * (3 + F)
    assert size["surv"] == 4 * size["point_list"] and size["keys"] == size["keys_unsorted"] == 2 * size["point_list"]

    # the three older debug calls
    L = _lib.lib()
    ku, pl, rg, cap = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_int32()
    _lib.check(L.mgs_debug_binning_layout(ctypes.byref(a), V, ctypes.byref(ku), ctypes.byref(pl), ctypes.byref(rg), ctypes.byref(cap)),
               "binning_layout")
    off = {(r[0], r[1]): r[2] for r in regs}
    assert (off["binning", "keys_unsorted"], off["binning", "point_list"], off["img", "ranges"]) == (ku.value, pl.value, rg.value)
    assert size["point_list"] == 4 * max(cap.value, 1)
    if a.binning_capacity:
        assert cap.value == a.binning_capacity
    dk, stride = ctypes.c_size_t(), ctypes.c_int32()
    _lib.check(L.mgs_debug_direct_keys(ctypes.byref(a), V, ctypes.byref(dk), ctypes.byref(stride)), "direct_keys")
    direct = [r for r in regs if r[1] == "direct_keys"]
    if stride.value:
        assert len(direct) == 1 and direct[0] is regs[-1]
        _, _, doff, dn, dkind, dalias = direct[0]
        assert doff == dk.value and dn == 8 * T * P and dkind == _lib.REGION_INDEX
        # inside the two key arrays (an alias), or behind everything carved
        assert dalias == (1 if doff == off["binning", "keys_unsorted"] else 0)
        if dalias:
            assert doff + dn <= off["binning", "point_list"]
        else:
            assert doff >= off["binning", "partial"] + size["partial"] and doff + dn + ALIGN == total["binning"]
    else:
        assert not direct
    if not V:
        d, r, c, v = (ctypes.c_size_t() for _ in range(4))
        _lib.check(L.mgs_debug_geom_layout(P, M, W, H, ctypes.byref(d), ctypes.byref(r), ctypes.byref(c), ctypes.byref(v)), "geom_layout")
        assert (off["geom", "depths"], off["geom", "rec"], off["geom", "rgb"], off["geom", "cov3D"]) == (d.value, r.value, c.value, v.value)


def test_the_direct_keys_follow_the_options_and_the_sizing():
    """The worst-case workspace holds the direct keys inside its two key arrays; a workspace sized from the marks gets room behind
    the carved arrays; dbg = 32768 (the scatter launch) and bin_mode 1 / 0 have none."""
    P, M, F, W, H, V = SHAPES["padded_width_f5"]
    a, _, _ = _args(SHAPES["padded_width_f5"], "worst_named")
    assert _lib.workspace_regions(a)[-1][1:] == ("direct_keys", 0, 8 * 16 * P, _lib.REGION_INDEX, 1)
    b, _, _ = _args(SHAPES["padded_width_f5"], "marks_named")
    last = _lib.workspace_regions(b)[-1]
    assert last[1] == "direct_keys" and last[5] == 0
    for opt in (dict(dbg=32768), dict(bin_mode=1), dict(bin_mode=0)):
        _lib.fill_options(a, dict(_lib.DEFAULT_OPTIONS, **opt))
        assert _lib.workspace_regions(a)[-1][1] == "partial", opt


def test_bad_arguments_and_the_counting_call():
    L = _lib.lib()
    a, _, _ = _args(SHAPES["padded_width_f5"], "worst_named")
    n = ctypes.c_int32(-1)
    assert L.mgs_debug_workspace_regions(ctypes.byref(a), 0, None, 0, ctypes.byref(n)) == _lib.MGS_OK and n.value == 26
    out = (_lib.MgsWorkspaceRegion * 4)()
    assert L.mgs_debug_workspace_regions(ctypes.byref(a), 0, out, 4, ctypes.byref(n)) == _lib.MGS_ERR_INVALID_ARG and n.value == 26
    assert [r.name.decode() for r in out] == ["depths", "rec", "rect", "rgb"]
    assert L.mgs_debug_workspace_regions(ctypes.byref(a), 0, out, 4, None) == _lib.MGS_ERR_INVALID_ARG
    assert L.mgs_debug_workspace_regions(ctypes.byref(a), 17, out, 4, ctypes.byref(n)) == _lib.MGS_ERR_INVALID_ARG
    a.binning_bytes = 1024
    a.binning_capacity = 0
    assert L.mgs_debug_workspace_regions(ctypes.byref(a), 0, out, 4, ctypes.byref(n)) == _lib.MGS_ERR_WORKSPACE
