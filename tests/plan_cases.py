"""The workspace plan (include/mgsplat.h, "the workspace plan"; csrc/mgs_plan.hip) restated in plain Python over the library's
PRIMITIVE size queries, and the grid of cases tests/test_plan.py walks.  This file is the written specification: every formula
below is what the two host bindings computed by hand before the plan moved into the library, and agreed with those helpers over
the whole grid when it did.  L: the ctypes library (manigaussian_amd._lib.lib())."""
import itertools

PS = (1, 1000, 16384, 100000, 500000, 2000000)
SIZES = ((16, 16), (128, 128), (256, 256), (1024, 1024), (1040, 1024), (1920, 1080))  # 4096 tiles exactly; above LDS_TILES
FS = (0, 3, 32, 64)
VS = (0, 1, 4, 16)
BUDGETS = (0, 1 << 30, 9 << 30)
M = 4
HEADROOMS = (1.0, 1.5, 2.0)
# (P, M, F, V, colours precomputed, S) -> (total floats, accum_bytes) of the backward's allocation
GRADIENTS = {(1000, 4, 8, 3, False, 2): (140068, 292256), (1000, 0, 8, 3, True, 2): (113068, 280256),
             (16384, 4, 3, 0, False, 0): (884804, 1442048), (100000, 16, 32, 4, False, 0): (18500068, 43200256),
             (5, 0, 0, 1, True, 0): (311, 832)}


def shapes():
    """(P, W, H, F, V) over the grid"""
    return [(P, W, H, F, V) for P, (W, H), F, V in itertools.product(PS, SIZES, FS, VS)]


def up256(n):
    return (n + 255) & ~255


def tiles(W, H, V):
    return max(V, 1) * ((W + 15) // 16) * ((H + 15) // 16)  # the tiles binned: those of every view


def arena(L, P, M, W, H, V):
    g, i = (L.mgs_views_geom_bytes(P, M, W, H, V), L.mgs_views_img_bytes(W, H, V)) if V else \
        (L.mgs_geom_bytes(P, M, W, H), L.mgs_img_bytes(W, H))
    return up256(g), up256(i)


def binning_bytes(L, cap, pool, W, H, F, V, P_direct=0):
    """P_direct > 0: plus the direct-key room where the library offers it"""
    v = L.mgs_views_binning_bytes2(cap, pool, W, H, F, V) if V else L.mgs_binning_bytes2(cap, pool, W, H, F)
    extra = L.mgs_binning_direct_extra(P_direct, V, W, H) if P_direct > 0 else 0
    return up256(v) + extra if extra else v


def worst_case(L, P, W, H, F, V, budget):
    """(fits, capacity, chunk pool, bytes): every Gaussian in every tile"""
    cap = P * tiles(W, H, V)
    nbytes = binning_bytes(L, cap, 0, W, H, F, V) if cap < (1 << 30) else 0
    ok = 0 < nbytes <= budget
    pool = 0 if not ok else L.mgs_views_chunk_pool_max(cap, W, H, V) if V else L.mgs_chunk_pool_max(cap, W, H)
    return ok, cap, pool, nbytes


def capacity_headroom(R, chunks, head_instances, head_chunks):
    return int(R * head_instances) + 4096, int(chunks * head_chunks) + 64  # (truncated, not rounded)


def capacity_count(R, P, V):
    """R: a mark or a reported count; None: nothing known"""
    return (R + R // 4 + 4096 if R is not None else 4 * max(V, 1) * P + 4096), 0


def options(seg, bin_mode, R, T):
    seg2 = 4096 if seg == 2048 and R and R > 8192 * T else seg
    if bin_mode == 2 and R and R > 24576 * T:
        return seg2, 1
    return seg2, bin_mode


def gradients(L, P, M, F, V, precomp, S):
    """(float offsets of [scratch | colors | feature | means3D | opacity | sh | scales | rotations | cov3D | means2D | pad],
    total, accum_bytes)"""
    scratch = L.mgs_sets_backward_scratch_bytes(P, M, F, V, S) if S else \
        L.mgs_views_backward_scratch_bytes(P, M, F, V) if V else L.mgs_backward_scratch_bytes(P, M, F)
    scratch_f = (scratch + 3) // 4
    n, G = max(V, 1) * P, max(S, 1) * P  # (view, Gaussian) pairs, (set, Gaussian) rows
    ncol = G if precomp else n
    sizes = [scratch_f, 3 * ncol, F * G, 3 * G, G, 3 * M * G, 3 * G, 4 * G, 6 * G, 3 * n, 4]
    offs = tuple(itertools.accumulate([0] + sizes[:-1]))
    return offs, sum(sizes), ((scratch_f + 3 * ncol + F * G) * 4 + 15) // 16 * 16
