"""A stand-in for the `torch` module inside manigaussian_amd._C and manigaussian_amd.views that decides what the rasterizer's
workspaces and results hold BEFORE the kernels run (tests/test_rasterizer_dirty_workspace.py; modelled on _GuardedTorch of
tests/test_gpu_parity.py).  It is installed with monkeypatch.setattr on those two modules only, under _C.use_compiled(False): the
ctypes shim's allocations can be intercepted, the compiled binding's cannot (the interleaving test of the GPU file covers that
binding through the caching allocator's own reuse).  Nothing here touches a conftest.py, a pytest setting or tests/poison.py's
global patch.

The fills of a uint8 allocation (the arena [geom | img | binning], or the three workspaces under _SPLIT_WORKSPACES, or the second
binning workspace of the capacity retry):

  zeros        0x00 everywhere: the baseline run Z.
  donor        a byte copy of what a DONOR CALL (forward + backward, synchronised: snapshot()) left in its k-th uint8 allocation.
               Used only when the donor call had the same shape key and its k-th allocation has the same byte count: the layout
               of a workspace is a function of its byte count and the problem shape alone (csrc/mgs_common.h), so every stale
               word is then a valid word of its own kind -- a key that names a Gaussian of this shape, an offset inside this
               list, a count within this capacity.  Otherwise the fill is zeros; `fills` says which was used, and the tests
               assert it.
  donor + poison   the donor bytes, with every FLOAT region of the library's region map (mgs_debug_workspace_regions, DESIGN.md
               8b) overwritten with 0xFF bytes (float32 NaN) or 0x7F bytes (3.3962e38).

INDEX regions never get 0xFF or 0x7F: their words become addresses, loop bounds, LDS indices and sort buckets, and on a machine
that others share a stale read there must show as a WRONG VALUE under the donor fill, never as an out-of-bounds access.

Results: every float32 / int32 `empty` (the images, radii, the backward's flat gradient buffer on the prezeroed and on the
non-prezeroed path) is filled with 0xFF or 0x7F bytes when `results` is set.

The wrapper around _C._forward keeps the ForwardHandle of every forward: its MgsRasterArgs (the final one: the capacity retry
swaps the binning workspace in it) is what the region map is asked for, and its pointers say which allocation holds which region."""
import ctypes

import torch

from manigaussian_amd import _lib

FLOAT, INDEX = _lib.REGION_FLOAT, _lib.REGION_INDEX


class Donor:
    """What a donor call left behind: its shape key, clones of its uint8 allocations in order, and the FLOAT byte ranges of each."""

    def __init__(self, key, arenas, float_ranges, regions):
        self.key, self.arenas, self.float_ranges, self.regions = key, arenas, float_ranges, regions


class DirtyTorch:
    def __init__(self):
        self.forward = None        # the real _C._forward (install())
        self.begin(None)

    def __getattr__(self, name):
        return getattr(torch, name)

    # ---- installation ------------------------------------------------------------------------------------------------------
    def install(self, monkeypatch):
        from manigaussian_amd import _C, views
        self.forward = _C._forward
        monkeypatch.setattr(_C, "torch", self)
        monkeypatch.setattr(views, "torch", self)
        monkeypatch.setattr(_C, "_forward", self._forward)
        return self

    def _forward(self, *args, **kw):
        out = self.forward(*args, **kw)
        self.handles.append(out[0])
        return out

    # ---- one call ----------------------------------------------------------------------------------------------------------
    def begin(self, key, arena="zeros", donor=None, poison=None, results=None):
        """The next call's fills.  key: the call's shape key; arena: "zeros" | "donor"; poison: None, 0xFF or 0x7F over the
        donor's FLOAT regions; results: None, 0xFF or 0x7F over every float32 / int32 empty."""
        assert arena in ("zeros", "donor") and (arena == "donor") == (donor is not None)
        assert poison in (None, 0xFF, 0x7F) and results in (None, 0xFF, 0x7F) and (poison is None or donor is not None)
        self.key, self.arena, self.donor, self.poison, self.results = key, arena, donor, poison, results
        self.u8 = []               # this call's uint8 allocations, in order
        self.fills = []            # ... and the fill each one got: "zeros" | "donor"
        self.poisoned_bytes = 0    # bytes of FLOAT regions overwritten with the poison
        self.results_filled = 0    # float32 / int32 allocations filled
        self.results_seen = 0      # ... of how many
        self.handles = []

    def empty(self, size, *a, **kw):
        t = torch.empty(size, *a, **kw)
        dt = kw.get("dtype")
        if dt is torch.uint8:
            if t.numel() == 0:
                return t
            k = len(self.u8)
            d = self.donor
            if d is not None and d.key == self.key and k < len(d.arenas) and d.arenas[k].numel() == t.numel():
                t.copy_(d.arenas[k])
                self.fills.append("donor")
                if self.poison is not None:
                    for off, n in d.float_ranges[k]:
                        assert 0 <= off and off + n <= t.numel()
                        t[off:off + n] = self.poison
                        self.poisoned_bytes += n
            else:
                t.zero_()
                self.fills.append("zeros")
            self.u8.append(t)
        elif dt in (torch.float32, torch.int32) and t.numel():
            self.results_seen += 1
            if self.results is not None:
                t.view(torch.uint8).fill_(self.results)
                self.results_filled += 1
        return t

    # ---- after the call ----------------------------------------------------------------------------------------------------
    def handle(self):
        """The ForwardHandle of the call's (last) forward."""
        assert self.handles and not isinstance(self.handles[-1], int), "the call ran no forward through the ctypes shim"
        return self.handles[-1]

    def shape_of(self, h):
        a = h.a
        V = h.views[1] if h.views is not None else 0
        S = h.sets[0] if h.sets is not None else 0
        return (int(a.P), int(a.M), int(a.F) if a.include_feature else 0, int(a.W), int(a.H), V, S)

    def regions(self):
        """[(region name, kind, index of the uint8 allocation that holds it, byte offset inside it, bytes)] of the call's final
        workspaces, aliases (direct keys inside the two key arrays) left out.  The allocations are found by address."""
        h = self.handle()
        a = h.a
        V = h.views[1] if h.views is not None else 0
        base = {"geom": int(a.geom), "img": int(a.img), "binning": int(a.binning)}
        size = {"geom": int(a.geom_bytes), "img": int(a.img_bytes), "binning": int(a.binning_bytes)}
        where = {}
        for ws, p in base.items():
            hit = [k for k, t in enumerate(self.u8) if t.data_ptr() <= p and p + size[ws] <= t.data_ptr() + t.numel()]
            assert len(hit) == 1, (ws, hit)
            where[ws] = (hit[0], p - self.u8[hit[0]].data_ptr())
        out = []
        for ws, name, off, n, kind, alias in _lib.workspace_regions(a, V):
            if alias:
                continue
            assert off + n <= size[ws], (ws, name)
            out.append((name, kind, where[ws][0], where[ws][1] + off, n))
        return out

    def region(self, name):
        """The bytes of one region of the call's final workspaces, as a view of its allocation."""
        for nm, kind, k, off, n in self.regions():
            if nm == name:
                return self.u8[k][off:off + n]
        raise KeyError(name)

    def snapshot(self):
        """The call as a donor (after torch.cuda.synchronize())."""
        assert self.key is not None and self.shape_of(self.handle()) == tuple(self.key[:7]), (self.key, self.shape_of(self.handle()))
        regs = self.regions()
        ranges = [[(off, n) for _, kind, k, off, n in regs if k == i and kind == FLOAT] for i in range(len(self.u8))]
        return Donor(self.key, [t.clone() for t in self.u8], ranges, regs)


def raster_args(P, M, F, W, H, V=0, named=True, budget=1 << 40, capacity=None, pool=0):
    """A forward's MgsRasterArgs as _C._forward fills the fields the region map reads, without a device: the worst-case arena of
    the shape (capacity None), or `capacity` / `pool`; named = the capacity travels in the struct (else the library derives the
    carving from the binning workspace's byte count, as for the raw pair)."""
    a = _lib.MgsRasterArgs()
    a.P, a.D, a.M, a.F, a.W, a.H, a.include_feature = P, 1, M, F, W, H, int(F > 0)
    gb, ib, fits, cap_worst, pool_worst, _ = _lib.plan_arena(P, M, F, W, H, V, budget)
    cap, pl = (cap_worst, pool_worst) if capacity is None else (capacity, pool)
    a.geom_bytes, a.img_bytes = gb, ib
    a.binning_bytes = _lib.plan_binning_bytes(P, F, W, H, V, cap, pl, bool(named and cap != cap_worst))
    if named:
        a.binning_capacity, a.chunk_pool = cap, pl
    a.binning = ctypes.c_void_p(256)  # (never read: mgs_debug_direct_keys answers "none" for a NULL workspace)
    return a, gb, ib
