"""The rasterizer's results do not depend on what its workspaces and result tensors held before the call.

Every forward carves [geom | img | binning] out of one torch.empty arena and the backward's flat gradient buffer is torch.empty
too: the caching allocator hands back whatever an earlier call left there.  About twenty regions are carved, several of them
written only in part and by design (DESIGN.md 8b holds the table: region, kind, first writer, first reader, what part is written).
Here the stand-in allocator of tests/dirty_workspace.py decides what those bytes are:

  Z        everything 0x00: the baseline, gated against the float64 truth of tests/gradient_truth.py with the project's own gates;
  donor    the arena is a byte copy of what a donor call -- forward + backward of an EDIT of the test scene with the same shape --
           left in its arena: denser (more instances per tile, more rounds and chunk records, longer survivor prefixes), sparser
           (half the Gaussians behind the cameras), empty (all of them: no instance at all) and rolled (the same Gaussians under
           other ids: equal counts everywhere);
  donor + 0xFF / 0x7F   the same with every FLOAT region of the library's region map overwritten (float32 NaN / 3.3962e38);
  results 0xFF / 0x7F   every float32 / int32 torch.empty -- images, radii, the gradient buffer -- filled.

INDEX regions (keys, offsets, counts, ids, flags: everything a kernel turns into an address, a loop bound, an LDS index or a sort
bucket) only ever hold zeros or a donor's words of the same layout: a stale read there shows as a wrong value, never as an
out-of-bounds access.  No fill puts another pattern there.

Every dirty run must equal Z bit for bit in colour, feature, radii, the reference's instance count and the binned count, lie within
2e-5 max|g_Z| + 1e-12 of Z in every gradient tensor (the project's bound for the order of float atomics, tests/test_gpu_parity.py),
pass the same truth gates, and have no non-finite element where Z's is finite; the stand-in's counters must show that the arena
and every result were actually filled.

The stand-in intercepts the ctypes shim (_C.use_compiled(False)).  The compiled binding allocates in C++: its allocations are
covered by the interleaving test alone, where the caching allocator's own reuse across three shapes is the dirt."""
import contextlib
import warnings

import numpy as np
import pytest
import torch

import dirty_workspace as dw
import gradient_truth as gt
import util
from manigaussian_amd import _lib
from manigaussian_amd import synthetic as syn

gpu = pytest.mark.gpu
pytestmark = gpu
BOUND = 2e-5          # float atomics: the order differs from run to run (tests/test_gpu_parity.py)
POISONS = (0xFF, 0x7F)
POISON_WORDS = (0xFFFFFFFF, 0x7F7F7F7F)


def _need_gpu():
    from test_gradient_truth import _need_gpu as need
    need()
    return torch.device("cuda:0")


# ---- the donors: edits of a Gaussian set that keep P and every shape -------------------------------------------------------
def _behind(sc, rows):
    """Rows of the set moved behind every camera of syn.circle_cameras (they look down at the scene from z = target + 0.9: a point
    1000 above it has a negative view-space z for all of them, the near cull drops it)."""
    m = sc["means3D"].clone()
    m[rows, 2] += 1000.0
    return m


DONORS = {
    "denser": lambda sc: dict(sc, scales=(sc["scales"] * 3.0).contiguous()),
    "sparser": lambda sc: dict(sc, scales=(sc["scales"] * 0.3).contiguous(), means3D=_behind(sc, slice(0, None, 2))),
    "empty": lambda sc: dict(sc, means3D=_behind(sc, slice(None))),
    "rolled": lambda sc: {k: torch.roll(v, 1, 0).contiguous() for k, v in sc.items()},
}


# ---- the scenes ------------------------------------------------------------------------------------------------------------
class Single:
    """A case of gradient_truth.CASES: (sc, cam, kw, dC, dF)."""

    def __init__(self, name, s=None):
        self.name = name
        self.s = s if s is not None else gt.case_truth(name)[0]

    def truth(self):
        return gt.case_truth(self.name)[1]

    def edited(self, edit):
        sc, cam, kw, dC, dF = self.s
        return Single(self.name, (edit(sc), cam, kw, dC, dF))

    def key(self):
        from manigaussian_amd import _C
        sc, cam, kw, dC, dF = self.s
        P, inc = sc["means3D"].shape[0], bool(kw["include_feature"])
        F = _C._padded_F(sc["language_feature"].shape[1]) if inc else 0
        return (P, sc["shs"].shape[1] if "shs" in sc else 0, F, kw["image_width"], kw["image_height"], 0, 0)

    def run(self, raw=False):
        sc, cam, kw, dC, dF = self.s
        inc = bool(kw["include_feature"])
        if raw:
            return _raw_pair(self.s)
        return util.run_hip(sc, cam, dC, dF, kw["sh_degree"], inc, tuple(kw["bg"].tolist()), scale_modifier=kw["scale_modifier"])

    def gate(self, tag, out):
        from test_gradient_truth import _gate_scene
        _gate_scene(tag, self.s, self.truth(), out, few=None)


class Batch:
    """A batch of gradient_truth.VIEW_BATCHES: (sc, cams, dC, dF) through GaussianRasterizerBatch."""

    def __init__(self, name, s=None):
        self.name = name
        self.s = s if s is not None else gt.batch_truth(name)[0]

    def truth(self):
        return gt.batch_truth(self.name)[1]

    def edited(self, edit):
        sc, cams, dC, dF = self.s
        return Batch(self.name, (edit(sc), cams, dC, dF))

    def key(self):
        sc, cams, dC, dF = self.s
        return (sc["means3D"].shape[0], sc["shs"].shape[1], dF.shape[1], dC.shape[-1], dC.shape[-2], len(cams), 0)

    def run(self, raw=False):
        from test_gpu_parity import _run_batch
        sc, cams, dC, dF = self.s
        cb, fb, rb, g, m2 = _run_batch(sc, cams, dC, dF, gt.BG)
        return cb, fb, rb, dict(g, means2D=m2)

    def gate(self, tag, out):
        """The gates of test_gradient_truth.test_view_batch_per_gaussian_against_the_float64_truth."""
        cb, fb, rb, g = out
        T0 = self.truth()
        assert torch.equal(rb, T0.radii), "radii differ"
        T = gt.follow(T0, cb, fb)
        V = cb.shape[0]
        for v in range(V):
            gt.gate_image(f"{tag}/view{v}", "color", cb[v], T.images["color"][v], T.fragile_px[v], T.image_yard["color"])
            gt.gate_image(f"{tag}/view{v}", "feature", fb[v], T.images["feature"][v], T.fragile_px[v], T.image_yard["feature"])
        got = {util.GRAD_KEYS[k]: v for k, v in g.items() if k != "means2D"}
        got.update({f"means2D[{v}]": g["means2D"][v] for v in range(V)})
        assert set(got) == set(T.yard), (sorted(got), sorted(T.yard))
        gt.gate_gradients(tag, T, got)


class Sets:
    """The two-set batch of test_gradient_truth.test_set_batch_per_gaussian_against_the_float64_truth (two different sets of 2000,
    one view each, through render_sets_stacked): held to Z only."""
    P, F, W = 2000, 3, 64

    def __init__(self, name="two_sets_f3_64", scs=None):
        self.name = name
        self.scs = scs if scs is not None else [syn.make_scene(self.P, F=self.F, M=4, seed=11 + v) for v in range(2)]
        cams = syn.circle_cameras(4, self.W, self.W, negative_focal=True)
        self.views = [cams[0], cams[2]]
        g = torch.Generator().manual_seed(8)
        self.dC, self.dF = torch.randn(2, 3, self.W, self.W, generator=g), torch.randn(2, self.F, self.W, self.W, generator=g)

    def edited(self, edit):
        return Sets(self.name, [edit(sc) for sc in self.scs])

    def key(self):
        return (self.P, 4, self.F, self.W, self.W, 2, 2)

    def run(self, raw=False):
        from manigaussian_amd.gaussian_renderer import render_sets_stacked
        dev, W = torch.device("cuda:0"), self.W

        def data_of(cam):
            kw = syn.camera_settings_kwargs(cam, 1, True, device=dev)
            return {"novel_view": {"tanfov_host": [(kw["tanfovx"], kw["tanfovy"])], "size_host": [(W, W)],
                                   "world_view_transform": kw["viewmatrix"][None], "full_proj_transform": kw["projmatrix"][None],
                                   "camera_center": kw["campos"][None]}}

        leaves = [{k: v.to(dev).clone().requires_grad_(True) for k, v in sc.items()} for sc in self.scs]
        items = [(data_of(cam), 0, lv["means3D"], lv["rotations"], lv["scales"], lv["opacities"], None, lv["shs"],
                  lv["language_feature"]) for cam, lv in zip(self.views, leaves)]
        outs, batch = render_sets_stacked(items, gt.BG)
        torch.autograd.backward([batch["render"], batch["render_embed"]], [self.dC.to(dev), self.dF.to(dev)])
        torch.cuda.synchronize()
        g = {f"{k}[{s}]": t.grad.cpu() for s, lv in enumerate(leaves) for k, t in lv.items()}
        g["means2D"] = batch["viewspace_points"].grad.cpu()
        return batch["render"].detach().cpu(), batch["render_embed"].detach().cpu(), batch["radii"].cpu(), g

    def gate(self, tag, out):
        pass


def _raw_pair(s):
    """The reference-shaped pair _C.rasterize_gaussians -> _C.rasterize_gaussians_backward(R: int, the three byte buffers): the
    forward hands out no gradient buffer, the backward allocates its own and fills the accumulators (accum_prezeroed = 0)."""
    from manigaussian_amd import _C
    dev = torch.device("cuda:0")
    sc, cam, kw, dC, dF = s
    inc = bool(kw["include_feature"])
    assert inc and "shs" in sc and "scales" in sc
    d = {k: v.to(dev) for k, v in sc.items()}
    kwd = syn.camera_settings_kwargs(cam, kw["sh_degree"], inc, bg=tuple(kw["bg"].tolist()), device=dev)
    e = torch.Tensor([])
    sm = float(kw["scale_modifier"])
    R, c, f, radii, geom, binning, img = _C.rasterize_gaussians(
        kwd["bg"], d["means3D"], e, d["language_feature"], d["opacities"], d["scales"], d["rotations"], sm, e, kwd["viewmatrix"],
        kwd["projmatrix"], kwd["tanfovx"], kwd["tanfovy"], kw["image_height"], kw["image_width"], d["shs"], kw["sh_degree"],
        kwd["campos"], False, False, True)
    assert isinstance(R, int)
    if _raw_pair.between is not None:
        torch.cuda.synchronize()
        _raw_pair.between()
    out = _C.rasterize_gaussians_backward(
        kwd["bg"], d["means3D"], radii, e, d["language_feature"], d["scales"], d["rotations"], sm, e, kwd["viewmatrix"],
        kwd["projmatrix"], kwd["tanfovx"], kwd["tanfovy"], dC.to(dev), dF.to(dev), d["shs"], kw["sh_degree"], kwd["campos"], geom, R,
        binning, img, False, True)
    torch.cuda.synchronize()
    g_m2, g_col, g_feat, g_op, g_m3, g_cov, g_sh, g_sc, g_rot = out
    g = {"means3D": g_m3, "means2D": g_m2, "opacities": g_op.reshape(sc["opacities"].shape), "scales": g_sc, "rotations": g_rot,
         "shs": g_sh, "language_feature": g_feat}
    return c.cpu(), f.cpu(), radii.cpu(), {k: v.cpu() for k, v in g.items()}


_raw_pair.between = None   # the sensitivity test's hook between forward and backward


# ---- the paths -------------------------------------------------------------------------------------------------------------
OPTION_PATHS = {"scatter_launch": dict(dbg=32768), "bin_mode_1": dict(bin_mode=1), "bin_mode_0": dict(bin_mode=0),
                "table_init_1": dict(table_init=1)}
PATHS = ("default", "scatter_launch", "bin_mode_1", "bin_mode_0", "table_init_1", "blocking", "raw_pair", "marks_only",
         "capacity_retry", "split_workspaces")
TINY_MARK = 16   # a mark far below every scene: the waiting path's capacity is then 4116 instances (mgs_plan_capacity)


@contextlib.contextmanager
def _path(name, monkeypatch):
    """The settings of a path for the whole test (the per-call options are put back by conftest's fixture, everything else here)."""
    from manigaussian_amd import _C
    from test_gpu_parity import _forward_mode, _marks_only
    with contextlib.ExitStack() as es:
        es.enter_context(_C.use_compiled(False))
        for k, v in OPTION_PATHS.get(name, {}).items():
            _lib.set_option(k, v)
        if name in ("blocking", "capacity_retry"):
            es.enter_context(_forward_mode("blocking"))
        if name == "marks_only":
            es.enter_context(_marks_only())
        if name == "split_workspaces":
            monkeypatch.setattr(_C, "_SPLIT_WORKSPACES", True)
        yield


@pytest.fixture
def marks_restored():
    """The high-water marks are process-wide: what the donors raise here is put back."""
    from manigaussian_amd import _state
    st = _state.device_state(torch.device("cuda:0"))
    before = {k: st.marks[k] for k in list(st.marks)}
    yield st
    torch.cuda.synchronize()
    _state.check_status(torch.device("cuda:0"))
    for k in list(st.marks):
        if k not in before:
            del st.marks[k]
    for k, v in before.items():
        st.marks[k] = v


class Harness:
    """One (scene, path): the stand-in installed, the runs and their comparison."""

    def __init__(self, scene, path, monkeypatch, st):
        self.scene, self.path, self.st = scene, path, st
        self.dt = dw.DirtyTorch().install(monkeypatch)
        self.raw = path == "raw_pair"
        self.key = scene.key()
        P, M, F, W, H, V, S = self.key
        rest = (P, W, H, F, _lib.DEFAULT_OPTIONS["tight_bins"])
        self.mark_key = ("sets", S, V) + rest if S else ("views", V) + rest if V else rest   # _state._mark_key

    def _before_run(self):
        if self.path == "capacity_retry":     # the waiting path sizes its first pass from a mark far too small
            self.st.marks[self.mark_key] = [TINY_MARK, None]

    def run(self, scene, **fill):
        """One forward + backward of `scene` under the fills; returns (what the scene's run returned, counts, the stand-in's record)."""
        from manigaussian_amd import _state
        self._before_run()
        self.dt.begin(self.key, **fill)
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)   # an overflow repaired behind a warning is another path than the one named
            out = scene.run(raw=self.raw)
            torch.cuda.synchronize()
            h = self.dt.handle()
            counts = (int(h), h.binned())
            _state.check_status(torch.device("cuda:0"))
        assert self.dt.shape_of(h) == self.key, (self.dt.shape_of(h), self.key)
        return out, counts

    def prime(self):
        """The densest scene first, twice: the marks of the shape are then at their high-water level for every run of the test, so
        that Z, every donor and every dirty run carve workspaces of the same byte counts (a donor's bytes are used only then)."""
        if self.mark_key in self.st.marks:   # (marks an earlier test left: the first dense call must not be sized from a smaller scene)
            del self.st.marks[self.mark_key]
        dense = self.scene.edited(DONORS["denser"])
        for _ in range(2):
            self.run(dense)
        assert self.mark_key in self.st.marks, (self.mark_key, list(self.st.marks))

    def donor(self, name):
        d = self.scene.edited(DONORS[name])
        (c, f, r, g), counts = self.run(d)
        if name == "empty":
            assert counts == (0, 0) and int(r.abs().sum()) == 0, "the empty donor rendered something"
        if name == "rolled":
            assert counts == self.z_counts
        assert self.dt.fills and set(self.dt.fills) == {"zeros"}
        return self.dt.snapshot()

    def baseline(self):
        self.z, self.z_counts = self.run(self.scene)
        assert set(self.dt.fills) == {"zeros"} and self.dt.results_seen >= 3 and self.dt.results_filled == 0
        self.z_allocs = [t.numel() for t in self.dt.u8]
        print(f"  Z/{self.scene.name}/{self.path}: instances (reference, binned) {self.z_counts}, uint8 allocations {self.z_allocs}")
        self.scene.gate(f"Z/{self.scene.name}/{self.path}", self.z)
        return self.z

    def compare(self, tag, out, counts):
        c0, f0, r0, g0 = self.z
        c, f, r, g = out
        assert torch.equal(c, c0), f"{tag}: colour differs from Z in {int((c != c0).sum())} elements"
        assert torch.equal(f, f0), f"{tag}: feature differs from Z in {int((f != f0).sum())} elements"
        assert torch.equal(r, r0), f"{tag}: radii differ from Z"
        assert counts == self.z_counts, (tag, counts, self.z_counts)
        assert g.keys() == g0.keys()
        for k in g0:
            d = (g[k] - g0[k]).abs().max().item() if g0[k].numel() else 0.0
            bound = BOUND * g0[k].abs().max().item() + 1e-12
            print(f"  {tag} {k}: max |g - g_Z| {d:.3g} (bound {bound:.3g})")
            assert not bool((~torch.isfinite(g[k]) & torch.isfinite(g0[k])).any()), f"{tag} {k}: non-finite where Z is finite"
            assert d <= bound, f"{tag} {k}: {d:.3g} from Z, bound {bound:.3g}"
        for nm, t, t0 in (("color", c, c0), ("feature", f, f0)):
            assert not bool((~torch.isfinite(t) & torch.isfinite(t0)).any()), f"{tag} {nm}: non-finite where Z is finite"
        self.scene.gate(tag, out)

    def dirty(self, dname, donor):
        """Every other fill, once with this donor."""
        dt = self.dt
        fills = [("donor", dict(arena="donor", donor=donor))]
        fills += [(f"donor+{p:02X}", dict(arena="donor", donor=donor, poison=p)) for p in POISONS]
        fills += [(f"results_{p:02X}", dict(arena="zeros", results=p)) for p in POISONS]
        for fname, fill in fills:
            tag = f"{self.scene.name}/{self.path}/{dname}/{fname}"
            out, counts = self.run(self.scene, **fill)
            # what was actually filled
            if fill["arena"] == "donor":
                want = ["donor" if k < len(donor.arenas) and donor.arenas[k].numel() == t.numel() else "zeros"
                        for k, t in enumerate(dt.u8)]
                assert dt.fills == want and dt.fills[0] == "donor", (tag, dt.fills, [t.numel() for t in dt.u8],
                                                                     [t.numel() for t in donor.arenas])
                if self.path != "capacity_retry" or dname == "rolled":   # (a retry's second workspace is sized from the scene's count)
                    assert set(dt.fills) == {"donor"}, (tag, dt.fills)
                if "poison" in fill:
                    want_bytes = sum(n for k in range(len(dt.u8)) if dt.fills[k] == "donor" for _, n in donor.float_ranges[k])
                    assert dt.poisoned_bytes == want_bytes > 0, (tag, dt.poisoned_bytes, want_bytes)
                    names = {nm for nm, kind, k, off, n in donor.regions if kind == dw.FLOAT}
                    assert names == {"rgb", "cov3D", "final_T", "T_end", "T_mid", "q", "partial"}, names
            else:
                assert set(dt.fills) == {"zeros"} and dt.results_filled == dt.results_seen >= 3, (tag, dt.results_filled)
            assert [t.numel() for t in dt.u8] == self.z_allocs, (tag, "the run carved other workspaces than Z")
            self.compare(tag, out, counts)


def _scene(name):
    if name.startswith("batch:"):
        return Batch(name[6:])
    if name.startswith("sets:"):
        return Sets(name[5:])
    return Single(name)


# The first two cases run every path, the others the default path and one more.  capacity_retry is the waiting path with a mark far
# too small; the library never sizes a first pass below 4096 instances (mgs_plan_capacity), which the two small cases do not reach:
# they take the waiting path without a second workspace, and the two cases that bin more than that -- the long lists of a single
# view (the render-only second pass) and the view batch (the whole batch runs again) -- run the path as well and must retry.
ALL_PATHS = ("partial_blocks_17x33_f64", "padded_width_f5")
RETRY_CASES = ("translucent_long_lists_f3", "batch:3_views_f3_72x40")
MATRIX = [(c, p) for c in ALL_PATHS for p in PATHS] + [
    ("black_background_posfocal_f32", "default"), ("black_background_posfocal_f32", "raw_pair"),
    ("translucent_long_lists_f3", "default"), ("translucent_long_lists_f3", "capacity_retry"),
    ("batch:3_views_f3_72x40", "default"), ("batch:3_views_f3_72x40", "marks_only"), ("batch:3_views_f3_72x40", "capacity_retry"),
    ("sets:two_sets_f3_64", "default"), ("sets:two_sets_f3_64", "split_workspaces"),
    # (beyond the list above: precomputed colours without features -- geom.rgb and geom.clamped are then never written nor read, and
    #  the colour gradient is an accumulator region of the caller's buffer instead of slots 6-8 of acc16)
    ("precomp_rgb_no_feature", "default"),
]


@pytest.mark.parametrize("case,path", MATRIX, ids=[f"{c.split(':')[-1]}-{p}" for c, p in MATRIX])
def test_results_do_not_depend_on_what_the_workspaces_held(case, path, monkeypatch, marks_restored):
    _need_gpu()
    scene = _scene(case)
    with _path(path, monkeypatch):
        h = Harness(scene, path, monkeypatch, marks_restored)
        h.prime()
        h.baseline()
        n_u8 = len(h.dt.u8)
        assert n_u8 >= (3 if path == "split_workspaces" else 1)
        if path == "capacity_retry":
            cap = _lib.plan_capacity(_lib.SIZE_COUNT, h.key[0], h.key[5], TINY_MARK)[0]
            retried = h.z_counts[1] > cap
            assert n_u8 == (2 if retried else 1), (n_u8, h.z_counts, cap)
            if case in RETRY_CASES:
                assert retried, "the case no longer outgrows the first pass: the retry path is not exercised"
        # the path is the one named
        a, V = h.dt.handle().a, h.key[5]
        assert a.accum_prezeroed == (0 if path == "raw_pair" else 1)   # who zeroes the backward's accumulators
        waiting = path in ("blocking", "raw_pair", "capacity_retry")
        assert a.async_forward == (0 if waiting else 1), (path, a.async_forward)
        cap_worst = _lib.plan_arena(h.key[0], h.key[1], h.key[2], h.key[3], h.key[4], V, 1 << 40)[3]
        if path == "marks_only":
            assert 0 < a.binning_capacity != cap_worst and a.chunk_pool > 0, (a.binning_capacity, a.chunk_pool, cap_worst)  # the marks
        elif not waiting:
            assert a.binning_capacity == cap_worst                      # safe mode: the worst-case arena
        elif not V:
            assert a.binning_capacity == 0                              # a single view on the waiting path: carved by byte count
        direct = _lib.workspace_regions(a, V)[-1][1] == "direct_keys"   # (on the waiting path the capacity decides: not asserted)
        if not waiting:
            assert direct == (path not in ("scatter_launch", "bin_mode_1", "bin_mode_0")), (path, direct)
        for dname in DONORS:
            donor = h.donor(dname)
            h.dirty(dname, donor)


# ---- the check bites ---------------------------------------------------------------------------------------------------------
def test_a_stale_chunk_record_leaves_the_bound(monkeypatch, marks_restored):
    """Sensitivity: on the raw pair, between forward and backward, the FLOAT chunk-record regions the backward legitimately reads
    (T_end, T_mid, partial) are overwritten with the denser donor's bytes of the same regions.  The gradients must then LEAVE the
    2e-5 bound against Z: the comparison of the test above sees a stale record.  Nothing INDEX is touched.  The same hook without
    the overwrite changes nothing (so it is the overwrite that the comparison sees)."""
    _need_gpu()
    scene = Single("padded_width_f5")
    names = ("T_end", "T_mid", "partial")
    with _path("raw_pair", monkeypatch):
        h = Harness(scene, "raw_pair", monkeypatch, marks_restored)
        h.prime()
        z = h.baseline()
        donor = h.donor("denser")
        src = {nm: (k, off, n) for nm, kind, k, off, n in donor.regions if nm in names}
        assert set(src) == set(names) and all(kind == dw.FLOAT for nm, kind, k, off, n in donor.regions if nm in names)

        def attempt(overwrite):
            done = []

            def between():
                for nm in names:
                    k, off, n = src[nm]
                    dst = h.dt.region(nm)
                    assert dst.numel() == n, "the forward carved another layout than the donor"
                    if overwrite:
                        dst.copy_(donor.arenas[k][off:off + n])
                    done.append(nm)
                torch.cuda.synchronize()

            _raw_pair.between = between
            try:
                out, counts = h.run(scene)
            finally:
                _raw_pair.between = None
            assert done == list(names)
            c, f, r, g = out
            assert torch.equal(c, z[0]) and torch.equal(f, z[1]) and torch.equal(r, z[2]) and counts == h.z_counts  # the forward is Z's
            worst = max((g[k] - z[3][k]).abs().max().item() / (BOUND * z[3][k].abs().max().item() + 1e-12) for k in z[3])
            print(f"  sensitivity: worst gradient deviation {worst:.3g} x the bound (overwrite={overwrite})")
            return worst

        assert attempt(False) <= 1.0   # the hook alone changes nothing ...
        assert attempt(True) > 1.0     # ... the stale records do


def test_float_regions_written_in_full_hold_no_poison(monkeypatch, marks_restored):
    """Map sanity, default path: after a synchronised forward + backward on a donor arena whose FLOAT regions were poisoned, what
    DESIGN.md 8b documents as written holds neither poison pattern: final_T of a single view in full; rgb and cov3D in the rows
    of the Gaussians with a radius; T_end, T_mid and partial in the records of round 0 of every block, at the pixels that visited
    the chunk (last_chunk, nsurv say which).  Where the table says "not written" nothing is asserted."""
    _need_gpu()
    scene = Single("padded_width_f5")
    with _path("default", monkeypatch):
        h = Harness(scene, "default", monkeypatch, marks_restored)
        h.prime()
        h.baseline()
        donor = h.donor("denser")
        for poison, word in zip(POISONS, POISON_WORDS):
            out, counts = h.run(scene, arena="donor", donor=donor, poison=poison)
            assert set(h.dt.fills) == {"donor"} and h.dt.poisoned_bytes > 0
            u32 = lambda nm: h.dt.region(nm).cpu().numpy().view(np.uint32)   # noqa: E731
            P, M, F, W, H, V, S = h.key
            T = ((W + 15) // 16) * ((H + 15) // 16)
            radii = out[2].numpy()
            assert (u32("final_T")[:W * H] != word).all(), "final_T"
            vis = radii > 0
            assert vis.any() and (~vis).any()
            assert (u32("rgb")[:3 * P].reshape(P, 3)[vis] != word).all(), "rgb"
            assert (u32("cov3D")[:6 * P].reshape(P, 6)[vis] != word).all(), "cov3D"
            lc = u32("last_chunk")[:T * 256].reshape(T * 4, 64)
            ns = u32("nsurv")[:T * 8].reshape(T * 4, 2)
            nwf = 8 if (F > 32 or 4 * T > 256) else 16       # fwd_waves(): chunk records per round
            nch = 3 + F
            te, tm, pa = u32("T_end"), u32("T_mid"), u32("partial")
            checked = 0
            for b in range(T * 4):
                for c in range(min(int(lc[b].max()), nwf)):
                    slot = int(ns[b, 1]) + c
                    px = np.nonzero(lc[b] > c)[0]
                    assert (te[slot * 64 + px] != word).all() and (tm[slot * 64 + px] != word).all(), ("T_end / T_mid", b, c)
                    rows = pa[slot * nch * 64:(slot + 1) * nch * 64].reshape(nch, 64)
                    assert (rows[:, px] != word).all(), ("partial", b, c)
                    checked += len(px)
            assert checked > 64 * T, checked
            # ... and something of the poison is still there: the records nobody took, the rows of culled Gaussians
            assert (te == word).any() and (u32("rgb")[:3 * P].reshape(P, 3)[~vis] == word).all()


# ---- call order: the caching allocator's own reuse, through the default binding ------------------------------------------------
def test_interleaved_shapes_repeat_their_first_results():
    """A single view, a view batch and a set batch -- other tile counts, feature widths and kinds -- through the default binding
    (the compiled one where it is built), in the order A B C A C B A, twice: the caching allocator hands every call blocks that the
    calls before it left dirty.  Every repeat equals its shape's first occurrence: images and radii bit for bit, gradients within
    the bound of the float atomics' order."""
    _need_gpu()
    shapes = {"A": Single("padded_width_f5"), "B": Batch("3_views_f3_72x40"), "C": Sets()}
    first = {}
    for rep in range(2):
        for s in "ABCACBA":
            c, f, r, g = shapes[s].run()
            if s not in first:
                first[s] = (c, f, r, g)
                continue
            c0, f0, r0, g0 = first[s]
            tag = f"{s} (round {rep})"
            assert torch.equal(c, c0) and torch.equal(f, f0) and torch.equal(r, r0), tag
            assert g.keys() == g0.keys()
            for k in g0:
                assert (g[k] - g0[k]).abs().max().item() <= BOUND * g0[k].abs().max().item() + 1e-12, (tag, k)
