"""CPU tests of the workspace plan (include/mgsplat.h "the workspace plan", csrc/mgs_plan.hip): the one place that decides how
large a forward's workspaces are and where each gradient lives, for both host bindings.  The library's answers must equal the
restatement over the primitive size queries (tests/plan_cases.py) EXACTLY over the whole grid; no device is needed."""
import ctypes
import itertools

import pytest

from manigaussian_amd import _lib, _state

import plan_cases as pc

INT_MAX = 2**31 - 1


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def test_arena_and_worst_case_equal_the_restatement_over_the_grid(L):
    fits = big = 0
    for (P, W, H, F, V), budget in itertools.product(pc.shapes(), pc.BUDGETS):
        gb, ib, ok, cap, pool, nbytes = _lib.plan_arena(P, pc.M, F, W, H, V, budget)
        assert (gb, ib) == pc.arena(L, P, pc.M, W, H, V), (P, W, H, V)
        assert (ok, cap, pool, nbytes) == pc.worst_case(L, P, W, H, F, V, budget), (P, W, H, F, V, budget)
        if ok:  # what a forward is given and what the budget is charged: one number
            assert _lib.plan_binning_bytes(P, F, W, H, V, cap, pool, False) == nbytes
        fits += ok
        big += cap >= 1 << 30
    assert (fits, 576 * 3 - fits, big) == (408, 1320, 444)  # every branch is reached


def test_binning_bytes_equal_the_restatement_with_and_without_direct_room(L):
    offered = 0
    for P, W, H, F, V in pc.shapes():
        T = pc.tiles(W, H, V)
        offered += L.mgs_binning_direct_extra(P, V, W, H) > 0
        assert L.mgs_binning_direct_extra(P, V, W, H) == L.mgs_binning_direct_extra(P, max(V, 1), W, H)
        for cap, pool in ((4096, 0), (8192 * T + 4097, 64), (min(P * T, (1 << 30) - 1), 0), (123457, 1000)):
            assert _lib.plan_binning_bytes(P, F, W, H, V, cap, pool, False) == pc.binning_bytes(L, cap, pool, W, H, F, V)
            assert _lib.plan_binning_bytes(P, F, W, H, V, cap, pool, True) == pc.binning_bytes(L, cap, pool, W, H, F, V, P)
    assert (offered, 576 - offered) == (244, 332)


def test_capacities_follow_the_marks_the_headroom_and_the_counts():
    st = _state.DeviceState.__new__(_state.DeviceState)  # (no pinned memory needed for the marks)
    old = dict(_state._HEADROOM)
    try:
        for R, chunks, hi, hc in itertools.product((0, 1, 3, 10001, 8192 * 64 + 1, 2**31 + 7), (0, 1, 401, 99999),
                                                   pc.HEADROOMS, pc.HEADROOMS):
            want = pc.capacity_headroom(R, chunks, hi, hc)
            assert _lib.plan_capacity(_lib.SIZE_HEADROOM, 0, 0, R, chunks, hi, hc) == want
            _state._HEADROOM.update(instances=hi, chunks=hc)
            st.marks = {"k": [R, chunks], "pool unknown": [R, None]}
            assert st.guess("k") == want and st.guess("pool unknown") is None and st.guess("no marks") is None
    finally:
        _state._HEADROOM.update(old)
    assert pc.capacity_headroom(3, 1, 1.5, 1.5) == (4 + 4096, 1 + 64)  # 4.5 and 1.5 truncated, not rounded
    for P, V in itertools.product(pc.PS, pc.VS):
        assert _lib.plan_capacity(_lib.SIZE_COUNT, P, V, -1) == pc.capacity_count(None, P, V)  # no mark: first call of a shape
        for R in (0, 1, 3, 4095, 123457, 2**31 - 1):  # a mark alone, or the count the device reported (retry, recover)
            assert _lib.plan_capacity(_lib.SIZE_COUNT, P, V, R) == pc.capacity_count(R, P, V)


def test_options_are_tuned_from_the_mark_and_an_explicit_seg_is_left_alone():
    changed = 0
    for (W, H), V in itertools.product(pc.SIZES, pc.VS):
        T = pc.tiles(W, H, V)
        for R in (0, 8192 * T, 8192 * T + 1, 24576 * T, 24576 * T + 1):
            for seg, bin_mode in itertools.product((512, 2048, 4096), (0, 1, 2)):
                got = _lib.plan_options(seg, bin_mode, R, W, H, V) or (seg, bin_mode)
                assert got == pc.options(seg, bin_mode, R, T), (W, H, V, R, seg, bin_mode)
                assert seg == 2048 or got[0] == seg
                changed += got != (seg, bin_mode)
    assert changed == len(pc.SIZES) * len(pc.VS) * (3 + 3 + 5)  # seg alone above 8192 T; bin_mode (and seg) above 24576 T


def test_gradient_layout_equals_the_restatement_and_the_recorded_totals(L):
    for (P, M, F, V, precomp, S), (total, accum) in pc.GRADIENTS.items():
        got = _lib.plan_gradients(P, M, F, V, S, precomp)
        assert got == pc.gradients(L, P, M, F, V, precomp, S)
        assert got[1:] == (total, accum)
    for P, M, F, V, S, precomp in itertools.product((1, 1000, 100000, 2000000), (0, 4, 16), (0, 3, 64), (0, 1, 16), (0, 2, 16),
                                                    (False, True)):
        if not S or V:
            assert _lib.plan_gradients(P, M, F, V, S, precomp) == pc.gradients(L, P, M, F, V, precomp, S)


def test_bad_shapes_are_refused_not_wrapped(L):
    ok = dict(P=1000, M=4, F=3, W=128, H=128, V=0, S=0, colors_precomp=0)
    bad = [dict(P=-1), dict(W=-16), dict(W=0), dict(H=-1), dict(M=-1), dict(F=-1), dict(V=-1), dict(V=_lib.MAX_VIEWS + 1),
           dict(V=2, S=_lib.MAX_VIEWS + 1), dict(S=2), dict(P=INT_MAX // 16 + 1, V=16), dict(P=INT_MAX // 2 + 1, V=2, S=2),
           dict(W=INT_MAX, H=INT_MAX), dict(W=1 << 20, H=1 << 20)]
    arena, grads = _lib.MgsArenaPlan(), _lib.MgsGradientPlan()
    cap, pool = ctypes.c_int64(7), ctypes.c_int64(7)
    for change in [{}] + bad:
        s = _lib.MgsPlanShape(**dict(ok, **change))
        want = _lib.MGS_ERR_INVALID_ARG if change else _lib.MGS_OK
        opt = _lib.MgsOptions(seg=2048, bin_mode=2)
        assert L.mgs_plan_arena(s, 1 << 30, arena) == want, change
        assert L.mgs_plan_gradients(s, grads) == want, change
        assert L.mgs_plan_capacity(s, _lib.SIZE_COUNT, 1000, 0, 1.0, 1.0, cap, pool) == want, change
        assert L.mgs_plan_options(s, 1 << 40, opt) == want, change
        assert (L.mgs_plan_binning_bytes(s, 4096, 0, 1) == 0) == bool(change), change
        if change:
            assert (arena.geom_bytes, arena.img_bytes, arena.worst_bytes, arena.worst_fits, grads.total, grads.accum_bytes,
                    cap.value, pool.value, opt.seg, opt.bin_mode) == (0, 0, 0, 0, 0, 0, 0, 0, 2048, 2), change
            assert _lib.last_error()
    s = _lib.MgsPlanShape(**ok)
    for capacity, chunk_pool in ((INT_MAX + 1, 0), (-1, 0), (4096, INT_MAX + 1), (4096, -1), (1 << 32, 0)):  # past the ABI's int
        assert L.mgs_plan_binning_bytes(s, capacity, chunk_pool, 0) == 0
    assert L.mgs_plan_capacity(s, _lib.SIZE_HEADROOM, -1, 0, 1.5, 2.0, cap, pool) == _lib.MGS_ERR_INVALID_ARG
    assert L.mgs_plan_capacity(s, _lib.SIZE_HEADROOM, 10, 10, 0.5, 2.0, cap, pool) == _lib.MGS_ERR_INVALID_ARG
    assert L.mgs_plan_capacity(s, 7, 10, 10, 1.5, 2.0, cap, pool) == _lib.MGS_ERR_INVALID_ARG
    with pytest.raises(RuntimeError, match="mgs_plan_arena"):
        _lib.plan_arena(-1, 4, 3, 128, 128, 0, 1 << 30)
    with pytest.raises(RuntimeError, match="do not fit an int"):
        _lib.plan_binning_bytes(1000, 3, 128, 128, 0, INT_MAX + 1, 0, False)


class _CountingLibrary:
    """The library behind a counter of the calls that reach it."""

    def __init__(self, L):
        self.L, self.calls = L, 0

    def __getattr__(self, name):
        fn = getattr(self.L, name)

        def call(*a):
            self.calls += 1
            return fn(*a)
        return call


def test_a_repeated_look_up_does_not_reach_the_library(L, monkeypatch):
    """What the shim's speed rests on: a warm forward sizes itself from _lib._PLANS -- also where the answer is None (options
    that stay as they are: the usual case), and also after the count-keyed answers of a growing scene were dropped."""
    counting = _CountingLibrary(L)
    monkeypatch.setattr(_lib, "lib", lambda: counting)
    monkeypatch.setattr(_lib, "_PLANS", {})
    asks = [lambda: _lib.plan_arena(16384, 4, 3, 128, 128, 0, 1 << 30),
            lambda: _lib.plan_gradients(16384, 4, 3, 0, 0, False),
            lambda: _lib.plan_binning_bytes(16384, 3, 128, 128, 0, 94096, 1864, True),
            lambda: _lib.plan_capacity(_lib.SIZE_HEADROOM, 0, 0, 60000, 900, 1.5, 2.0),
            lambda: _lib.plan_capacity(_lib.SIZE_COUNT, 16384, 0, 60000),
            lambda: _lib.plan_options(2048, 2, 60000, 128, 128, 0),            # short lists: None
            lambda: _lib.plan_options(2048, 2, 24576 * 64 + 1, 128, 128, 0)]   # very long ones: (4096, 1)
    first = [ask() for ask in asks]
    assert first[5] is None and first[6] == (4096, 1)
    assert counting.calls == len(asks)
    for _ in range(5):
        assert [ask() for ask in asks] == first
    assert counting.calls == len(asks)
    # marks that keep growing fill the dict with count-keyed answers: dropping them keeps what is keyed by the shape alone
    for R in range(5000):
        _lib.plan_capacity(_lib.SIZE_COUNT, 16384, 0, R)
    assert len(_lib._PLANS) <= 4097
    calls = counting.calls
    assert [asks[0](), asks[1]()] == first[:2] and counting.calls == calls
