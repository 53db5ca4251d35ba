"""The report ledger of libmgsplat.so (csrc/mgs_ledger.hip, include/mgsplat.h "the report ledger"): who is outstanding, what was
learned, what to say -- driven through ctypes without a device.  Each test takes a device index nothing else uses, gives it a
numpy array as its ring of status slots and writes the status words a device would write by hand:
  bits 63..48 the tag, 47..32 flags, the low 32 bits the value; all ones: pending
  word 0: instances binned (flag bit 1: the table hand-shake gave up), word 1: chunk records (bit 32: the pool overflowed),
  word 2: the reference's count."""
import ctypes
import itertools

import numpy as np
import pytest

from manigaussian_amd import _lib, _state

OK, NEED_CAPACITY, PENDING, RETRY = _lib.MGS_OK, _lib.MGS_NEED_CAPACITY, _lib.MGS_PENDING, _lib.MGS_RETRY_TABLE_INIT
ALL_ONES = np.uint64(0xffffffffffffffff)
KEY = (1000, 64, 64, 3, 1)
_DEVICES = itertools.count(20)  # (7 and 9 serve tests/test_compiled.py and tests/test_api.py; a GPU test's devices are 0..)
_RINGS = []                     # a ring outlives its test: the ledger keeps the address


def word(tag, value, flags=0):
    return np.uint64((tag << 48) | (flags << 32) | value)


class Forward:
    def __init__(self, ticket, first_word, tag, slot):
        self.ticket, self.w, self.tag, self.slot = ticket, first_word, tag, slot


class Ledger:
    """One device of the ledger over a ring of plain memory."""

    def __init__(self, nslots=8):
        self.L, self.dev, self.nslots = _lib.lib(), next(_DEVICES), nslots
        self.ring = np.full(nslots * _lib.LEDGER_SLOT_WORDS, ALL_ONES, dtype=np.uint64)
        _RINGS.append(self.ring)
        assert self.L.mgs_ledger_ring(self.dev, None, 0) is None
        assert self.L.mgs_ledger_ring(self.dev, self.ring.ctypes.data, nslots) == self.ring.ctypes.data
        assert self.L.mgs_ledger_ring_slots(self.dev) == nslots
        self.marks = _state._Marks(self.dev)

    def take_slot(self):
        slot, tag = ctypes.c_void_p(), ctypes.c_uint32()
        rc = self.L.mgs_ledger_take_slot(self.dev, slot, tag)
        return rc, slot.value, tag.value

    def forward(self, flags=0, key=KEY, capacity=100, pool=10, V=0):
        """What a binding does around an asynchronous forward: a slot, the arguments, (the launch,) a ticket."""
        rc, slot, tag = self.take_slot()
        assert rc == OK
        a = _lib.MgsRasterArgs()
        a.P, a.W, a.H, a.F, a.include_feature = 1000, 64, 64, 3, 1
        a.binning_capacity, a.chunk_pool, a.binning_bytes, a.status_tag, a.async_forward = capacity, pool, 1 << 40, tag, 1
        w = (slot - self.ring.ctypes.data) // 8
        self.ring[w:w + 3] = ALL_ONES  # (the forward call sets its words to pending before it enqueues)
        t = self.L.mgs_ledger_add(self.dev, a, V, slot, _state._mark_key(key), flags)
        assert t
        return Forward(t, w, tag, slot)

    def report(self, f, binned=50, chunks=5, ref=60, handshake=False, pool_overflow=False, tag=None):
        tag = f.tag if tag is None else tag
        self.ring[f.w + 2] = word(tag, ref)
        self.ring[f.w] = word(tag, binned, 2 if handshake else 0)
        self.ring[f.w + 1] = word(tag, chunks, 1 if pool_overflow else 0)

    def poll(self, f):
        r = _lib.MgsReport()
        rc = self.L.mgs_ledger_poll(f.ticket, r)
        assert rc == r.rc
        return rc, r.num_rendered, r.chunks_used, r.ref_rendered

    def drain(self, wait=False, sync=None):
        """(error text or None, warning texts)"""
        out = _lib.MgsLedgerOut()
        fn = _lib.LEDGER_SYNC_FN(sync if sync is not None else lambda ctx: None)
        assert self.L.mgs_ledger_drain(self.dev, int(wait), fn, None, out) == OK
        return (out.error.decode() if out.error else None), [out.warnings[i].decode() for i in range(out.n_warnings)]

    def check_captured(self):
        out = _lib.MgsLedgerOut()
        assert self.L.mgs_ledger_check_captured(self.dev, out) == OK
        return (out.error.decode() if out.error else None), [out.warnings[i].decode() for i in range(out.n_warnings)]

    def outstanding(self):
        return self.L.mgs_ledger_outstanding(self.dev)


@pytest.fixture
def policy():
    """Sets the overflow policy for one test (the configuration is the process's)."""
    L = _lib.lib()
    old = _lib.MgsLedgerConfig()
    L.mgs_ledger_get_config(old)

    def set_policy(name):
        c = _lib.MgsLedgerConfig(old.mode, {"repair": 0, "raise": 1}[name], old.head_instances, old.head_chunks, old.safe_bytes)
        L.mgs_ledger_set_config(c)
    yield set_policy
    L.mgs_ledger_set_config(old)


def test_a_finished_forward_is_learned_and_its_counts_are_handed_out():
    led = Ledger()
    f = led.forward()
    assert led.poll(f) == (PENDING, -1, -1, -1) and led.drain() == (None, []) and led.outstanding() == 1
    led.ring[f.w + 2], led.ring[f.w] = word(f.tag, 60), word(f.tag, 50)  # the preprocess has reported, the render has not
    assert led.poll(f) == (PENDING, 50, -1, 60) and led.drain() == (None, []) and KEY not in led.marks
    led.report(f)
    assert led.drain() == (None, []) and led.outstanding() == 0
    assert led.marks[KEY] == [50, 5] and led.poll(f) == (OK, 50, 5, 60)
    g = led.forward()
    led.report(g, binned=40, chunks=9)
    assert led.drain() == (None, []) and led.marks[KEY] == [50, 9]  # marks only grow
    for x in (f, g):
        led.L.mgs_ledger_release(x.ticket)


def test_instances_over_capacity_raise_the_instance_mark_and_keep_the_chunk_mark():
    led = Ledger()
    led.marks[KEY] = [50, 5]
    f = led.forward(capacity=100)
    led.ring[f.w + 2], led.ring[f.w] = word(f.tag, 700), word(f.tag, 500)  # word 0 alone says so: nothing was binned
    assert led.poll(f)[:2] == (NEED_CAPACITY, 500)
    err, warns = led.drain()
    assert "outgrew the workspace" in err and "500 (Gaussian, tile) instances > capacity 100" in err and warns == []
    assert "gradients were computed on the incomplete state" in err  # (not recoverable: nobody can re-render it)
    assert led.marks[KEY] == [500, 5] and led.outstanding() == 0
    assert led.drain() == (None, [])


def test_a_pool_overflow_resets_the_chunk_mark_and_there_is_no_guess():
    led = Ledger()
    led.marks[KEY] = [50, 5]
    cap, pool = ctypes.c_int64(), ctypes.c_int64()
    assert led.L.mgs_marks_guess(led.dev, _state._mark_key(KEY), cap, pool) == 1
    assert (cap.value, pool.value) == _lib.plan_capacity(_lib.SIZE_HEADROOM, 0, 0, 50, 5, 1.5, 2.0) == (75 + 4096, 10 + 64)
    f = led.forward(pool=10)
    led.report(f, binned=60, chunks=10, pool_overflow=True)
    assert led.poll(f)[0] == NEED_CAPACITY
    err, warns = led.drain()
    assert "outgrew the workspace" in err and "chunk pool of 10 records" in err and warns == []
    assert led.marks[KEY] == [60, None]
    assert led.L.mgs_marks_guess(led.dev, _state._mark_key(KEY), cap, pool) == 0


def test_a_handshake_give_up_asks_for_a_retry_and_teaches_nothing():
    led = Ledger()
    f = led.forward()
    led.report(f, binned=0, chunks=0, handshake=True)
    assert led.poll(f)[0] == RETRY
    err, warns = led.drain()
    assert "zeroed tile tables" in err and "table_init=1" in err and warns == []
    assert KEY not in led.marks and len(led.marks) == 0


@pytest.mark.parametrize("what", ["instances", "handshake"])
def test_policy_repair_warns_once_for_a_recoverable_ticket_and_raises_once_its_backward_is_enqueued(policy, what):
    policy("repair")
    led = Ledger()
    bad = dict(binned=500) if what == "instances" else dict(binned=0, chunks=0, handshake=True)
    f = led.forward(flags=_lib.TICKET_RECOVERABLE)
    led.report(f, **bad)
    err, warns = led.drain()
    assert err is None and len(warns) == 1 and "re-renders" in warns[0]
    assert ("outgrew the workspace" if what == "instances" else "zeroed tile tables") in warns[0]
    assert led.drain() == (None, [])
    g = led.forward(flags=_lib.TICKET_RECOVERABLE)
    led.L.mgs_ledger_backward_enqueued(g.ticket)  # (its report had not arrived at backward entry)
    led.report(g, **bad)
    err, warns = led.drain()
    assert warns == [] and "gradients were computed on the incomplete state" in err and "re-renders" not in err
    assert ("outgrew" if what == "instances" else "zeroed tile tables") in err
    assert led.drain() == (None, [])


def test_policy_raise_raises_once_and_the_backward_has_its_own_words(policy):
    policy("raise")
    led = Ledger()
    f = led.forward(flags=_lib.TICKET_RECOVERABLE)
    led.report(f, binned=500)
    err, warns = led.drain()
    assert warns == [] and "outgrew the workspace" in err and "the step is lost (overflow policy 'raise')" in err
    assert led.drain() == (None, []) and led.marks[KEY][0] == 500
    assert "outgrew" in led.L.mgs_ledger_lost_step_message(NEED_CAPACITY).decode()
    assert "zeroed tile tables" in led.L.mgs_ledger_lost_step_message(RETRY).decode()


def test_a_superseded_ticket_is_accounted_once(policy):
    policy("raise")  # (a ticket that a recovery re-ran is a warning under either policy)
    led = Ledger()
    f = led.forward(flags=_lib.TICKET_RECOVERABLE)
    led.report(f, binned=500)
    assert led.poll(f)[0] == NEED_CAPACITY  # the backward sees it first, re-renders under a ticket of its own ...
    g = led.forward(capacity=1000, pool=0)
    led.L.mgs_ledger_superseded(f.ticket)
    led.report(g, binned=500, chunks=30)
    err, warns = led.drain()
    assert err is None and len(warns) == 1 and "re-renders" in warns[0] and led.outstanding() == 0
    assert led.marks[KEY] == [500, 30]
    assert led.drain() == (None, []) and led.drain(wait=True) == (None, [])


def test_a_stale_tag_is_still_pending():
    led = Ledger()
    f = led.forward()
    led.report(f, tag=(f.tag + 1) & 0xffff)  # an earlier user of the slot, or a later one
    assert led.poll(f) == (PENDING, -1, -1, -1) and led.drain() == (None, []) and led.outstanding() == 1
    led.report(f)
    assert led.drain() == (None, []) and led.outstanding() == 0 and led.marks[KEY] == [50, 5]


def test_wait_synchronises_once_and_accounts_what_arrived_by_then():
    led = Ledger()
    f, g = led.forward(), led.forward()
    calls = []

    def sync(ctx):
        calls.append(ctx)
        led.report(f)
        led.report(g, binned=70, chunks=3)
    assert led.drain(wait=True, sync=sync) == (None, []) and len(calls) == 1
    assert led.outstanding() == 0 and led.marks[KEY] == [70, 5]
    assert led.drain(wait=True, sync=sync) == (None, []) and len(calls) == 1  # nothing outstanding: no synchronisation


def test_a_forward_that_never_reports_fails_the_wait_and_is_dropped():
    led = Ledger()
    led.forward()
    err, warns = led.drain(wait=True)
    assert "finished without reporting its instance count" in err and warns == [] and led.outstanding() == 0
    assert led.drain(wait=True) == (None, [])


def test_a_ticket_added_during_the_synchronisation_is_kept():
    led = Ledger()
    f = led.forward()
    late = []

    def sync(ctx):
        led.report(f)
        late.append(led.forward())  # another thread's forward, enqueued after the device was synchronised
    assert led.drain(wait=True, sync=sync) == (None, []) and led.outstanding() == 1
    led.report(late[0], binned=90)
    assert led.drain() == (None, []) and led.outstanding() == 0 and led.marks[KEY] == [90, 5]


def test_more_than_half_the_ring_outstanding_synchronises_without_being_asked():
    led = Ledger(nslots=8)
    calls = []
    fs = [led.forward() for _ in range(3)]
    assert led.drain(sync=calls.append) == (None, []) and calls == [] and led.outstanding() == 3
    fs += [led.forward() for _ in range(2)]  # 5 forwards: behind the first of them 4 = 8 / 2 are still outstanding

    def sync(ctx):
        calls.append(ctx)
        for f in fs:
            led.report(f)
    assert led.drain(sync=sync) == (None, []) and len(calls) == 1 and led.outstanding() == 0


def test_captured_tickets_keep_their_slots_and_report_at_every_replay():
    led = Ledger(nslots=4)
    f = led.forward(flags=_lib.TICKET_CAPTURED)
    assert led.outstanding() == 0  # (not a forward a drain waits for)
    taken = [led.take_slot() for _ in range(7)]
    assert all(rc == OK and slot != f.slot for rc, slot, _ in taken) and len({slot for _, slot, _ in taken}) == 3
    assert len({tag for _, _, tag in taken}) == 7
    assert led.check_captured() == (None, [])
    led.report(f, binned=500)  # a replay on a scene that grew
    err, warns = led.check_captured()
    assert "outgrew the workspace" in err and warns == [] and led.marks[KEY][0] == 500
    led.report(f)              # the next replay fits
    assert led.check_captured() == (None, []) and led.drain(wait=True) == (None, [])


def test_a_ring_whose_slots_are_all_captured_has_none_to_give():
    led = Ledger(nslots=2)
    for _ in range(2):
        led.forward(flags=_lib.TICKET_CAPTURED)
    rc, _, _ = led.take_slot()
    assert rc == _lib.MGS_ERR_INVALID_ARG and _lib.last_error() == "all status slots are held by captured graphs"


def test_hold_refuses_what_would_pass_the_budget_and_changes_nothing():
    L, dev = _lib.lib(), next(_DEVICES)
    assert L.mgs_ledger_held(dev) == 0
    assert L.mgs_ledger_hold(dev, 60, 100) == 1 and L.mgs_ledger_held(dev) == 60
    assert L.mgs_ledger_hold(dev, 41, 100) == 0 and L.mgs_ledger_held(dev) == 60
    assert L.mgs_ledger_hold(dev, 40, 100) == 1 and L.mgs_ledger_held(dev) == 100
    assert L.mgs_ledger_hold(dev, 1, 100) == 0 and L.mgs_ledger_hold(dev, 0, 0) == 0
    L.mgs_ledger_unhold(dev, 60)
    L.mgs_ledger_unhold(dev, 40)
    assert L.mgs_ledger_held(dev) == 0 and L.mgs_ledger_hold(dev, 0, 0) == 1
    assert _state.held_bytes(dev) == 0


def test_marks_round_trip_for_the_three_kinds_of_key():
    m = _state._Marks(next(_DEVICES))
    keys = [(1000, 64, 64, 3, 1), ("views", 4, 1000, 64, 64, 3, 1), ("sets", 2, 4, 1000, 64, 64, 3, 1), (1000, 64, 64, 3, 0)]
    for i, k in enumerate(keys):
        assert k not in m and m.get(k) is None
        m[k] = [100 + i, None if i % 2 else 7 + i]
    assert len(m) == 4 and set(m) == set(keys)
    for i, k in enumerate(keys):
        assert m[k] == [100 + i, None if i % 2 else 7 + i]
    m[keys[1]] = [2 ** 40, 2 ** 33]
    assert m[keys[1]] == [2 ** 40, 2 ** 33] and m[keys[0]] == [100, 7]
    del m[keys[2]]
    with pytest.raises(KeyError):
        del m[keys[2]]
    with pytest.raises(KeyError):
        m[keys[2]]
    with pytest.raises(KeyError):
        m[("tiles", 1, 2, 3, 4, 5, 6)]
    assert set(m) == {keys[0], keys[1], keys[3]}
    m.clear()
    assert len(m) == 0 and list(m) == []


def test_configuration_round_trips_and_bad_devices_are_refused():
    L = _lib.lib()
    old, got = _lib.MgsLedgerConfig(), _lib.MgsLedgerConfig()
    L.mgs_ledger_get_config(old)
    try:
        L.mgs_ledger_set_config(_lib.MgsLedgerConfig(1, 1, 3.0, 4.0, 12345))
        L.mgs_ledger_get_config(got)
        assert (got.mode, got.overflow_policy, got.head_instances, got.head_chunks, got.safe_bytes) == (1, 1, 3.0, 4.0, 12345)
    finally:
        L.mgs_ledger_set_config(old)
    out = _lib.MgsLedgerOut()
    for dev in (-1, 64):
        assert L.mgs_ledger_ring(dev, None, 0) is None and L.mgs_ledger_drain(dev, 1, _lib.LEDGER_SYNC_FN(), None, out) < 0
        assert L.mgs_ledger_hold(dev, 1, 10) == 0 and L.mgs_ledger_held(dev) == 0
