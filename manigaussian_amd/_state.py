"""Host-side bookkeeping of the asynchronous forward (include/mgsplat.h: mgs_rasterize_forward with async_forward = 1).

The reference blocks every forward on a cudaMemcpy of `num_rendered` (RAST/cuda_rasterizer/rasterizer_impl.cu:284) because
its binning buffer is sized from that count.  Three forward modes (set_forward_mode / MGS_FORWARD_MODE):

  "safe" (default)  a forward can NEVER hand back incomplete images.  A shape whose worst-case workspace fits the budget
                    (set_safe_workspace, default 1 GB: ManiGaussian's own 16 384-Gaussian shape needs 206 MB) is enqueued
                    without any host-device synchronisation -- it cannot overflow; every other shape enqueues everything
                    with a workspace sized from the shape's marks and waits for the PREPROCESS's report only (two pinned
                    words; round 4 waited for the whole render): binning and render are running while the call returns, and
                    a scene that outgrew the buffer is binned and rendered again with room before the call returns.
  "async" (opt-in)  every shape is enqueued without synchronisation: the workspace is sized from what earlier forwards of the
                    same shape needed (high-water marks + head-room) and the device reports {instances, chunk records used,
                    overflow} through two pinned host words.  What HIP-graph capture and a GPU-bound 0.15 ms step need;
                    the price is the overflow protocol below (a scene that outgrows its marks is repaired at backward entry
                    with a RuntimeWarning, or raises late).
  "blocking"        every forward waits for the count (the reference's behaviour, also for small shapes).

The accounting itself lives in libmgsplat.so (csrc/mgs_ledger.hip, include/mgsplat.h "the report ledger"), one store per
device for this shim and the compiled binding alike:

  * the ring of pinned status slots (one per in-flight forward, tagged so that a stale write is recognisable),
  * the high-water marks per (device, problem shape),
  * the forwards whose report has not been read yet, the budget of worst-case workspaces, every message.

This module holds the switches (mode, policy, head-room, budget: pushed to the ledger), the Python faces of a device's state
and of a ticket (DeviceState, Pending), and issues what a drain hands back as RuntimeWarning / RuntimeError.

Reports are read lazily and never waited for on the hot path: at the next forward, at a backward, or on
`check_status()`.  If a scene outgrew its workspace the images (and gradients) of THAT call were incomplete; the first
later call into this module raises RuntimeError (loud, late) after raising the marks so that a re-run fits.  The first
forward of a shape, `debug=True` settings and `set_forward_mode("blocking")` take the blocking path, which cannot overflow.
"""
import collections
import collections.abc
import ctypes
import os
import threading
import warnings
import weakref

import numpy
import torch

from . import _lib

NSLOTS = 1024  # status slots per device (four 64-bit words each, three used); far more than forwards can be in flight
SLOT_WORDS = 4
SLOT_BYTES = 8 * SLOT_WORDS

# ---- the compiled binding (csrc/mgs_torch.cpp -> _mgs_torch.so): the hot autograd path when present ---------------------------
_EXT = [False]  # False: not looked for yet; None: absent / disabled; else the module


def ext():
    """manigaussian_amd._mgs_torch, or None (not built, MGS_NO_COMPILED=1): the ctypes shim then does everything."""
    e = _EXT[0]
    if e is False:
        e = None
        if not os.environ.get("MGS_NO_COMPILED"):
            try:
                _lib.lib()  # the binding links libmgsplat.so: fail with the loader's message, not the linker's
                from . import _mgs_torch as e
                if e.ABI_VERSION != _lib.ABI_VERSION:
                    raise ImportError(f"_mgs_torch ABI {e.ABI_VERSION} != {_lib.ABI_VERSION}")
            except ImportError as err:
                warnings.warn(f"manigaussian_amd: the compiled binding is not available ({err}); using the ctypes shim "
                              "(same kernels, ~3x the host time per call).  Build it with `make -C manigaussian_amd/csrc ext`.",
                              RuntimeWarning)
                e = None
        _EXT[0] = e
        if e is not None:
            _push_config()
            _lib.push_options()
    return e


def _push_config():
    """The switches below, to the ledger: its messages and mgs_marks_guess go by them, the compiled binding reads them there."""
    c = _lib.MgsLedgerConfig({"safe": 0, "async": 1, "blocking": 2}[_MODE], {"repair": 0, "raise": 1}[_OVERFLOW],
                             _HEADROOM["instances"], _HEADROOM["chunks"], -1 if _SAFE_BYTES is None else _SAFE_BYTES)
    _lib.lib().mgs_ledger_set_config(c)


_WORDS = {}  # slot pointer -> (numpy view of its device's status block, index of the slot's first word)
_MODE = os.environ.get("MGS_FORWARD_MODE", "safe")  # "safe" | "async" | "blocking"
_STATES = {}
_LOCK = threading.Lock()


def set_forward_mode(mode: str):
    """"safe" (default): no host-device synchronisation for shapes whose worst-case workspace fits the budget (they cannot
    overflow), the reference's blocking read of the instance count for every other shape -- a forward never returns
    incomplete images; "async": no synchronisation for any shape, workspaces sized from earlier calls (opt-in: see the
    module docstring for what an overflow then means); "blocking": every forward waits like the reference does.
    Returns the previous mode."""
    global _MODE
    if mode not in ("safe", "async", "blocking"):
        raise ValueError("forward mode is 'safe', 'async' or 'blocking'")
    old, _MODE = _MODE, mode
    _push_config()
    return old


def forward_mode() -> str:
    return _MODE


# "async" mode only: what the backward does when it learns that ITS forward outgrew the workspace.  "repair": render the
# forward again on the blocking path into the same output tensors, warn, go on -- the gradients are those of the complete
# render, but whatever the caller computed from the incomplete images in between (the loss VALUE, its cotangents) is not
# repaired: the step mixes the two.  "raise": RuntimeError at backward entry; the step is lost, nothing inconsistent is
# applied.  (The default mode "safe" never gets here.)
_OVERFLOW = os.environ.get("MGS_OVERFLOW_POLICY", "repair")


def set_overflow_policy(policy: str):
    """"repair" (default) or "raise": see above.  Returns the previous policy."""
    global _OVERFLOW
    if policy not in ("repair", "raise"):
        raise ValueError("overflow policy is 'repair' or 'raise'")
    old, _OVERFLOW = _OVERFLOW, policy
    _push_config()
    return old


def overflow_policy() -> str:
    return _OVERFLOW


def lazy_allowed(cannot_overflow: bool) -> bool:
    """May a forward be enqueued without waiting for its instance count?  "async": always (marks permitting); "safe": only
    with a workspace that cannot overflow; "blocking": never."""
    return _MODE == "async" or (_MODE == "safe" and cannot_overflow)


# Head-room of an asynchronous forward's workspace over the high-water marks of its shape: the scene may grow by these
# factors from one call to the next before a call overflows (and raises, late).  Scenes that differ wildly between calls of
# one shape (a parity sweep, a data loader mixing scenes) want more, or set_forward_mode("blocking").
def _headroom(v) -> float:
    if not 1.0 <= float(v) < 1024.0:  # (the range mgs_plan_capacity sizes a workspace for: include/mgsplat.h)
        raise ValueError("head-room factors are >= 1 (and below 1024)")
    return float(v)


_HEADROOM = {"instances": _headroom(os.environ.get("MGS_HEADROOM_INSTANCES", 1.5)),
             "chunks": _headroom(os.environ.get("MGS_HEADROOM_CHUNKS", 2.0))}


# A shape whose WORST-CASE workspace (every Gaussian in every tile, every chunk of every block visited) stays below this many
# bytes is always given that workspace: its forwards cannot overflow, need no warm-up call, no marks and NO wait of any kind.
# Default (round 5): 1/32 of the device's memory, at least 1 GB -- 9 GB on a 288 GB MI355X: ManiGaussian's own shape (16 384
# Gaussians, 128 x 128, 3 feature channels) needs 206 MB, BASELINE configs[1] / [2] (100 000 Gaussians, 128 x 128) 4.0 GB per
# forward in flight; the configs[4] shape (500 000 at 256 x 256: 79 GB) waits for the preprocess's report instead.  Rounds 2-4
# used a fixed 1 GB: configs[2] then went by the marks, and under default options its host ran in lock step with the device
# (one wait per forward; up to +12 % on a slow host, profiles/r05_bench_c2.json).  MGS_SAFE_WORKSPACE_MB / set_safe_workspace
# fix the budget in megabytes (0: never allocate the worst case).
_SAFE_BYTES = (int(float(os.environ["MGS_SAFE_WORKSPACE_MB"]) * (1 << 20)) if os.environ.get("MGS_SAFE_WORKSPACE_MB") else None)
_AUTO_SAFE = {}  # device index -> max(1 GB, total memory / 32)
SAFE_FRACTION = 32


def set_safe_bytes(nbytes):
    """The budget in bytes; None: the default (1/32 of the device's memory, at least 1 GB).  Returns the previous setting."""
    global _SAFE_BYTES
    old, _SAFE_BYTES = _SAFE_BYTES, (None if nbytes is None else int(nbytes))
    _push_config()
    return old


def set_safe_workspace(megabytes):
    """Largest worst-case workspace (MB) a forward simply allocates instead of sizing it from earlier calls / the device's
    report (None: the default, 1/32 of the device's memory)."""
    set_safe_bytes(None if megabytes is None else int(float(megabytes) * (1 << 20)))


def safe_bytes(dev=None) -> int:
    if _SAFE_BYTES is not None:
        return _SAFE_BYTES
    idx = -1
    if torch.cuda.is_available():
        idx = dev.index if (dev is not None and getattr(dev, "index", None) is not None) else torch.cuda.current_device()
    v = _AUTO_SAFE.get(idx)
    if v is None:
        total = torch.cuda.get_device_properties(idx).total_memory if idx >= 0 else 0
        v = _AUTO_SAFE[idx] = max(1 << 30, total // SAFE_FRACTION)
    return v


# ---- worst-case workspaces that live forwards still hold: the budget is charged against their SUM per device -----------------
# (round 5 tested it per call: V forwards before the first backward pinned V x 4 GB at BASELINE configs[2].)  The ledger keeps
# the counter: the compiled binding's forwards charge it too.
def held_bytes(index: int) -> int:
    """Bytes of worst-case workspaces live forwards hold on device `index`."""
    return int(_lib.lib().mgs_ledger_held(index))


def worst_case_fits(index: int, nbytes: int, dev=None) -> bool:
    """Would a worst-case workspace of `nbytes` fit now?  (what is held + this one) <= the budget.  Only a look: a forward
    that acts on the answer takes a Charge, which asks and reserves in one step."""
    return held_bytes(index) + int(nbytes) <= safe_bytes(dev)


def _unhold(index, nbytes):
    _lib.lib().mgs_ledger_unhold(index, nbytes)


def hold(index: int, nbytes: int, owner):
    """Charge `nbytes` against device `index`'s budget, whatever is held, until `owner` (the workspace tensor) is freed."""
    Charge(index, nbytes, None).give(owner)


class Charge:
    """A worst-case workspace of `nbytes` asked of device `index`'s budget (None: not asked, charged whatever is held).
    `held`: it was granted -- mgs_ledger_hold reserves and checks in one step, so two forwards cannot both take the last
    room.  The charge ends with this object (also when an exception unwinds its frame) unless give() hands it to the
    workspace tensor, which then carries it until it is freed."""
    __slots__ = ("index", "nbytes", "held")

    def __init__(self, index, nbytes, budget):
        self.index, self.nbytes = index, int(nbytes)
        self.held = bool(_lib.lib().mgs_ledger_hold(index, self.nbytes, (1 << 63) - 1 if budget is None else int(budget)))

    def give(self, owner):
        if self.held:
            self.held = False
            weakref.finalize(owner, _unhold, self.index, self.nbytes)

    def drop(self):
        if self.held:
            self.held = False
            _unhold(self.index, self.nbytes)

    __del__ = drop


def set_headroom(instances: float = None, chunks: float = None):
    """Factors (>= 1) by which an asynchronous forward's instance list / chunk-record pool exceed the largest count seen."""
    for k, v in (("instances", instances), ("chunks", chunks)):
        if v is not None:
            _HEADROOM[k] = _headroom(v)
    _push_config()


_KEYS = {}  # marks key (tuple) -> MgsMarkKey


def _mark_key(key):
    """(P, W, H, F, tight_bins), ("views", V, P, W, H, F, tight_bins) or ("sets", S, V, P, W, H, F, tight_bins) as the ledger's
    key struct."""
    t = tuple(key)
    k = _KEYS.get(t)
    if k is None:
        if len(t) == 5:
            V, S, rest = 0, 0, t
        elif len(t) == 7 and t[0] == "views":
            V, S, rest = t[1], 0, t[2:]
        elif len(t) == 8 and t[0] == "sets":
            V, S, rest = t[2], t[1], t[3:]
        else:
            raise KeyError("a marks key is (P, W, H, F, tight_bins), ('views', V, P, W, H, F, tight_bins) or "
                           "('sets', S, V, P, W, H, F, tight_bins)")
        if len(_KEYS) > 4096:
            _KEYS.clear()
        k = _KEYS[t] = _lib.MgsMarkKey(int(V), int(S), *(int(x) for x in rest))
    return k


def _key_tuple(k):
    rest = (k.P, k.W, k.H, k.F, k.tight_bins)
    return rest if k.V == 0 else ("sets", k.S, k.V) + rest if k.S > 0 else ("views", k.V) + rest


class Pending:
    """One forward whose device report has not been read yet: the Python face of a ledger ticket."""
    __slots__ = ("a", "V", "slot_ptr", "key", "num_rendered", "chunks_used", "ref_rendered", "rc", "captured", "recoverable",
                 "recovered", "backward_enqueued", "words", "ticket", "_release")

    def __init__(self, a, V, slot_ptr, key, captured=False, recoverable=False):
        self.a, self.V, self.slot_ptr, self.key = a, V, slot_ptr, key
        self.words = _WORDS.get(slot_ptr)  # (numpy view of the status block, index of word 0) for a cheap "anything yet?"
        self.num_rendered = self.chunks_used = -1   # instances BINNED (what sizes a workspace), chunk records used
        self.ref_rendered = -1                      # the reference's num_rendered (3-sigma rects), status word 2
        self.rc = _lib.MGS_PENDING
        self.captured = captured
        self.recoverable = recoverable    # a backward will follow and can re-render (manigaussian_amd._C.recover_forward)
        self.recovered = False
        self.backward_enqueued = False    # ... but it has been enqueued on the incomplete state already
        self.ticket = None                # DeviceState.add: the ledger copies `a` as THIS run was given it

    def __del__(self):
        if self.ticket:
            self._release(self.ticket)

    def poll(self):
        """Non-blocking read of the status words; returns the library's code (MGS_PENDING until both words arrived)."""
        if self.rc != _lib.MGS_PENDING:
            return self.rc
        w = self.words
        if w is not None and w[0][w[1]] == -1 and w[0][w[1] + 1] == -1:  # both words still "pending": no call into the library
            return self.rc
        r = _lib.MgsReport()
        rc = _lib.lib().mgs_ledger_poll(self.ticket, r)
        if r.num_rendered >= 0:
            self.num_rendered = r.num_rendered
        if r.chunks_used >= 0:
            self.chunks_used = r.chunks_used
        if r.ref_rendered >= 0:
            self.ref_rendered = r.ref_rendered
        if rc != _lib.MGS_PENDING:
            self.rc = rc
        return rc

    def supersede(self):
        """A recovery has run this forward again (under a ticket of its own)."""
        self.recovered = True
        _lib.lib().mgs_ledger_superseded(self.ticket)

    def enqueue_backward(self):
        """Its backward has been enqueued before its report arrived: too late to repair."""
        self.backward_enqueued = True
        _lib.lib().mgs_ledger_backward_enqueued(self.ticket)


class _Marks(collections.abc.MutableMapping):
    """The marks of one device: ONE store, in the ledger, shared by the compiled binding's hot path and by this shim (a shape
    warmed up through either is known to both).  Values are [instances, chunk records or None] lists, copies -- assign to
    change one."""

    def __init__(self, index):
        self.index = index

    def __getitem__(self, key):
        v = self.get(key)
        if v is None:
            raise KeyError(key)
        return v

    def get(self, key, default=None):  # (the hot path's form: no exception for a new shape)
        R, chunks = ctypes.c_int64(), ctypes.c_int64()
        if _lib.lib().mgs_marks_get(self.index, _mark_key(key), R, chunks) != 1:
            return default
        return [R.value, None if chunks.value < 0 else chunks.value]

    def __contains__(self, key):
        return self.get(key) is not None

    def __setitem__(self, key, value):
        _lib.lib().mgs_marks_set(self.index, _mark_key(key), int(value[0]), -1 if value[1] is None else int(value[1]))

    def __delitem__(self, key):
        if _lib.lib().mgs_marks_erase(self.index, _mark_key(key)) != 1:
            raise KeyError(key)

    def __iter__(self):
        L = _lib.lib()
        n = L.mgs_marks_keys(self.index, None, 0)
        keys = (_lib.MgsMarkKey * max(n, 1))()
        n = min(n, L.mgs_marks_keys(self.index, keys, n))
        return iter([_key_tuple(keys[i]) for i in range(n)])

    def __len__(self):
        return _lib.lib().mgs_marks_keys(self.index, None, 0)


def _report(out, stacklevel):
    """Issue what a drain handed back (the texts live in the calling thread's storage until its next ledger call)."""
    error = out.error.decode() if out.error else None
    for text in [out.warnings[i].decode() for i in range(out.n_warnings)]:
        warnings.warn(text, RuntimeWarning, stacklevel=stacklevel)
    if error:
        raise RuntimeError(error)


_NO_SYNC_FN = _lib.LEDGER_SYNC_FN()  # NULL: the library synchronises by itself (the ctypes call has released the GIL)


_TLS = threading.local()  # .out: this thread's MgsLedgerOut (a drain runs in front of every forward)


def _drain(index, wait=False, stacklevel=5):
    try:
        out = _TLS.out
    except AttributeError:
        out = _TLS.out = _lib.MgsLedgerOut()
    _lib.lib().mgs_ledger_drain(index, int(wait), _NO_SYNC_FN, None, out)
    if out.error or out.n_warnings:
        _report(out, stacklevel)


class DeviceState:
    """The Python face of one device's ledger state."""

    def __init__(self, dev):
        self.dev = dev
        self.index = dev.index if dev.index is not None else torch.cuda.current_device()
        _push_config()
        L = _lib.lib()
        ring = L.mgs_ledger_ring(self.index, None, 0)
        if not ring:  # this binding is the first to touch the device: its pinned block becomes the device's ring
            self.status = torch.full((SLOT_WORDS * NSLOTS,), -1, dtype=torch.int64).pin_memory()
            ring = L.mgs_ledger_ring(self.index, self.status.data_ptr(), NSLOTS)
        self.base_ptr = ring
        n = L.mgs_ledger_ring_slots(self.index)
        words = numpy.frombuffer((ctypes.c_int64 * (SLOT_WORDS * n)).from_address(ring), dtype=numpy.int64)
        for i in range(n):
            _WORDS[ring + SLOT_BYTES * i] = (words, SLOT_WORDS * i)
        # shape key -> [instances high-water, chunk records high-water or None (unknown: worst case)]
        self.marks = _Marks(self.index)
        self.pending = collections.deque()  # this shim's forwards whose report had not arrived when last looked at
        self.captured = []   # forwards recorded into HIP graphs: their slots stay reserved, check_status() reads them
        self.deferred = collections.deque(maxlen=64)  # this shim's forwards that reported an overflow (diagnostics)
        self.lock = threading.Lock()  # (of `pending`: ctypes calls release the GIL)

    def take_slot(self):
        """(pointer to two pinned words, tag) for one forward."""
        slot, tag = ctypes.c_void_p(), ctypes.c_uint32()
        if _lib.lib().mgs_ledger_take_slot(self.index, slot, tag) != _lib.MGS_OK:
            raise RuntimeError(_lib.last_error())
        return slot.value, tag.value

    def add(self, pending):
        """Register a forward whose report is outstanding."""
        L = _lib.lib()
        flags = (_lib.TICKET_RECOVERABLE if pending.recoverable else 0) | (_lib.TICKET_CAPTURED if pending.captured else 0)
        pending._release = L.mgs_ledger_release
        pending.ticket = L.mgs_ledger_add(self.index, pending.a, pending.V, pending.slot_ptr, _mark_key(pending.key), flags)
        if not pending.ticket:
            raise RuntimeError(_lib.last_error())
        if pending.captured:
            self.captured.append(pending)
        else:
            with self.lock:
                self.pending.append(pending)

    # ---- high-water marks ---------------------------------------------------------------------------------------
    def guess(self, key):
        """(capacity, chunk pool) for an asynchronous forward of this shape, or None if the shape is new."""
        return self.guess_of(self.marks.get(key))

    @staticmethod
    def guess_of(m):
        """guess() from marks already read (a forward reads its shape's marks once).  Answered from the shim's cache of
        the library's plan (_lib.plan_capacity) and its own copy of the head-room, not by mgs_marks_guess: a warm forward
        makes no sizing call into the library, and a DeviceState over any mapping of marks can be asked."""
        if m is None or m[1] is None:
            return None
        return _lib.plan_capacity(_lib.SIZE_HEADROOM, 0, 0, m[0], m[1], _HEADROOM["instances"], _HEADROOM["chunks"])

    def learn(self, key, R=None, chunks=None, pool_unknown=False):
        _lib.lib().mgs_marks_learn(self.marks.index, _mark_key(key), -1 if R is None else int(R),
                                   -1 if chunks is None else int(chunks), int(pool_unknown))

    # ---- reports --------------------------------------------------------------------------------------------------
    def drain(self, wait=False):
        """Read every report of the device that has arrived, this shim's forwards and the compiled binding's alike (wait=True:
        all of them, synchronising with the device once if one is still outstanding).  Raises if a forward overflowed its
        workspace or finished without reporting."""
        try:
            _drain(self.index, wait)
        finally:
            if self.pending:
                with self.lock:
                    for _ in range(len(self.pending)):
                        p = self.pending.popleft()
                        rc = p.poll()
                        if rc == _lib.MGS_PENDING and not wait:
                            self.pending.append(p)
                        elif rc in (_lib.MGS_NEED_CAPACITY, _lib.MGS_RETRY_TABLE_INIT):
                            self.deferred.append(p)

    def check_captured(self):
        out = _lib.MgsLedgerOut()
        _lib.lib().mgs_ledger_check_captured(self.index, out)
        error = out.error.decode() if out.error else None  # (the texts live until this thread's next ledger call)
        for p in self.captured:  # every replay reports anew: refresh what the tools read, then raise
            p.rc = _lib.MGS_PENDING
            p.poll()
        if error:
            raise RuntimeError(error)


def device_state(dev) -> DeviceState:
    st = _STATES.get(dev)
    if st is None:
        with _LOCK:
            st = _STATES.get(dev)
            if st is None:
                st = DeviceState(dev)
                _STATES[dev] = st
    return st


def check_status(device=None, wait=True):
    """Read the outstanding forward reports of `device` (default: all devices used so far), waiting for them unless
    wait=False, and raise if one of them -- or a forward replayed from a captured HIP graph -- overflowed its workspace.
    A training loop calls this wherever it synchronises anyway (logging a loss, an optimizer step)."""
    L = _lib.lib()
    if device is None:
        indices = range(torch.cuda.device_count())
    else:
        d = torch.device(device)
        indices = [d.index if d.index is not None else torch.cuda.current_device()]
    for i in indices:
        st = _STATES.get(torch.device("cuda", i))
        if st is not None:
            st.drain(wait=wait)
            st.check_captured()
        elif L.mgs_ledger_ring(i, None, 0):  # only the compiled binding has used it (it captures nothing)
            _drain(i, wait)
