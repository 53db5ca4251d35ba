// mgs_ledger.hip -- WHO IS OUTSTANDING, WHAT WAS LEARNED, WHAT TO SAY: the host-side accounting of the asynchronous forward
// (include/mgsplat.h "the report ledger"), once, for every host binding that loads this library.  Per device: the ring of status
// slots, the high-water marks per shape, the forwards whose device report has not been folded into the marks, the budget of
// worst-case workspaces -- and every overflow / hand-shake message.  Plain host C++: no kernel, no torch, no Python; the one HIP
// call is the device synchronisation of a drain whose caller gave no function for it.  Each device has ONE mutex, a leaf lock:
// nothing is called while it is held except the status-word decode (mgs_forward_result*) and the plan's arithmetic.
#include <algorithm>
#include <atomic>
#include <deque>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "mgs_common.h"

using namespace mgs;

struct MgsTicket {
  MgsRasterArgs a;  // as given to THIS run (status_tag, binning_capacity, chunk_pool, binning_bytes, the shape)
  int32_t V = 0;
  const uint64_t* slot = nullptr;
  MgsMarkKey key{};
  int device = 0, flags = 0;
  MgsReport report{MGS_PENDING, -1, -1, -1};
  std::string decode_error;  // mgs_last_error() of the decode that failed (the thread that accounts may be another)
  bool superseded = false, backward_enqueued = false;
  std::atomic<int> refs{2};  // the ledger's (while outstanding or captured) and the holder's
};

namespace {

struct KeyHash {
  size_t operator()(const MgsMarkKey& k) const {
    uint64_t h = 0x9e3779b97f4a7c15ull;
    for (int32_t v : {k.V, k.S, k.P, k.W, k.H, k.F, k.tight_bins}) h = (h ^ (uint64_t)(uint32_t)v) * 0x100000001b3ull + 0x632be59bd9b4e019ull;
    return (size_t)h;
  }
};
struct KeyEq {
  bool operator()(const MgsMarkKey& a, const MgsMarkKey& b) const {
    return a.V == b.V && a.S == b.S && a.P == b.P && a.W == b.W && a.H == b.H && a.F == b.F && a.tight_bins == b.tight_bins;
  }
};
struct Mark { int64_t R = 0, chunks = -1; };  // chunks < 0: unknown (worst-case pool)

struct Device {
  std::mutex mu;
  uint64_t* ring = nullptr;
  int nslots = 0, next_slot = 0;
  uint32_t tag = 0;
  std::vector<bool> reserved;  // slots of captured tickets
  std::unordered_map<MgsMarkKey, Mark, KeyHash, KeyEq> marks;
  std::deque<MgsTicket*> outstanding;
  std::vector<MgsTicket*> captured;
  std::atomic<int64_t> held{0};
};
Device* const g_dev = new Device[MGS_LEDGER_MAX_DEVICES];  // never destroyed: a thread may still drain while the process exits

std::mutex g_cfg_mu;
MgsLedgerConfig g_cfg = {0, 0, 1.5, 2.0, -1};

// what a drain hands back: valid until this thread's next ledger call
thread_local std::string t_error;
thread_local std::vector<std::string> t_warnings;
thread_local std::vector<const char*> t_warning_ptrs;

Device* device(int index, const char* fn) {
  if (index >= 0 && index < MGS_LEDGER_MAX_DEVICES) return &g_dev[index];
  set_error("%s: device index %d (0 .. %d)", fn, index, MGS_LEDGER_MAX_DEVICES - 1);
  return nullptr;
}

void unref(MgsTicket* t) {
  if (t->refs.fetch_sub(1) == 1) delete t;
}

void publish(MgsLedgerOut* out) {
  t_warning_ptrs.clear();
  for (const std::string& w : t_warnings) t_warning_ptrs.push_back(w.c_str());
  out->error = t_error.empty() ? nullptr : t_error.c_str();
  out->n_warnings = (int32_t)t_warning_ptrs.size();
  out->warnings = t_warning_ptrs.data();
}

// ---- (device mutex held from here to the end of the namespace) ----
void learn(Device& d, const MgsMarkKey& k, int64_t R, int64_t chunks, bool pool_unknown) {
  Mark& m = d.marks[k];
  if (R > m.R) m.R = R;  // the marks only grow ...
  if (pool_unknown) m.chunks = -1;  // ... but a pool that overflowed says nothing about the pool that would have fit
  else if (chunks > m.chunks) m.chunks = chunks;
}

int poll(MgsTicket& t) {
  MgsReport& r = t.report;
  if (r.rc != MGS_PENDING || t.superseded) return r.rc;
  int32_t nr = -1, ch = -1, ref = -1;
  const int rc = t.V ? mgs_forward_result_views(&t.a, t.V, t.slot, &nr, &ch, &ref) : mgs_forward_result(&t.a, t.slot, &nr, &ch, &ref);
  if (nr >= 0) r.num_rendered = nr;
  if (ch >= 0) r.chunks_used = ch;
  if (ref >= 0) r.ref_rendered = ref;
  if (rc != MGS_PENDING) r.rc = rc;
  if (rc < 0) t.decode_error = mgs_last_error();
  return rc;
}

const char* const kOutgrew = "an asynchronous rasterizer forward outgrew the workspace sized from earlier calls of the same shape";
const char* const kHandshake = "an asynchronous rasterizer forward's preprocess gave up waiting for its zeroed tile tables (a workgroup "
                               "of the launch made no progress for about a second) and binned nothing";
const char* const kSafeMode = "manigaussian_amd.set_forward_mode('safe') (the default)";
const char* const kTableInit = "manigaussian_amd.set_options(table_init=1) removes the hand-shake";

// Fold a finished forward into the marks; the text the caller must raise, or "" (warnings go to t_warnings).
std::string account(Device& d, MgsTicket& t, int rc, int policy) {
  const MgsReport& r = t.report;
  if (rc == MGS_OK) { learn(d, t.key, r.num_rendered, r.chunks_used, false); return ""; }
  if (rc != MGS_NEED_CAPACITY && rc != MGS_RETRY_TABLE_INIT)
    return "rasterizer forward failed: " + t.decode_error + " (code " + std::to_string(rc) + ")";
  const bool grew = rc == MGS_NEED_CAPACITY;
  std::string msg;
  if (grew) {
    const int cap = t.a.binning_capacity;
    const bool over_inst = r.num_rendered > cap && cap > 0;
    learn(d, t.key, r.num_rendered, -1, !over_inst);
    msg = std::string(kOutgrew) + " (" +
          (over_inst ? std::to_string(r.num_rendered) + " (Gaussian, tile) instances > capacity " + std::to_string(cap)
                     : "chunk pool of " + std::to_string(t.a.chunk_pool) + " records") +
          "): the images of THAT call were incomplete.  The marks are raised";
  } else {  // nothing to learn: the scene did not grow, a workgroup of the preprocess launch was held back
    msg = std::string(kHandshake) + ": the images of THAT call were incomplete";
  }
  const bool repairable = (t.flags & MGS_TICKET_RECOVERABLE) && !(t.flags & MGS_TICKET_CAPTURED) && !t.backward_enqueued;
  if (t.superseded || (policy == MGS_OVERFLOW_REPAIR && repairable)) {
    // its backward re-renders first: the gradients come from a complete forward; only what the caller computed from the
    // incomplete images in between cannot be repaired
    t_warnings.push_back(msg + "; the call's backward re-renders on the blocking path before it runs, but a loss computed from "
                               "those images was computed from incomplete images.  " +
                         (grew ? std::string("For scenes that grow abruptly use ") + kSafeMode + " or a larger set_headroom()."
                               : std::string(kTableInit) + "."));
    return "";
  }
  if (repairable) {       // overflow policy "raise"
    t.superseded = true;  // its backward, if it still comes, raises too (mgs_ledger_lost_step_message)
    return msg + "; the step is lost (overflow policy 'raise'): re-run it" +
           (grew ? std::string(", or use ") + kSafeMode + " for scenes that grow abruptly." : ".");
  }
  return msg + " and its gradients were computed on the incomplete state; re-run the step" +
         (grew ? std::string(", or use ") + kSafeMode + " for scenes that grow abruptly." : std::string(" (") + kTableInit + ").");
}

}  // namespace

extern "C" {

void mgs_ledger_set_config(const MgsLedgerConfig* c) {
  if (!c) return;
  std::lock_guard<std::mutex> lk(g_cfg_mu);
  g_cfg = *c;
}
void mgs_ledger_get_config(MgsLedgerConfig* c) {
  if (!c) return;
  std::lock_guard<std::mutex> lk(g_cfg_mu);
  *c = g_cfg;
}

// ---- the ring ----
uint64_t* mgs_ledger_ring(int dev, uint64_t* words, int nslots) {
  Device* d = device(dev, "mgs_ledger_ring");
  if (!d) return nullptr;
  std::lock_guard<std::mutex> lk(d->mu);
  if (!d->ring && words && nslots > 0) {
    d->ring = words;
    d->nslots = nslots;
    d->reserved.assign((size_t)nslots, false);
  }
  return d->ring;
}
int mgs_ledger_ring_slots(int dev) {
  Device* d = device(dev, "mgs_ledger_ring_slots");
  if (!d) return 0;
  std::lock_guard<std::mutex> lk(d->mu);
  return d->nslots;
}
int mgs_ledger_take_slot(int dev, uint64_t** slot, uint32_t* tag) {
  Device* d = device(dev, "mgs_ledger_take_slot");
  if (!d) return MGS_ERR_INVALID_ARG;
  if (!slot || !tag) { set_error("mgs_ledger_take_slot: an output is NULL"); return MGS_ERR_INVALID_ARG; }
  std::lock_guard<std::mutex> lk(d->mu);
  for (int tries = 0; tries < d->nslots; tries++) {
    const int i = d->next_slot;
    d->next_slot = (i + 1) % d->nslots;
    if (d->reserved[(size_t)i]) continue;
    d->tag = (d->tag + 1) & 0xffffu;  // (unique per in-flight forward of this device is all that is needed)
    *slot = d->ring + (size_t)i * MGS_LEDGER_SLOT_WORDS;
    *tag = d->tag;
    return MGS_OK;
  }
  if (d->ring) set_error("all status slots are held by captured graphs");
  else set_error("mgs_ledger_take_slot: device %d has no status ring", dev);
  return MGS_ERR_INVALID_ARG;
}

// ---- the marks ----
int mgs_marks_get(int dev, const MgsMarkKey* key, int64_t* R, int64_t* chunks) {
  Device* d = device(dev, "mgs_marks_get");
  if (!d || !key) return MGS_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(d->mu);
  auto it = d->marks.find(*key);
  if (it == d->marks.end()) return 0;
  if (R) *R = it->second.R;
  if (chunks) *chunks = it->second.chunks;
  return 1;
}
int mgs_marks_set(int dev, const MgsMarkKey* key, int64_t R, int64_t chunks) {
  Device* d = device(dev, "mgs_marks_set");
  if (!d || !key) return MGS_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(d->mu);
  d->marks[*key] = Mark{R, chunks < 0 ? -1 : chunks};
  return MGS_OK;
}
int mgs_marks_erase(int dev, const MgsMarkKey* key) {
  Device* d = device(dev, "mgs_marks_erase");
  if (!d || !key) return MGS_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(d->mu);
  return d->marks.erase(*key) != 0;
}
int mgs_marks_keys(int dev, MgsMarkKey* out, int room) {
  Device* d = device(dev, "mgs_marks_keys");
  if (!d) return MGS_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(d->mu);
  int n = 0;
  for (const auto& kv : d->marks) {
    if (out && n < room) out[n] = kv.first;
    n++;
  }
  return n;
}
int mgs_marks_learn(int dev, const MgsMarkKey* key, int64_t R, int64_t chunks, int pool_unknown) {
  Device* d = device(dev, "mgs_marks_learn");
  if (!d || !key) return MGS_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(d->mu);
  learn(*d, *key, R, chunks, pool_unknown != 0);
  return MGS_OK;
}
int mgs_marks_guess(int dev, const MgsMarkKey* key, int64_t* capacity, int64_t* chunk_pool) {
  Device* d = device(dev, "mgs_marks_guess");
  if (!d || !key) return MGS_ERR_INVALID_ARG;
  MgsLedgerConfig c;
  mgs_ledger_get_config(&c);
  Mark m;
  {
    std::lock_guard<std::mutex> lk(d->mu);
    auto it = d->marks.find(*key);
    if (it == d->marks.end() || it->second.chunks < 0) return 0;  // no guess without a chunk mark
    m = it->second;
  }
  const MgsPlanShape any = {0, 0, 0, 1, 1, 0, 0, 0};  // (the head-room rule does not look at the shape)
  return mgs_plan_capacity(&any, MGS_SIZE_HEADROOM, m.R, m.chunks, c.head_instances, c.head_chunks, capacity, chunk_pool) == MGS_OK;
}

// ---- the budget ----
int mgs_ledger_hold(int dev, int64_t bytes, int64_t budget) {
  Device* d = device(dev, "mgs_ledger_hold");
  if (!d || bytes < 0) return 0;
  if (d->held.fetch_add(bytes) + bytes <= budget) return 1;  // reserved first, then checked: two callers cannot both pass
  d->held.fetch_sub(bytes);
  return 0;
}
void mgs_ledger_unhold(int dev, int64_t bytes) {
  if (Device* d = device(dev, "mgs_ledger_unhold")) d->held.fetch_sub(bytes);
}
int64_t mgs_ledger_held(int dev) {
  Device* d = device(dev, "mgs_ledger_held");
  return d ? d->held.load() : 0;
}

// ---- tickets ----
MgsTicket* mgs_ledger_add(int dev, const MgsRasterArgs* a, int32_t V, const uint64_t* slot, const MgsMarkKey* key, int flags) {
  Device* d = device(dev, "mgs_ledger_add");
  if (!d) return nullptr;
  if (!a || !slot || !key || V < 0) { set_error("mgs_ledger_add: bad argument"); return nullptr; }
  MgsTicket* t = new MgsTicket();
  t->a = *a; t->V = V; t->slot = slot; t->key = *key; t->device = dev; t->flags = flags;
  std::lock_guard<std::mutex> lk(d->mu);
  if (flags & MGS_TICKET_CAPTURED) {  // reports at every replay: its slot is never handed out again
    d->captured.push_back(t);
    const ptrdiff_t i = d->ring ? (slot - d->ring) / MGS_LEDGER_SLOT_WORDS : -1;
    if (i >= 0 && i < d->nslots) d->reserved[(size_t)i] = true;
  } else {
    d->outstanding.push_back(t);
  }
  return t;
}
int mgs_ledger_poll(MgsTicket* t, MgsReport* report) {
  if (!t) { set_error("mgs_ledger_poll: ticket is NULL"); return MGS_ERR_INVALID_ARG; }
  std::lock_guard<std::mutex> lk(g_dev[t->device].mu);
  const int rc = poll(*t);
  if (report) { *report = t->report; report->rc = rc; }
  return rc;
}
void mgs_ledger_backward_enqueued(MgsTicket* t) {
  if (!t) return;
  std::lock_guard<std::mutex> lk(g_dev[t->device].mu);
  t->backward_enqueued = true;
}
void mgs_ledger_superseded(MgsTicket* t) {
  if (!t) return;
  std::lock_guard<std::mutex> lk(g_dev[t->device].mu);
  t->superseded = true;
}
void mgs_ledger_release(MgsTicket* t) {
  if (t) unref(t);
}
int mgs_ledger_outstanding(int dev) {
  Device* d = device(dev, "mgs_ledger_outstanding");
  if (!d) return 0;
  std::lock_guard<std::mutex> lk(d->mu);
  return (int)d->outstanding.size();
}

// ---- reports ----
int mgs_ledger_drain(int dev, int wait, void (*sync_fn)(void*), void* ctx, MgsLedgerOut* out) {
  t_error.clear();
  t_warnings.clear();
  if (out) publish(out);
  Device* d = device(dev, "mgs_ledger_drain");
  if (!d || !out) return MGS_ERR_INVALID_ARG;
  MgsLedgerConfig cfg;
  mgs_ledger_get_config(&cfg);
  // tickets that were outstanding when the device was synchronised, by reference: another thread's drain may account and
  // free one in the meantime, and a ticket added AFTER the synchronisation may be allocated at that very address
  std::vector<MgsTicket*> must_finish;
  {
    std::lock_guard<std::mutex> lk(d->mu);
    if (d->outstanding.empty()) return MGS_OK;
    const size_t n = d->outstanding.size();
    size_t kept = 0;
    for (size_t i = 0; i < n; i++) {
      MgsTicket* t = d->outstanding[i];
      if (poll(*t) != MGS_PENDING || t->superseded) continue;
      // synchronise only if asked to, or if more than half the ring is outstanding (a slot must not come round again unread)
      if (wait || (n - i - 1) + kept >= (size_t)d->nslots / 2) { t->refs++; must_finish.push_back(t); }
      else kept++;
    }
  }
  if (!must_finish.empty()) {  // everything enqueued so far has run after this: a report that is still missing never comes
    if (sync_fn) {
      sync_fn(ctx);
    } else {
      int cur = -1;
      (void)hipGetDevice(&cur);
      if (cur != dev) (void)hipSetDevice(dev);
      (void)hipDeviceSynchronize();
      if (cur != dev && cur >= 0) (void)hipSetDevice(cur);
    }
  }
  {
    std::lock_guard<std::mutex> lk(d->mu);
    std::deque<MgsTicket*> keep;
    for (MgsTicket* t : d->outstanding) {
      const int rc = poll(*t);
      if (rc == MGS_PENDING) {
        if (std::find(must_finish.begin(), must_finish.end(), t) != must_finish.end()) {
          if (t_error.empty()) t_error = "a rasterizer forward finished without reporting its instance count";
        } else if (!t->superseded) {
          keep.push_back(t);  // (added in the meantime, or not yet due)
          continue;
        }
      } else {
        std::string f = account(*d, *t, rc, cfg.overflow_policy);
        if (t_error.empty()) t_error = std::move(f);
      }
      unref(t);  // accounted once: no longer the ledger's
    }
    d->outstanding.swap(keep);
  }
  for (MgsTicket* t : must_finish) unref(t);
  publish(out);
  return MGS_OK;
}

int mgs_ledger_check_captured(int dev, MgsLedgerOut* out) {
  t_error.clear();
  t_warnings.clear();
  if (out) publish(out);
  Device* d = device(dev, "mgs_ledger_check_captured");
  if (!d || !out) return MGS_ERR_INVALID_ARG;
  MgsLedgerConfig cfg;
  mgs_ledger_get_config(&cfg);
  {
    std::lock_guard<std::mutex> lk(d->mu);
    for (MgsTicket* t : d->captured) {
      t->report.rc = MGS_PENDING;  // every replay reports anew
      const int rc = poll(*t);
      if (rc == MGS_OK || rc == MGS_PENDING) continue;
      std::string f = account(*d, *t, rc, cfg.overflow_policy);
      if (!f.empty()) t_error = std::move(f);
    }
  }
  publish(out);
  return MGS_OK;
}

const char* mgs_ledger_lost_step_message(int rc) {
  static const std::string grew =
      "the asynchronous rasterizer forward of this backward outgrew its workspace (the scene grew past the head-room over earlier "
      "calls of its shape): its images are incomplete and the step is lost; the next call of the shape gets a larger workspace "
      "(overflow policy 'raise')";
  static const std::string handshake = std::string(kHandshake) + ": its images are incomplete and the step is lost (overflow policy 'raise')";
  return (rc == MGS_RETRY_TABLE_INIT ? handshake : grew).c_str();
}

}  // extern "C"
