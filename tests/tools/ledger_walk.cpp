// Host-only sanitizer walk of the report ledger (csrc/mgs_ledger.hip): several threads add tickets, fill status words, drain,
// poll and release concurrently on ONE device whose ring is plain memory; then a single-thread pass over the lifetime of a
// ticket (released before and after it is accounted, superseded, never reporting, captured).  No device, no Python.
// Address + undefined-behaviour sanitizers, against the library's host objects (the real status-word decode of mgs_api.hip):
//   S="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all"
//   for f in manigaussian_amd/csrc/*.hip; do hipcc -O1 -std=c++17 --offload-arch=gfx950 -munsafe-fp-atomics $S -c $f -o $(basename $f .hip).o; done
//   hipcc -std=c++17 --offload-arch=gfx950 $S -c tests/tools/ledger_walk.cpp -o ledger_walk.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined *.o -o ledger_walk && ./ledger_walk
// Thread sanitizer: the walk's threads play the device, and the library's decode reads the words a device writes with plain
// volatile loads, which the sanitizer would report against any host writer; -DLEDGER_WALK_STANDIN_DECODE replaces the decode
// (and set_error / mgs_last_error, which live beside it) with the documented word layout read atomically:
//   S="-Xarch_host -fsanitize=thread"
//   hipcc -std=c++17 --offload-arch=gfx950 $S -c manigaussian_amd/csrc/mgs_plan.hip -o mgs_plan.o      (and mgs_ledger.hip)
//   hipcc -std=c++17 --offload-arch=gfx950 $S -DLEDGER_WALK_STANDIN_DECODE -c tests/tools/ledger_walk.cpp -o ledger_walk.o
//   hipcc -fsanitize=thread mgs_plan.o mgs_ledger.o ledger_walk.o -o ledger_walk && ./ledger_walk
// Exit status 1 if a count at the end is not what the walk must leave behind.
#include <stdio.h>
#include <string.h>

#include <atomic>
#include <thread>
#include <vector>

#include "../../include/mgsplat.h"

static const uint64_t kPending = ~0ull;
static void store(uint64_t* p, uint64_t v) { __atomic_store_n(p, v, __ATOMIC_RELEASE); }
static uint64_t word(uint32_t tag, uint32_t value, uint32_t flags = 0) { return ((uint64_t)tag << 48) | ((uint64_t)flags << 32) | value; }

#ifdef LEDGER_WALK_STANDIN_DECODE
static uint64_t load(const uint64_t* p) { return __atomic_load_n(p, __ATOMIC_ACQUIRE); }
namespace mgs { void set_error(const char*, ...) {} }
extern "C" const char* mgs_last_error(void) { return "(ledger_walk)"; }
extern "C" int mgs_forward_result(const MgsRasterArgs* a, const uint64_t* hs, int32_t* nr, int32_t* ch, int32_t* ref) {
  *nr = *ch = *ref = -1;
  const uint64_t w0 = load(hs), w1 = load(hs + 1), w2 = load(hs + 2);
  const auto arrived = [&](uint64_t w) { return w != kPending && (uint32_t)(w >> 48) == (a->status_tag & 0xffffu); };
  if (arrived(w0)) {
    *nr = (int32_t)(uint32_t)w0;
    if (arrived(w2)) *ref = (int32_t)(uint32_t)w2;
    if ((w0 >> 32) & 2u) return MGS_RETRY_TABLE_INIT;
    if (*nr > a->binning_capacity) return MGS_NEED_CAPACITY;
  }
  if (arrived(w1)) *ch = (int32_t)(uint32_t)w1;
  if (!arrived(w0) || !arrived(w1)) return MGS_PENDING;
  return ((w1 >> 32) & 1u) ? MGS_NEED_CAPACITY : MGS_OK;
}
extern "C" int mgs_forward_result_views(const MgsRasterArgs* a, int32_t, const uint64_t* hs, int32_t* nr, int32_t* ch, int32_t* ref) {
  return mgs_forward_result(a, hs, nr, ch, ref);
}
#endif

// (a ring that does not come round within the walk: a slot handed out again while its first holder is descheduled between its
//  forward and its report would have two writers, which no stream of a real device does to a slot within 1024 forwards)
static const int DEV = 3, THREADS = 4, STEPS = 4000, NSLOTS = 2 * THREADS * STEPS;
static const MgsMarkKey KEY = {0, 0, 1000, 64, 64, 3, 1};
static std::vector<uint64_t> g_ring((size_t)NSLOTS* MGS_LEDGER_SLOT_WORDS, kPending);
static std::atomic<long> g_errors{0}, g_warnings{0}, g_bad{0};

static void no_sync(void*) {}

static MgsTicket* forward(uint64_t** slot, uint32_t* tag, int flags, int capacity = 100) {
  if (mgs_ledger_take_slot(DEV, slot, tag) != MGS_OK) { g_bad++; return nullptr; }
  for (int i = 0; i < 3; i++) store(*slot + i, kPending);
  MgsRasterArgs a;
  memset(&a, 0, sizeof(a));
  a.P = 1000; a.W = a.H = 64; a.binning_capacity = capacity; a.chunk_pool = 10; a.binning_bytes = (size_t)1 << 40;
  a.status_tag = *tag; a.async_forward = 1;
  MgsTicket* t = mgs_ledger_add(DEV, &a, 0, *slot, &KEY, flags);
  if (!t) g_bad++;
  return t;
}
static void report(uint64_t* slot, uint32_t tag, uint32_t binned, uint32_t chunks, bool pool_overflow = false) {
  store(slot + 2, word(tag, binned + 7));
  store(slot, word(tag, binned));
  store(slot + 1, word(tag, chunks, pool_overflow ? 1 : 0));
}
static void drain(bool wait) {
  MgsLedgerOut out;
  if (mgs_ledger_drain(DEV, wait, &no_sync, nullptr, &out) != MGS_OK) g_bad++;
  if (out.error) g_errors += strlen(out.error) > 0;
  for (int i = 0; i < out.n_warnings; i++) g_warnings += strlen(out.warnings[i]) > 0;
}

static void worker(int id) {
  for (int i = 0; i < STEPS; i++) {
    uint64_t* slot;
    uint32_t tag;
    const bool recoverable = (i + id) % 3 == 0, grows = i % 97 == 5, pool = i % 89 == 7;
    MgsTicket* t = forward(&slot, &tag, recoverable ? MGS_TICKET_RECOVERABLE : 0);
    if (!t) return;
    if (i % 5 == 0) drain(false);                 // (its own report has not arrived: another thread's may have)
    if (i % 11 == 3) mgs_ledger_backward_enqueued(t);
    const bool early = i % 7 == 1;
    if (early) mgs_ledger_release(t);             // the holder lets go before the ledger has accounted it
    report(slot, tag, grows ? 500 + i % 50 : 10 + (i + id) % 80, 3 + i % 6, pool);
    MgsReport r;
    if (!early && mgs_ledger_poll(t, &r) == MGS_PENDING) g_bad++;
    if (mgs_ledger_hold(DEV, 100, 250)) mgs_ledger_unhold(DEV, 100);  // (at most two of the four threads at a time)
    drain(i % 13 == 0);
    int64_t R = 0, chunks = 0, cap = 0, pl = 0;
    if (mgs_marks_get(DEV, &KEY, &R, &chunks) == 1 && chunks >= 0 && mgs_marks_guess(DEV, &KEY, &cap, &pl) == 1 && cap < R) g_bad++;
    if (!early) {
      if (mgs_ledger_poll(t, &r) == MGS_PENDING) g_bad++;  // accounted or not, the holder's reference keeps it readable
      mgs_ledger_release(t);
    }
  }
}

int main() {
  if (mgs_ledger_ring(DEV, g_ring.data(), NSLOTS) != g_ring.data() || mgs_ledger_ring_slots(DEV) != NSLOTS) return 1;
  std::vector<std::thread> threads;
  for (int i = 0; i < THREADS; i++) threads.emplace_back(worker, i);
  for (std::thread& t : threads) t.join();
  drain(true);
  int64_t R = 0, chunks = 0;
  const int found = mgs_marks_get(DEV, &KEY, &R, &chunks);
  printf("ledger_walk: %d threads x %d forwards: %ld errors, %ld warnings; marks R=%lld chunks=%lld; outstanding %d, held %lld\n",
         THREADS, STEPS, g_errors.load(), g_warnings.load(), (long long)R, (long long)chunks, mgs_ledger_outstanding(DEV),
         (long long)mgs_ledger_held(DEV));
  // (the largest count a worker reports is 549; a forward that another thread's waiting drain dropped is never learned)
  bool ok = g_bad == 0 && found == 1 && R >= 500 && R <= 549 && mgs_ledger_outstanding(DEV) == 0 && mgs_ledger_held(DEV) == 0 &&
            g_errors > 0 && g_warnings > 0;

  // ---- one thread: the lifetime of a ticket ----
  const long errors0 = g_errors, warnings0 = g_warnings;
  uint64_t* slot;
  uint32_t tag;
  MgsReport r;
  MgsTicket* t = forward(&slot, &tag, 0);         // released before it is accounted: the ledger's reference carries it
  mgs_ledger_release(t);
  report(slot, tag, 20, 4);
  drain(false);
  t = forward(&slot, &tag, 0);                    // released after: still readable
  report(slot, tag, 30, 4);
  drain(false);
  ok = ok && mgs_ledger_poll(t, &r) == MGS_OK && r.num_rendered == 30 && r.chunks_used == 4 && r.ref_rendered == 37;
  mgs_ledger_release(t);
  t = forward(&slot, &tag, MGS_TICKET_RECOVERABLE);  // overflowed, re-run under another ticket, accounted once as a warning
  report(slot, tag, 900, 0);
  ok = ok && mgs_ledger_poll(t, &r) == MGS_NEED_CAPACITY;
  uint64_t* slot2;
  uint32_t tag2;
  MgsTicket* t2 = forward(&slot2, &tag2, 0, 2000);
  mgs_ledger_superseded(t);
  mgs_ledger_release(t);
  report(slot2, tag2, 900, 9);
  drain(false);
  drain(true);
  mgs_ledger_release(t2);
  ok = ok && g_errors == errors0 && g_warnings == warnings0 + 1 && mgs_ledger_outstanding(DEV) == 0;
  t = forward(&slot, &tag, 0);                    // never reports: fails the wait, is dropped, stays readable for its holder
  drain(true);
  ok = ok && g_errors == errors0 + 1 && mgs_ledger_poll(t, &r) == MGS_PENDING && mgs_ledger_outstanding(DEV) == 0;
  mgs_ledger_release(t);
  t = forward(&slot, &tag, MGS_TICKET_CAPTURED);  // captured: the ledger keeps it (and its slot) for good
  mgs_ledger_release(t);
  report(slot, tag, 40, 4);
  MgsLedgerOut out;
  ok = ok && mgs_ledger_check_captured(DEV, &out) == MGS_OK && !out.error && out.n_warnings == 0;
  for (int i = 0; i < NSLOTS + 8; i++) {
    uint64_t* s;
    ok = ok && mgs_ledger_take_slot(DEV, &s, &tag) == MGS_OK && s != slot;
  }
  ok = ok && g_bad == 0 && mgs_marks_get(DEV, &KEY, &R, &chunks) == 1 && R == 900;
  printf("ledger_walk: %s\n", ok ? "OK" : "FAILED");
  return ok ? 0 : 1;
}
