// mgs_api.hip -- the C ABI of libmgsplat.so (declared in include/mgsplat.h): argument validation,
// workspace carving, stage sequencing on the caller's stream.  No torch, no global device state.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <atomic>
#include <mutex>
#include <utility>
#include <vector>

#include "mgs_common.h"

namespace mgs {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int launch_done(const char* fn) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { set_error("%s: %s", fn, hipGetErrorString(e)); return MGS_ERR_HIP; }
  return MGS_OK;
}

bool misaligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) != 0; }

int workspace_short(const char* fn, size_t have, size_t need) {
  if (have >= need) return MGS_OK;
  set_error("%s: workspace of %zu bytes, %zu needed", fn, have, need);
  return MGS_ERR_WORKSPACE;
}

// Nonces of the preprocess's table hand-shake: a process-wide counter under a per-process random word, never 0.  Not
// option state and not device state: two calls never share a value, that is all.
unsigned long long next_nonce() {
  static std::atomic<unsigned long long> counter{0};
  static const unsigned long long salt = [] {
    unsigned long long v = 0x9e3779b97f4a7c15ull ^ (unsigned long long)(uintptr_t)&counter;
    FILE* f = fopen("/dev/urandom", "rb");
    if (f) { unsigned long long r = 0; if (fread(&r, sizeof(r), 1, f) == 1) v ^= r; fclose(f); }
    return v << 32;
  }();
  const unsigned long long c = counter.fetch_add(1) + 1;
  const unsigned long long n = salt ^ c ^ (c << 40);
  return n ? n : 1ull;
}

static int g_profile = 0;  // diagnostics only (mgs_set_option("profile", .)): never results or layouts
int profile_level() { return g_profile; }

// MgsOptions of a call with the defaults filled in
static Options options_of(const MgsRasterArgs* a) {
  Options o;
  if (a && a->opt.set) {
    o.tight_bins = a->opt.tight_bins; o.fast_exp = a->opt.fast_exp; o.exact_cull = a->opt.exact_cull;
    o.bin_mode = (a->opt.bin_mode >= 0 && a->opt.bin_mode <= 2) ? a->opt.bin_mode : 2; o.gm_waves = (a->opt.gm_waves == 8 || a->opt.gm_waves == 16) ? a->opt.gm_waves : 12; o.dbg = a->opt.dbg;
    o.seg = (a->opt.seg == 512 || a->opt.seg == 1024 || a->opt.seg == 4096) ? a->opt.seg : 2048;
    o.table_init = a->opt.table_init ? 1 : 0;
  }
  if (a && a->debug) o.table_init = 1;  // a debugged device may hold any workgroup: no workgroup waits for another
  return o;
}

static bool supported_F(int F) {
  switch (F) {
    case 0: case 3: case 4: case 8: case 16: case 32: case 64: return true;
    default: return false;
  }
}

// ---- per-stage timing with hipEvents on the caller's stream (mgs_set_option("profile", 1|2)) ----
enum Stage { ST_PREPROCESS = 0, ST_RENDER_FWD, ST_BWD_MEMSET, ST_RENDER_BWD, ST_PREPROCESS_BWD, ST_BIN_SCATTER, ST_BIN_SEGSORT,
             ST_BIN_MERGE, ST_COUNT };
// (bin_scatter covers the table kernel too when the tables live in memory)
static const char* const kStageNames[ST_COUNT] = {"preprocess_fwd", "render_fwd", "bwd_memset", "render_bwd",
                                                  "preprocess_bwd", "bin_scatter", "bin_segsort", "bin_merge"};
struct Profiler {
  std::mutex mu;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> used[ST_COUNT];
  std::vector<hipEvent_t> pool;
  hipEvent_t get() {
    if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
  }
};
static Profiler& profiler() { static Profiler p; return p; }

struct StageTimer {  // RAII: records start now, stop at scope exit
  int stage; hipStream_t stream; hipEvent_t e0 = nullptr, e1 = nullptr;
  StageTimer(int st, hipStream_t s) : stage(st), stream(s) {
    const int lvl = g_profile;
    if (lvl == 0 || (lvl == 1 && st != ST_RENDER_BWD)) return;
    Profiler& p = profiler();
    std::lock_guard<std::mutex> lk(p.mu);
    e0 = p.get(); e1 = p.get();
    if (e0 && e1) (void)hipEventRecord(e0, stream); else e0 = e1 = nullptr;
  }
  ~StageTimer() {
    if (!e0) return;
    (void)hipEventRecord(e1, stream);
    Profiler& p = profiler();
    std::lock_guard<std::mutex> lk(p.mu);
    p.used[stage].push_back({e0, e1});
  }
};

#define MGS_HIP(expr, what)                                                      \
  do {                                                                           \
    hipError_t _e = (expr);                                                      \
    if (_e != hipSuccess) {                                                      \
      set_error("%s failed: %s", what, hipGetErrorString(_e));                   \
      return MGS_ERR_HIP;                                                        \
    }                                                                            \
  } while (0)

// debug=1: synchronise and check after a stage (RAST auxiliary.h:166-173 CHECK_CUDA)
#define MGS_STAGE(expr, what, dbg, stream)                                       \
  do {                                                                           \
    MGS_HIP(expr, what);                                                         \
    if (dbg) MGS_HIP(hipStreamSynchronize(stream), what " (debug sync)");        \
  } while (0)

static int check_common(const MgsRasterArgs* a) {
  if (!a) { set_error("args is NULL"); return MGS_ERR_INVALID_ARG; }
  if (a->P < 0 || a->W <= 0 || a->H <= 0) { set_error("bad P/W/H (%d,%d,%d)", a->P, a->W, a->H); return MGS_ERR_INVALID_ARG; }
  if (a->P > 0) {
    if (!a->means3D || !a->viewmatrix || !a->projmatrix || !a->campos || !a->background) {
      set_error("means3D/viewmatrix/projmatrix/campos/background must be non-NULL");
      return MGS_ERR_INVALID_ARG;
    }
    if ((a->shs == nullptr) == (a->colors_precomp == nullptr)) {
      // the reference hard-codes NUM_CHANNELS = 3; with neither it throws (rasterizer_impl.cu:245-248)
      set_error(a->shs ? "both shs and colors_precomp given" : "For non-RGB, provide precomputed Gaussian colors!");
      return a->shs ? MGS_ERR_INVALID_ARG : MGS_ERR_NON_RGB;
    }
    if (a->shs && a->M <= 0) { set_error("shs given but M <= 0"); return MGS_ERR_INVALID_ARG; }
    if (a->shs && (a->D < 0 || (a->D + 1) * (a->D + 1) > a->M || a->D > 3)) {
      set_error("sh_degree %d needs %d coefficients, M = %d (max degree 3)", a->D, (a->D + 1) * (a->D + 1), a->M);
      return MGS_ERR_INVALID_ARG;
    }
    const bool sr = a->scales && a->rotations;
    if (sr == (a->cov3D_precomp != nullptr) || (!sr && (a->scales || a->rotations))) {
      set_error("provide exactly one of scales+rotations or cov3D_precomp");
      return MGS_ERR_INVALID_ARG;
    }
    if (a->include_feature) {
      if (!a->language_feature) { set_error("include_feature set but language_feature is NULL"); return MGS_ERR_INVALID_ARG; }
      if (!supported_F(a->F) || a->F == 0) {
        set_error("feature width F=%d not compiled in (supported: 3,4,8,16,32,64; pad to the next one)", a->F);
        return MGS_ERR_INVALID_ARG;
      }
      // the render forward addresses feature rows by 32-bit byte offsets (buffer loads)
      if ((unsigned long long)a->P * (unsigned long long)a->F * 4ull >= (1ull << 32)) {
        set_error("P * F * 4 = %llu bytes of features: rows are addressed by 32-bit offsets (< 4 GiB)",
                  (unsigned long long)a->P * (unsigned long long)a->F * 4ull);
        return MGS_ERR_INVALID_ARG;
      }
    }
  }
  return MGS_OK;
}

}  // namespace mgs

using namespace mgs;

extern "C" {

int mgs_abi_version(void) { return MGS_ABI_VERSION; }
#ifndef MGS_BUILD_ID
#define MGS_BUILD_ID "unknown"
#endif
const char* mgs_build_id(void) { return MGS_BUILD_ID; }
const char* mgs_last_error(void) { return g_err; }

void mgs_options_default(MgsOptions* o) {
  if (!o) return;
  const Options d;
  o->set = 1; o->tight_bins = d.tight_bins; o->fast_exp = d.fast_exp; o->exact_cull = d.exact_cull;
  o->bin_mode = d.bin_mode; o->seg = d.seg; o->gm_waves = d.gm_waves; o->dbg = d.dbg; o->table_init = d.table_init;
}

int mgs_set_option(const char* key, int value) {
  if (!strcmp(key, "profile")) { g_profile = value; return MGS_OK; }
  set_error("unknown option %s (tuning switches are per call: MgsRasterArgs.opt)", key);
  return MGS_ERR_INVALID_ARG;
}
int mgs_get_option(const char* key) {
  if (!strcmp(key, "profile")) return g_profile;
  set_error("unknown option %s", key);
  return MGS_ERR_INVALID_ARG;
}

// the bin scatter keeps its per-tile tables in LDS; larger tile grids (or bin_mode 0) keep them in memory
static bool lds_tables(const Options& o, int T) { return o.bin_mode >= 1 && T <= LDS_TILES; }
// ... and the lists are ordered by ONE bucket-rank launch (bin_mode 2) instead of segment sort + rank merge
static bool bucket_rank(const Options& o, int T) { return o.bin_mode == 2 && T <= LDS_TILES; }

static Pass pass_of(const MgsRasterArgs* a, int V = 0, const MgsView* views = nullptr, int S = 1,
                    const int32_t* view_set = nullptr) {
  return pass_of(a->P, a->W, a->H, a->include_feature ? a->F : 0, V, views, S, view_set);
}
// first row of view v's Gaussian set in the stacked attribute tables
static int set_row(const Pass& s, int v) { return s.view_set ? s.view_set[v] * s.Pg : 0; }

static const uint64_t kStatusPending = ~0ull;

// How the caller carved the binning workspace: {instances it holds, chunk records}.  Explicit (binning_capacity > 0) or,
// for a buffer sized by mgs_binning_bytes, the largest count that fits with a worst-case pool.
struct BinShape { int cap; uint32_t pool; };
static int binning_capacity_uncached(size_t bytes, int T, int F) {
  auto need = [&](int R) { return binning_bytes_T(R, 0, T, F); };
  if (need(0) > bytes) return -1;
  int lo = 0, hi = 1;
  while (hi < (1 << 30) && need(hi) <= bytes) { lo = hi; hi <<= 1; }
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    if (need(mid) <= bytes) lo = mid; else hi = mid;
  }
  return lo;
}
static BinShape bin_shape(const MgsRasterArgs* a, int T, int F) {
  BinShape s = {-1, 0};
  if (a->binning_capacity > 0) {
    if (binning_bytes_T(a->binning_capacity, a->chunk_pool, T, F) > a->binning_bytes) return s;
    s.cap = a->binning_capacity;
    s.pool = a->chunk_pool > 0 ? (uint32_t)a->chunk_pool : chunk_pool_max((size_t)s.cap, T);
    return s;
  }
  struct Memo { size_t bytes; int T, F, cap; };
  static thread_local Memo memo = {0, -1, -1, -1};
  if (!(memo.bytes == a->binning_bytes && memo.T == T && memo.F == F))
    memo = {a->binning_bytes, T, F, binning_capacity_uncached(a->binning_bytes, T, F)};
  s.cap = memo.cap;
  s.pool = s.cap >= 0 ? chunk_pool_max((size_t)(s.cap > 0 ? s.cap : 1), T) : 0u;
  return s;
}
static int check_binning(const MgsRasterArgs* a, const BinShape& bs, int R) {
  if (!a->binning || bs.cap < 0) { set_error("binning workspace missing or smaller than its fixed part"); return MGS_ERR_WORKSPACE; }
  if (R > bs.cap) {
    set_error("binning workspace too small: %zu bytes hold %d instances, need %d", a->binning_bytes, bs.cap, R);
    return MGS_ERR_WORKSPACE;
  }
  return MGS_OK;
}

// Direct binning (mgs_common.h): where the forward preprocess of THIS call may write its keys -- inside the caller's binning
// workspace: the two key arrays if the capacity covers T * Pg keys (the worst-case workspaces of the default forward mode do),
// else bytes the caller added behind the carved arrays (mgs_binning_direct_extra); nullptr: the bin scatter kernel writes
// compact slices as before.  MgsOptions.dbg & 32768 switches it off (A/B).
static uint64_t* direct_region(const MgsRasterArgs* a, const BinShape& bs, const Pass& s, const Options& o) {
  if (!bucket_rank(o, s.T) || (o.dbg & 32768)) return nullptr;
  const size_t need = direct_keys_needed((size_t)s.P, s.V, s.T);
  if (!need) return nullptr;
  size_t total = 0;
  const BinView b = carve_binning(a->binning, bs.cap, s.T, s.F, bs.pool, nullptr, &total);
  const size_t span = (size_t)(reinterpret_cast<const char*>(b.point_list) - reinterpret_cast<const char*>(b.keys_unsorted));
  if (span >= need * sizeof(uint64_t)) return b.keys_unsorted;  // (the sorted-key array is unused by the bucket rank)
  const size_t off = (total + 255) & ~(size_t)255;
  if (need <= DIRECT_MAX_KEYS && a->binning_bytes >= off + need * sizeof(uint64_t))
    return reinterpret_cast<uint64_t*>(static_cast<char*>(a->binning) + off);
  return nullptr;
}

// The geom and img workspaces: checked against the shape, carved (the geom view's flag words are the img workspace's).
static int carve_state(const MgsRasterArgs* a, const Pass& s, GeomView& g, ImgView& im) {
  const size_t gb = geom_bytes(s, a->M), ib = img_bytes(s, a->W);
  if (!a->geom || a->geom_bytes < gb || !a->img || a->img_bytes < ib) {
    set_error("geom/img workspace too small: %zu < %zu or %zu < %zu", a->geom_bytes, gb, a->img_bytes, ib);
    return MGS_ERR_WORKSPACE;
  }
  g = carve_geom(a->geom, s.P, a->M, s.T, s.V, nullptr);
  im = carve_img(a->img, a->W, s.H, nullptr);
  g.flags = im.flags;
  return MGS_OK;
}

// The camera fields of FwdPreArgs / BwdPreArgs: a single view's come from MgsRasterArgs, a batch's from cam[] (one per view).
extern "C++" template <typename Args>  // (templates need C++ linkage)
static void fill_camera(Args& p, const MgsRasterArgs* a, const Pass& s) {
  p.use_cam = s.batch ? 1 : 0;
  if (!s.batch) {
    p.tanfovx = a->tanfovx; p.tanfovy = a->tanfovy;
    p.focal_y = a->H / (2.0f * a->tanfovy);  // rasterizer_impl.cu:225-226
    p.focal_x = a->W / (2.0f * a->tanfovx);
    p.viewmatrix = a->viewmatrix; p.projmatrix = a->projmatrix; p.campos = a->campos;
    return;
  }
  p.tanfovx = p.tanfovy = p.focal_x = p.focal_y = 0.f;
  p.viewmatrix = p.projmatrix = p.campos = nullptr;
  for (int v = 0; v < s.V; v++) {
    const MgsView& w = s.views[v];
    ViewCam& c = p.cam[v];
    c.tanfovx = w.tanfovx; c.tanfovy = w.tanfovy;
    c.focal_y = a->H / (2.0f * w.tanfovy);
    c.focal_x = a->W / (2.0f * w.tanfovx);
    c.viewmatrix = w.viewmatrix; c.projmatrix = w.projmatrix; c.campos = w.campos;
    c.row = set_row(s, v);
  }
}

// Everything of the forward before the instance count is known: (zero tables,) preprocess.  Leaves the carved workspaces in
// g, im (im.nonce: the launch's hand-shake nonce, im.direct_keys: where it wrote the tile keys).
// direct_keys: see direct_region (nullptr from the two-call path: its second call may come with another workspace).
static int enqueue_preprocess(const MgsRasterArgs* a, const Pass& s, const Options& o, int32_t* radii, uint64_t* direct_keys,
                              hipStream_t stream, GeomView& g, ImgView& im) {
  if (!radii || !a->opacities) { set_error("radii/opacities must be non-NULL"); return MGS_ERR_INVALID_ARG; }
  int rc = carve_state(a, s, g, im);
  if (rc) return rc;
  if (a->bwd_accum && ((reinterpret_cast<uintptr_t>(a->bwd_accum) & 15u) || (a->bwd_accum_bytes & 15u))) {
    set_error("bwd_accum must be 16-byte aligned and a multiple of 16 bytes");
    return MGS_ERR_INVALID_ARG;
  }
  FwdPreArgs p;
  p.V = s.V; p.Pg = s.Pg; p.Hp = s.batch ? s.Hp : 0;  // (0: a single view, its rows are H)
  p.P = s.P; p.D = a->D; p.M = a->M; p.W = a->W; p.H = a->H;
  p.tiles_x = s.tiles_x; p.tiles_y = s.tiles_yv;
  fill_camera(p, a, s);
  p.scale_modifier = a->scale_modifier;
  p.prefiltered = a->prefiltered; p.tight_bins = o.tight_bins;
  p.means3D = a->means3D; p.shs = a->shs; p.colors_precomp = a->colors_precomp; p.opacities = a->opacities;
  p.scales = a->scales; p.rotations = a->rotations; p.cov3D_precomp = a->cov3D_precomp;
  const bool lds = lds_tables(o, s.T);
  // LDS tables, table_init 0: workgroup 0 of the preprocess launch zeroes the tables and the others wait for its nonce (one
  // launch fewer; relies on workgroup 0 being dispatched first, bounded wait).  Otherwise a zero-fill launch of its own, ahead
  // of the preprocess in stream order: nonce 0, no workgroup waits for another.
  const bool handshake = lds && !o.table_init;
  if (!handshake) MGS_HIP(launch_zero_bytes(im.flags, im.zero_bytes, stream), "zero flags + tile tables");
  p.tables = im.flags; p.tables_words = (uint32_t)(im.zero_bytes / 4); p.ready = im.ready;
  p.nonce = handshake ? next_nonce() : 0ull;
  p.wg0_delay = (o.dbg & 1024) ? -1 : (o.dbg & 512) ? 100 : 0;
  im.nonce = p.nonce;
  p.zero_ptr = reinterpret_cast<float4*>(a->bwd_accum);
  p.zero_f4 = a->bwd_accum ? a->bwd_accum_bytes / 16 : 0;
  p.tile_hist = im.tile_hist;
  p.blk_base = lds ? g.blk_base : nullptr;
  p.ref_count = im.ref_count;
  im.direct_keys = lds ? direct_keys : nullptr; im.direct_stride = (uint32_t)s.Pg;
  p.direct_keys = im.direct_keys; p.direct_stride = im.direct_stride;
  { StageTimer t(ST_PREPROCESS, stream);
    MGS_STAGE(launch_preprocess_fwd(p, g, radii, stream), "preprocess", a->debug, stream); }
  return MGS_OK;
}

static const char* const kHandshakeMsg =
    "the forward preprocess gave up waiting for its zeroed tile tables (a workgroup of the launch did not make progress for "
    "about a second): nothing was binned for this call";
// Blocking read-back of {instance count, flags} (the reference's cudaMemcpy, rasterizer_impl.cu:284).  A hand-shake that
// gave up is reported as flag 2, as the status words report it.  *R_ref: the reference's count (instances of the 3-sigma rects).
static int read_count_blocking(const GeomView& g, const ImgView& im, hipStream_t stream, uint32_t* R, uint32_t* fl,
                               uint32_t* R_ref) {
  uint32_t host[2] = {0, 0};
  uint32_t ref = 0;
  MGS_HIP(hipMemcpyAsync(&ref, im.ref_count, sizeof(ref), hipMemcpyDeviceToHost, stream), "reference-count read-back");
  unsigned long long mark = 0ull;
  if (im.nonce)
    MGS_HIP(hipMemcpyAsync(&mark, im.ready + 1, sizeof(mark), hipMemcpyDeviceToHost, stream), "hand-shake read-back");
  MGS_HIP(hipMemcpyAsync(&host[0], g.flags + FLAG_NUM_RENDERED, sizeof(uint32_t), hipMemcpyDeviceToHost, stream),
          "num_rendered read-back");
  MGS_HIP(hipMemcpyAsync(&host[1], g.flags + FLAG_PREFILTERED, sizeof(uint32_t), hipMemcpyDeviceToHost, stream),
          "flag read-back");
  MGS_HIP(hipStreamSynchronize(stream), "stream sync");
  *R = host[0]; *fl = host[1];
  if (im.nonce && mark == im.nonce) *fl |= 2u;
  *R_ref = ref;
  return MGS_OK;
}

// The device counts instances in 32 unsigned bits; the C ABI (like the reference, rasterizer_impl.cu:282 `int num_rendered`)
// hands them out as int32: saturate instead of wrapping negative (advisor r4; 2^31 instances would need > 80 GB of lists).
static inline int32_t sat_i32(uint32_t v) { return v > 0x7fffffffu ? 0x7fffffff : (int32_t)v; }

// status word layout: tag (16) | flags (16) | count (32)
static inline bool status_arrived(uint64_t w, uint32_t tag) { return w != kStatusPending && (uint32_t)(w >> 48) == (tag & 0xffffu); }
static void status_pending(uint64_t* host_status) {
  volatile uint64_t* hs = host_status;
  hs[0] = kStatusPending; hs[1] = kStatusPending; hs[2] = kStatusPending;
}

// Wait for word 0 = {tag, flags, R} on the pinned status block (written by the binning kernel right after the preprocess).
// *R_ref: the reference's 3-sigma-rect count from word 2, which the device stores BEFORE word 0 (release order).
static int wait_status(uint64_t* host_status, uint32_t tag, hipStream_t stream, uint32_t* R, uint32_t* fl, uint32_t* R_ref) {
  volatile uint64_t* hs = host_status;
  uint64_t st = *hs;
  for (uint64_t spins = 0; !status_arrived(st, tag); spins++) {
    if ((spins & 0x3ff) == 0x3ff) {  // every ~1k polls: has the stream died or finished without reporting?
      hipError_t q = hipStreamQuery(stream);
      if (q != hipErrorNotReady) {
        st = *hs;
        if (status_arrived(st, tag)) break;
        set_error("forward finished without reporting the instance count: %s", hipGetErrorString(q));
        return MGS_ERR_HIP;
      }
    }
    __builtin_ia32_pause();
    st = *hs;
  }
  *R = (uint32_t)st; *fl = (uint32_t)(st >> 32) & 0xffffu;
  uint64_t w2 = hs[2];
  for (int spins = 0; !status_arrived(w2, tag) && spins < (1 << 20); spins++) { __builtin_ia32_pause(); w2 = hs[2]; }
  if (!status_arrived(w2, tag)) { set_error("forward reported its instance count without the reference count"); return MGS_ERR_HIP; }
  *R_ref = (uint32_t)w2;
  return MGS_OK;
}

static int check_prefiltered(uint32_t fl) {
  if (fl & 2u) { set_error("%s", kHandshakeMsg); return MGS_ERR_HIP; }  // (status-word flag of the bin scatter kernel)
  if (fl & 1u) {
    set_error("Point is filtered although prefiltered is set. This shouldn't happen!");  // auxiliary.h:158
    return MGS_ERR_INVALID_ARG;
  }
  return MGS_OK;
}

static RenderArgs render_args(const MgsRasterArgs* a, const Pass& s, const Options& o, const GeomView& g) {
  RenderArgs r;
  r.W = a->W; r.H = s.H; r.tiles_x = s.tiles_x; r.tiles_y = s.tiles_yv * s.V;
  r.F = s.F; r.include_feature = s.F > 0;
  r.fast_exp = o.fast_exp; r.exact_cull = o.exact_cull; r.gm_waves = o.gm_waves; r.dbg = o.dbg & ~(512 | 1024);
  r.nwf = fwd_waves(s.F, s.T);
  r.V = s.V; r.Pg = s.Pg; r.Hv = s.Hv; r.Hp = s.Hp;
  r.colors_per_view = s.batch && !a->colors_precomp;
  for (int v = 0; v < MAX_VIEWS; v++) r.row[v] = v < s.V ? set_row(s, v) : 0;
  r.bg = a->background;
  r.colors = a->colors_precomp ? a->colors_precomp : g.rgb;
  r.feats = a->language_feature;
  r.rec = g.rec;
  return r;
}

// Binning + render on the workspaces the preprocess left in g, im.  status: where the device reports (host == nullptr:
// nowhere); im.nonce: the preprocess's hand-shake for the bin scatter to check (0: the host has already looked at it).
static int enqueue_render(const MgsRasterArgs* a, const Pass& s, const Options& o, const BinShape& bs, const GeomView& g,
                          const ImgView& im, float* out_color, float* out_feature, StatusSink status, hipStream_t stream) {
  ChunkView cv;
  const BinView b = carve_binning(a->binning, bs.cap, s.T, s.F, bs.pool, &cv, nullptr);
  const bool lds = lds_tables(o, s.T), bucket = bucket_rank(o, s.T);
  for (int k = 0; k < 3; k++) {
    if (k == 2 && bucket) break;  // (the bucket rank of stage 1 wrote the sorted ids)
    if (k == 0 && bucket && im.direct_keys) continue;  // (direct binning: the preprocess wrote the keys, no scatter launch)
    StageTimer t(ST_BIN_SCATTER + k, stream);
    MGS_STAGE(launch_bin_segsort(k, lds, bucket, g, b, im, s.Pg, s.V, bs.cap, s.tiles_x, s.tiles_yv * s.V, o.seg, o.dbg, status,
                                 stream),
              "binning", a->debug, stream);
  }
  const RenderArgs r = render_args(a, s, o, g);
  { StageTimer t(ST_RENDER_FWD, stream);
    MGS_STAGE(launch_render_fwd_dense(r, b, im, cv, out_color, out_feature, status, stream), "render forward", a->debug,
              stream); }
  return MGS_OK;
}

// Output images of a forward: present; P == 0 (rasterize_points.cu:70-92): zero-filled, a completed status left behind,
// nothing else launched (*done).
static int check_outputs(const MgsRasterArgs* a, const Pass& s, float* out_color, float* out_feature, uint64_t* host_status,
                         hipStream_t stream, bool* done) {
  *done = false;
  if (!out_color) { set_error("out_color is NULL"); return MGS_ERR_INVALID_ARG; }
  if (s.F > 0 && !out_feature) { set_error("out_feature is NULL"); return MGS_ERR_INVALID_ARG; }
  if (a->P == 0) {
    const size_t N = (size_t)s.V * a->W * a->H;
    MGS_HIP(launch_zero_bytes(out_color, 3 * N * sizeof(float), stream), "memset out_color");
    if (s.F > 0) MGS_HIP(launch_zero_bytes(out_feature, s.F * N * sizeof(float), stream), "memset out_feature");
    if (host_status) {
      const uint64_t w = (uint64_t)(a->status_tag & 0xffffu) << 48;
      host_status[0] = w; host_status[1] = w; host_status[2] = w;
    }
    *done = true;
  }
  return MGS_OK;
}

// Every forward that enqueues the preprocess: the fused one (render), with the status words (host_status, debug 0) or with a
// blocking read-back, and stage 1 of the two-call path (!render, which only waits).  A form that waits for the preprocess and
// finds that its table hand-shake gave up runs again with the tables zeroed by a launch of their own (no workgroup waits for
// another on that path); an asynchronous one reports it through mgs_forward_result instead.
static int forward(const MgsRasterArgs* a, const Pass& s, bool render, int32_t* radii, float* out_color, float* out_feature,
                   int32_t* num_rendered, uint64_t* host_status, hipStream_t stream) {
  Options o = options_of(a);
  BinShape bs = {0, 0u};
  uint64_t* dk = nullptr;
  if (render) {
    bs = bin_shape(a, s.T, s.F);
    const int rc = check_binning(a, bs, -1);
    if (rc) return rc;
    dk = direct_region(a, bs, s, o);
  }
  const bool words = render && host_status && !a->debug;  // else no device->host status channel: read back like stage 1
  const StatusSink status = {host_status, a->status_tag};
  for (;;) {
    GeomView g; ImgView im;
    int rc = enqueue_preprocess(a, s, o, radii, dk, stream, g, im);
    if (rc) return rc;
    uint32_t R = 0, fl = 0, R_ref = 0;
    if (words) {
      // sync-free: everything is enqueued; the binning kernel stores {tag, reference count} and {tag, flags, R} to the mapped
      // host words as soon as the preprocess is done, and refuses to bin (empty ranges, zero segments) when R exceeds the
      // capacity.
      status_pending(host_status);
      rc = enqueue_render(a, s, o, bs, g, im, out_color, out_feature, status, stream);
      if (rc) return rc;
      if (a->async_forward) { *num_rendered = -1; return MGS_OK; }  // the caller reads mgs_forward_result later
      // Wait for the PREPROCESS only: word 0 arrives when the binning starts; binning and render run on while this call
      // returns.  The reference's integer comes through word 2 of the same block.
      rc = wait_status(host_status, a->status_tag, stream, &R, &fl, &R_ref);
    } else {
      if (render && a->async_forward) { set_error("async_forward needs host_status and debug == 0"); return MGS_ERR_INVALID_ARG; }
      rc = read_count_blocking(g, im, stream, &R, &fl, &R_ref);
    }
    if (rc) return rc;
    if ((fl & 2u) && !o.table_init) {
      // A preprocess workgroup gave up waiting for the zeroed tables (workgroup 0 of the launch made no progress for about a
      // second): nothing was binned.  (The first run's kernels still report through the same words: drain them first.)
      MGS_HIP(hipStreamSynchronize(stream), "stream sync before the hand-shake retry");
      o.table_init = 1; o.dbg &= ~(512 | 1024);
      continue;
    }
    rc = check_prefiltered(fl);
    if (rc) return rc;
    *num_rendered = sat_i32(R_ref);  // the reference's integer; the workspace has to hold the R instances actually binned
    if (!render) return MGS_OK;
    if ((int)R > bs.cap) return MGS_NEED_CAPACITY;
    if (words) return MGS_OK;
    if (host_status) status_pending(host_status);  // (debug: the words are reported by the kernels as usual)
    im.nonce = 0ull;  // (looked at above)
    return enqueue_render(a, s, o, bs, g, im, out_color, out_feature, status, stream);
  }
}

// Backward (render backward, preprocess backward) of a forward that ran on the same workspaces.
static int backward(const MgsRasterArgs* a, const Pass& s, int32_t R, const int32_t* radii, const float* dL_dout_color,
                    const float* dL_dout_feature, float* dL_dmeans2D, float* dL_dconic, float* dL_dopacity, float* dL_dcolors,
                    float* dL_dfeature, float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscales,
                    float* dL_drotations, void* scratch, size_t scratch_bytes, hipStream_t stream) {
  const int F = s.F;
  if (!radii || !dL_dout_color || !dL_dmeans2D || !dL_dopacity || !dL_dcolors || !dL_dmeans3D || !dL_dcov3D ||
      !dL_dscales || !dL_drotations || (a->M > 0 && !dL_dsh) || (F > 0 && (!dL_dfeature || !dL_dout_feature))) {
    set_error("backward: a required pointer is NULL");
    return MGS_ERR_INVALID_ARG;
  }
  const size_t scratch_total = mgs_backward_scratch_bytes(s.P, a->M, F);
  if (!scratch || scratch_bytes < scratch_total) { set_error("backward: scratch too small"); return MGS_ERR_WORKSPACE; }
  GeomView g; ImgView im;
  int rc = carve_state(a, s, g, im);
  if (rc) return rc;
  const BinShape bs = bin_shape(a, s.T, F);
  // (R is the integer the forward handed back -- the reference's 3-sigma-rect count, at least the instances binned -- or -1:
  //  only R == 0 is acted on here; that the workspace holds the binned lists was the forward's check)
  rc = check_binning(a, bs, -1);
  if (rc) return rc;
  if (F > 0 && (reinterpret_cast<uintptr_t>(a->language_feature) & 15u)) {  // the render backward reads feature rows as float4
    set_error("backward: language_feature must be 16-byte aligned");
    return MGS_ERR_INVALID_ARG;
  }
  const Options o = options_of(a);
  ChunkView cv;
  const BinView b = carve_binning(a->binning, bs.cap, s.T, F, bs.pool, &cv, nullptr);
  const BwdScratch sc = carve_bwd(scratch, s.P, a->M, F, nullptr);
  // accumulators the render backward adds into.  dL_dcolors is the gradient w.r.t. the per-Gaussian RGB whether it came from
  // colors_precomp or from SH (the reference returns it in both cases, rasterize_points.cu:169,224); a batch's has a row per
  // (view, Gaussian) with SH colours (they differ per view); with colors_precomp, and for dL_dfeature, one per (set, Gaussian)
  const size_t P = (size_t)a->P * s.S, PV = (size_t)s.P, ncol = s.batch && !a->colors_precomp ? PV : P;
  // With SH colours the render backward sums the colour gradient in acc16's slots 6-8 (one row per (view, Gaussian), like
  // dL_dcolors then) and the preprocess backward copies it out; with colors_precomp it adds into dL_dcolors directly.
  float* dcol = dL_dcolors;
  const bool merged = a->colors_precomp == nullptr;
  if (!a->accum_prezeroed)
  { StageTimer t(ST_BWD_MEMSET, stream);
    // one fill when the caller laid acc16 | dL_dcolors | dL_dfeature out back to back (manigaussian_amd/_C.py, views.py do)
    char* z0 = reinterpret_cast<char*>(sc.acc16);
    char* z_end = z0 + 16 * PV * sizeof(float);
    const bool adj_col = reinterpret_cast<char*>(dcol) >= z_end && reinterpret_cast<char*>(dcol) <= z0 + scratch_total + 64;
    const bool adj_feat = F == 0 || reinterpret_cast<char*>(dL_dfeature) == reinterpret_cast<char*>(dcol) + 3 * ncol * sizeof(float);
    if (adj_col && adj_feat) {
      char* end = reinterpret_cast<char*>(dcol) + (3 * ncol + (size_t)F * P) * sizeof(float);
      MGS_HIP(launch_zero_bytes(z0, (size_t)(end - z0), stream), "memset accumulators");
    } else {
      MGS_HIP(launch_zero_bytes(sc.acc16, 16 * PV * sizeof(float), stream), "memset acc16");
      if (!merged) MGS_HIP(launch_zero_bytes(dcol, 3 * ncol * sizeof(float), stream), "memset dL_dcolors");
      if (F > 0) MGS_HIP(launch_zero_bytes(dL_dfeature, (size_t)F * P * sizeof(float), stream), "memset dL_dfeature");
    } }
  if (R != 0) {  // R < 0: count unknown to the host (asynchronous forward) -- empty ranges make the kernel a no-op
    const RenderArgs r = render_args(a, s, o, g);
    StageTimer t(ST_RENDER_BWD, stream);
    MGS_STAGE(launch_render_bwd_gm(r, b, im, cv, dL_dout_color, dL_dout_feature, sc.acc16, merged ? nullptr : dcol, dL_dfeature, stream),
              "render backward", a->debug, stream);
  }
  BwdPreArgs p;
  p.V = s.V; p.S = s.S; p.cov3D_per_view = s.batch && !a->cov3D_precomp;
  p.P = a->P; p.D = a->D; p.M = a->M; p.W = a->W; p.H = a->H;
  fill_camera(p, a, s);
  p.scale_modifier = a->scale_modifier;
  p.means3D = a->means3D; p.shs = a->shs; p.scales = a->scales; p.rotations = a->rotations;
  p.cov3D = a->cov3D_precomp ? a->cov3D_precomp : g.cov3D;
  p.radii = radii; p.clamped = g.clamped; p.acc16 = sc.acc16; p.dL_dcolor = dcol;
  p.dL_dmeans2D = dL_dmeans2D; p.dL_dconic = dL_dconic; p.dL_dopacity = dL_dopacity; p.dL_dmeans3D = dL_dmeans3D;
  p.dL_dcov3D = dL_dcov3D; p.dL_dsh = dL_dsh; p.dL_dscales = dL_dscales; p.dL_drot = dL_drotations;
  { StageTimer t(ST_PREPROCESS_BWD, stream);
    MGS_STAGE(launch_preprocess_bwd(p, stream), "preprocess backward", a->debug, stream); }
  return MGS_OK;
}

static int check_views(const MgsRasterArgs* a, int V, const MgsView* views) {
  if (!a || !views || V < 1 || V > MAX_VIEWS) { set_error("views: need 1 <= V <= %d", MAX_VIEWS); return MGS_ERR_INVALID_ARG; }
  MgsRasterArgs a1 = *a;  // (the shared checks, on view 0's camera)
  a1.viewmatrix = views[0].viewmatrix; a1.projmatrix = views[0].projmatrix; a1.campos = views[0].campos;
  a1.tanfovx = views[0].tanfovx; a1.tanfovy = views[0].tanfovy;
  int rc = check_common(&a1);
  if (rc) return rc;
  for (int v = 0; v < V; v++)
    if (!views[v].viewmatrix || !views[v].projmatrix || !views[v].campos) { set_error("view %d: NULL matrix", v); return MGS_ERR_INVALID_ARG; }
  if (a->debug) { set_error("multi-view batches need debug 0"); return MGS_ERR_INVALID_ARG; }
  return MGS_OK;
}
// A set batch: the view checks, 1 <= S <= MAX_VIEWS, every view's set in [0, S), and rows that fit the kernels' 32-bit indices.
static int check_sets(const MgsRasterArgs* a, int V, const MgsView* views, int S, const int32_t* view_set) {
  int rc = check_views(a, V, views);
  if (rc) return rc;
  if (S < 1 || S > MAX_VIEWS) { set_error("sets: need 1 <= S <= %d, got S = %d", MAX_VIEWS, S); return MGS_ERR_INVALID_ARG; }
  if (!view_set) { set_error("sets: view_set is NULL"); return MGS_ERR_INVALID_ARG; }
  for (int v = 0; v < V; v++)
    if (view_set[v] < 0 || view_set[v] >= S) {
      set_error("sets: view %d renders set %d, outside [0, %d)", v, view_set[v], S);
      return MGS_ERR_INVALID_ARG;
    }
  const unsigned long long rows = (unsigned long long)a->P * (unsigned long long)S;
  if (rows > 0x7fffffffull) { set_error("sets: S * P = %llu rows exceed 2^31 - 1", rows); return MGS_ERR_INVALID_ARG; }
  if (a->include_feature && rows * (unsigned long long)a->F * 4ull >= (1ull << 32)) {
    set_error("sets: S * P * F * 4 = %llu bytes of features: rows are addressed by 32-bit offsets (< 4 GiB)",
              rows * (unsigned long long)a->F * 4ull);
    return MGS_ERR_INVALID_ARG;
  }
  return MGS_OK;
}

int mgs_rasterize_forward_preprocess(const MgsRasterArgs* a, int32_t* radii, int32_t* num_rendered,
                                     mgs_stream_t stream_) {
  int rc = check_common(a);
  if (rc) return rc;
  if (!num_rendered) { set_error("num_rendered is NULL"); return MGS_ERR_INVALID_ARG; }
  *num_rendered = 0;
  if (a->P == 0) return MGS_OK;  // rasterize_points.cu:92
  // (*num_rendered: the reference's integer, >= the instances actually binned: a safe size for stage 2)
  return forward(a, pass_of(a), false, radii, nullptr, nullptr, num_rendered, nullptr, (hipStream_t)stream_);
}

int mgs_rasterize_forward_render(const MgsRasterArgs* a, int32_t R, const int32_t* radii, float* out_color,
                                 float* out_feature, mgs_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  int rc = check_common(a);
  if (rc) return rc;
  const Pass s = pass_of(a);
  bool done;
  rc = check_outputs(a, s, out_color, out_feature, nullptr, stream, &done);
  if (rc || done) return rc;
  if (R < 0 || !radii) { set_error("num_rendered < 0 or radii NULL"); return MGS_ERR_INVALID_ARG; }
  GeomView g; ImgView im;
  rc = carve_state(a, s, g, im);
  if (rc) return rc;
  im.direct_stride = (uint32_t)s.Pg;  // (no direct keys: stage 1 may have run on another binning workspace)
  // the render forward's counters (chunk records taken, blocks done) may be left over from an earlier render on this img
  // workspace (the capacity-retry path): reset them; the preprocess's words (flags 0-1, histogram) stay
  MGS_HIP(launch_zero_bytes(im.flags + FLAG_CHUNKS_USED, 2 * sizeof(uint32_t), stream), "reset render counters");
  const BinShape bs = bin_shape(a, s.T, s.F);
  rc = check_binning(a, bs, R);
  if (rc) return rc;
  return enqueue_render(a, s, options_of(a), bs, g, im, out_color, out_feature, StatusSink{nullptr, 0}, stream);
}

int mgs_rasterize_forward(const MgsRasterArgs* a, int32_t* radii, float* out_color, float* out_feature,
                          int32_t* num_rendered, uint64_t* host_status, mgs_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  int rc = check_common(a);
  if (rc) return rc;
  if (!num_rendered) { set_error("num_rendered is NULL"); return MGS_ERR_INVALID_ARG; }
  *num_rendered = 0;
  const Pass s = pass_of(a);
  bool done;
  rc = check_outputs(a, s, out_color, out_feature, host_status, stream, &done);
  if (rc || done) return rc;
  return forward(a, s, true, radii, out_color, out_feature, num_rendered, host_status, stream);
}

// The forward of a view batch (view_set == nullptr: one set) or of a set batch; the arguments are checked.
static int forward_batch(const MgsRasterArgs* a, int V, const MgsView* views, int S, const int32_t* view_set, int32_t* radii,
                         float* out_color, float* out_feature, int32_t* num_rendered, uint64_t* host_status,
                         hipStream_t stream) {
  if (!num_rendered || !host_status) { set_error("num_rendered / host_status is NULL"); return MGS_ERR_INVALID_ARG; }
  *num_rendered = 0;
  const Pass s = pass_of(a, V, views, S, view_set);
  bool done;
  const int rc = check_outputs(a, s, out_color, out_feature, host_status, stream, &done);
  if (rc || done) return rc;
  return forward(a, s, true, radii, out_color, out_feature, num_rendered, host_status, stream);
}

int mgs_rasterize_forward_views(const MgsRasterArgs* a, int32_t V, const MgsView* views, int32_t* radii, float* out_color,
                                float* out_feature, int32_t* num_rendered, uint64_t* host_status, mgs_stream_t stream_) {
  const int rc = check_views(a, V, views);
  if (rc) return rc;
  return forward_batch(a, V, views, 1, nullptr, radii, out_color, out_feature, num_rendered, host_status,
                       (hipStream_t)stream_);
}

int mgs_rasterize_forward_sets(const MgsRasterArgs* a, int32_t V, const MgsView* views, int32_t S, const int32_t* view_set,
                               int32_t* radii, float* out_color, float* out_feature, int32_t* num_rendered,
                               uint64_t* host_status, mgs_stream_t stream_) {
  const int rc = check_sets(a, V, views, S, view_set);
  if (rc) return rc;
  return forward_batch(a, V, views, S, view_set, radii, out_color, out_feature, num_rendered, host_status,
                       (hipStream_t)stream_);
}

static int forward_result(const MgsRasterArgs* a, const Pass& s, const uint64_t* host_status, int32_t* num_rendered,
                          int32_t* chunks_used, int32_t* ref_rendered) {
  if (num_rendered) *num_rendered = -1;
  if (chunks_used) *chunks_used = -1;
  if (ref_rendered) *ref_rendered = -1;
  if (!host_status) { set_error("forward_result: NULL argument"); return MGS_ERR_INVALID_ARG; }
  const volatile uint64_t* hs = host_status;
  const uint64_t w0 = hs[0], w1 = hs[1];
  const bool a0 = status_arrived(w0, a->status_tag), a1 = status_arrived(w1, a->status_tag);
  if (a0 && num_rendered) *num_rendered = sat_i32((uint32_t)w0);
  if (a0 && ref_rendered) {  // (stored before word 0: arrived if word 0 has)
    const uint64_t w2 = hs[2];
    if (status_arrived(w2, a->status_tag)) *ref_rendered = sat_i32((uint32_t)w2);
  }
  if (a1 && chunks_used) *chunks_used = (int32_t)(uint32_t)w1;
  if (a0) {
    const uint32_t fl = (uint32_t)(w0 >> 32) & 0xffffu;
    if (fl & 2u) { set_error("%s", kHandshakeMsg); return MGS_RETRY_TABLE_INIT; }  // (nothing was binned; word 1 reports 0 chunks)
    const int rc = check_prefiltered(fl);
    if (rc) return rc;
    if (a->P > 0) {
      const BinShape bs = bin_shape(a, s.T, s.F);
      if ((int64_t)(uint32_t)w0 > (int64_t)bs.cap) return MGS_NEED_CAPACITY;  // nothing was binned: word 1 reports 0 chunks
    }
  }
  if (!a0 || !a1) return MGS_PENDING;
  if ((uint32_t)(w1 >> 32) & 1u) return MGS_NEED_CAPACITY;  // the chunk pool overflowed
  return MGS_OK;
}
int mgs_forward_result(const MgsRasterArgs* a, const uint64_t* host_status, int32_t* num_rendered, int32_t* chunks_used,
                       int32_t* ref_rendered) {
  if (!a) { set_error("forward_result: NULL argument"); return MGS_ERR_INVALID_ARG; }
  return forward_result(a, pass_of(a), host_status, num_rendered, chunks_used, ref_rendered);
}
int mgs_forward_result_views(const MgsRasterArgs* a, int32_t V, const uint64_t* host_status, int32_t* num_rendered,
                             int32_t* chunks_used, int32_t* ref_rendered) {
  if (!a || V < 1) { set_error("forward_result_views: bad argument"); return MGS_ERR_INVALID_ARG; }
  return forward_result(a, pass_of(a, V), host_status, num_rendered, chunks_used, ref_rendered);
}

int mgs_rasterize_backward(const MgsRasterArgs* a, int32_t R, const int32_t* radii, const float* dL_dout_color,
                           const float* dL_dout_feature, float* dL_dmeans2D, float* dL_dconic, float* dL_dopacity,
                           float* dL_dcolors, float* dL_dfeature, float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh,
                           float* dL_dscales, float* dL_drotations, void* scratch, size_t scratch_bytes,
                           mgs_stream_t stream_) {
  int rc = check_common(a);
  if (rc) return rc;
  if (a->P == 0) return MGS_OK;  // rasterize_points.cu:186: empty gradient tensors
  return backward(a, pass_of(a), R, radii, dL_dout_color, dL_dout_feature, dL_dmeans2D, dL_dconic, dL_dopacity, dL_dcolors,
                  dL_dfeature, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations, scratch, scratch_bytes,
                  (hipStream_t)stream_);
}

int mgs_rasterize_backward_views(const MgsRasterArgs* a, int32_t V, const MgsView* views, int32_t R, const int32_t* radii,
                                 const float* dL_dout_color, const float* dL_dout_feature, float* dL_dmeans2D,
                                 float* dL_dconic, float* dL_dopacity, float* dL_dcolors, float* dL_dfeature,
                                 float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscales, float* dL_drotations,
                                 void* scratch, size_t scratch_bytes, mgs_stream_t stream_) {
  int rc = check_views(a, V, views);
  if (rc) return rc;
  if (a->P == 0) return MGS_OK;
  return backward(a, pass_of(a, V, views), R, radii, dL_dout_color, dL_dout_feature, dL_dmeans2D, dL_dconic, dL_dopacity,
                  dL_dcolors, dL_dfeature, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations, scratch, scratch_bytes,
                  (hipStream_t)stream_);
}

int mgs_rasterize_backward_sets(const MgsRasterArgs* a, int32_t V, const MgsView* views, int32_t S, const int32_t* view_set,
                                int32_t R, const int32_t* radii, const float* dL_dout_color, const float* dL_dout_feature,
                                float* dL_dmeans2D, float* dL_dconic, float* dL_dopacity, float* dL_dcolors, float* dL_dfeature,
                                float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscales, float* dL_drotations,
                                void* scratch, size_t scratch_bytes, mgs_stream_t stream_) {
  int rc = check_sets(a, V, views, S, view_set);
  if (rc) return rc;
  if (a->P == 0) return MGS_OK;
  return backward(a, pass_of(a, V, views, S, view_set), R, radii, dL_dout_color, dL_dout_feature, dL_dmeans2D, dL_dconic,
                  dL_dopacity, dL_dcolors, dL_dfeature, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations, scratch,
                  scratch_bytes, (hipStream_t)stream_);
}

int mgs_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix, uint8_t* present,
                     mgs_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (P < 0) { set_error("P < 0"); return MGS_ERR_INVALID_ARG; }
  if (P == 0) return MGS_OK;
  if (!means3D || !viewmatrix || !projmatrix || !present) { set_error("mark_visible: NULL pointer"); return MGS_ERR_INVALID_ARG; }
  MGS_HIP(launch_mark_visible(P, means3D, viewmatrix, projmatrix, present, stream), "mark_visible");
  return MGS_OK;
}

// Diagnostic (blocking): what the forward that last ran on these workspaces left behind, in the units its state is kept in:
//   incidences    (8x8 block, Gaussian) pairs of the chunks some pixel of the block visited (the fill may have listed more)
//   chunks        64-survivor chunks some pixel of their block visited
//   pixel_chunks  (pixel, chunk) pairs visited: what the per-chunk state (partial sums, T_end, T_mid, last_pos) costs
int mgs_forward_stats(const MgsRasterArgs* a, int32_t V, int64_t* incidences, int64_t* chunks, int64_t* pixel_chunks,
                      mgs_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!a || !a->binning || V < 0 || V > MAX_VIEWS) { set_error("forward_stats: bad argument"); return MGS_ERR_INVALID_ARG; }
  const Pass s = pass_of(a, V);
  const BinShape bs = bin_shape(a, s.T, s.F);
  if (bs.cap < 0) { set_error("forward_stats: binning workspace smaller than its fixed part"); return MGS_ERR_WORKSPACE; }
  ChunkView cv;
  (void)carve_binning(a->binning, bs.cap, s.T, s.F, bs.pool, &cv, nullptr);
  std::vector<uint2> ns((size_t)s.T * 4);
  std::vector<uint32_t> lc((size_t)s.T * 4 * 64);
  MGS_HIP(hipMemcpyAsync(ns.data(), cv.nsurv, ns.size() * sizeof(uint2), hipMemcpyDeviceToHost, stream), "forward_stats copy");
  MGS_HIP(hipMemcpyAsync(lc.data(), cv.last_chunk, lc.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, stream), "forward_stats copy");
  MGS_HIP(hipStreamSynchronize(stream), "forward_stats sync");
  int64_t inc = 0, ch = 0, pc = 0;
  for (size_t b = 0; b < ns.size(); b++) {
    uint32_t vmax = 0;
    for (int p = 0; p < 64; p++) { const uint32_t v = lc[b * 64 + p]; pc += v; if (v > vmax) vmax = v; }
    ch += vmax;
    const int64_t listed = ns[b].x, visited = (int64_t)vmax * CHUNK;
    inc += listed < visited ? listed : visited;
  }
  if (incidences) *incidences = inc;
  if (chunks) *chunks = ch;
  if (pixel_chunks) *pixel_chunks = pc;
  return MGS_OK;
}

// Diagnostic: byte offsets of the per-Gaussian arrays the forward preprocess leaves in a geom workspace of mgs_geom_bytes(P,
// M, W, H) bytes (tests compare them bit for bit with the reference's GeometryState).
int mgs_debug_geom_layout(int P, int M, int W, int H, size_t* depths, size_t* rec, size_t* rgb, size_t* cov3D) {
  if (P < 0 || W <= 0 || H <= 0) { set_error("geom_layout: bad shape"); return MGS_ERR_INVALID_ARG; }
  char* const base = reinterpret_cast<char*>(ALIGN);  // (a non-null dummy base: carve_geom yields null pointers for nullptr)
  const GeomView g = carve_geom(base, P, M, num_tiles(W, H), 1, nullptr);
  if (depths) *depths = (size_t)(reinterpret_cast<char*>(g.depths) - base);
  if (rec) *rec = (size_t)(reinterpret_cast<char*>(g.rec) - base);
  if (rgb) *rgb = (size_t)(reinterpret_cast<char*>(g.rgb) - base);
  if (cov3D) *cov3D = (size_t)(reinterpret_cast<char*>(g.cov3D) - base);
  return MGS_OK;
}

int mgs_debug_binning_layout(const MgsRasterArgs* a, int32_t V, size_t* keys_unsorted, size_t* point_list, size_t* img_ranges,
                             int32_t* capacity) {
  if (!a || a->W <= 0 || a->H <= 0) { set_error("binning_layout: bad argument"); return MGS_ERR_INVALID_ARG; }
  const Pass s = pass_of(a, V);
  const BinShape bs = bin_shape(a, s.T, s.F);
  if (bs.cap < 0) { set_error("binning_layout: binning workspace smaller than its fixed part"); return MGS_ERR_WORKSPACE; }
  char* const base = reinterpret_cast<char*>(ALIGN);
  const BinView b = carve_binning(base, bs.cap, s.T, s.F, bs.pool, nullptr, nullptr);
  const ImgView im = carve_img(base, a->W, s.H, nullptr);
  if (keys_unsorted) *keys_unsorted = (size_t)(reinterpret_cast<char*>(b.keys_unsorted) - base);
  if (point_list) *point_list = (size_t)(reinterpret_cast<char*>(b.point_list) - base);
  if (img_ranges) *img_ranges = (size_t)(reinterpret_cast<char*>(im.ranges) - base);
  if (capacity) *capacity = bs.cap;
  return MGS_OK;
}

int mgs_debug_direct_keys(const MgsRasterArgs* a, int32_t V, size_t* keys, int32_t* stride) {
  if (!a || a->W <= 0 || a->H <= 0 || !keys || !stride) { set_error("direct_keys: bad argument"); return MGS_ERR_INVALID_ARG; }
  *keys = 0; *stride = 0;
  if (a->P <= 0 || !a->binning) return MGS_OK;
  const Pass s = pass_of(a, V);
  const BinShape bs = bin_shape(a, s.T, s.F);
  if (bs.cap < 0) { set_error("direct_keys: binning workspace smaller than its fixed part"); return MGS_ERR_WORKSPACE; }
  const uint64_t* dk = direct_region(a, bs, s, options_of(a));
  if (!dk) return MGS_OK;
  *keys = (size_t)(reinterpret_cast<const char*>(dk) - static_cast<const char*>(a->binning));
  *stride = a->P;
  return MGS_OK;
}

// Diagnostic (host code only): every region the three workspaces of `a` are carved into, read off the carve_* calls
// themselves (CarveLog), named and classified in carving order.  FLOAT: no kernel derives an address, a loop bound, an LDS
// index or a sort bucket from the region's words when it reads them legitimately (DESIGN.md 8b holds the table and the
// reasons); everything else, and everything in doubt, is INDEX.
struct RegionName { const char* name; int kind; };
static const RegionName kGeomRegions[] = {
    {"depths", MGS_REGION_INDEX}, {"rec", MGS_REGION_INDEX},     {"rect", MGS_REGION_INDEX},     {"rgb", MGS_REGION_FLOAT},
    {"cov3D", MGS_REGION_FLOAT},  {"clamped", MGS_REGION_INDEX}, {"blk_base", MGS_REGION_INDEX}};
static const RegionName kImgRegions[] = {{"final_T", MGS_REGION_FLOAT},
                                         {"ranges", MGS_REGION_INDEX},
                                         {"tables", MGS_REGION_INDEX},  // flags | tile_hist | seg_base | ref_count
                                         {"ready", MGS_REGION_INDEX},
                                         {"cursor", MGS_REGION_INDEX}};
static const RegionName kBinRegions[] = {
    {"keys_unsorted", MGS_REGION_INDEX}, {"keys", MGS_REGION_INDEX},       {"point_list", MGS_REGION_INDEX},
    {"seg_desc", MGS_REGION_INDEX},      {"round_base", MGS_REGION_INDEX}, {"last_chunk", MGS_REGION_INDEX},
    {"nsurv", MGS_REGION_INDEX},         {"surv", MGS_REGION_INDEX},       {"T_end", MGS_REGION_FLOAT},
    {"T_mid", MGS_REGION_FLOAT},         {"last_pos", MGS_REGION_INDEX},   {"q", MGS_REGION_FLOAT},
    {"partial", MGS_REGION_FLOAT}};

int mgs_debug_workspace_regions(const MgsRasterArgs* a, int32_t V, MgsWorkspaceRegion* out, int32_t max_regions,
                                int32_t* count) {
  if (!a || a->W <= 0 || a->H <= 0 || a->P <= 0 || V < 0 || V > MAX_VIEWS || !count || (max_regions > 0 && !out)) {
    set_error("workspace_regions: bad argument");
    return MGS_ERR_INVALID_ARG;
  }
  const Pass s = pass_of(a, V);
  const BinShape bs = bin_shape(a, s.T, s.F);
  if (bs.cap < 0) { set_error("workspace_regions: binning workspace smaller than its fixed part"); return MGS_ERR_WORKSPACE; }
  char* const base = reinterpret_cast<char*>(ALIGN);  // (a non-null dummy base: nothing is dereferenced)
  CarveLog lg, li, lb;
  (void)carve_geom(base, s.P, a->M, s.T, s.V, nullptr, &lg);
  (void)carve_img(base, a->W, s.H, nullptr, &li);
  size_t bin_total = 0;
  (void)carve_binning(base, bs.cap, s.T, s.F, bs.pool, nullptr, &bin_total, &lb);
  constexpr int NG = sizeof(kGeomRegions) / sizeof(RegionName), NI = sizeof(kImgRegions) / sizeof(RegionName),
                NB = sizeof(kBinRegions) / sizeof(RegionName);
  if (lg.n != NG || li.n != NI || lb.n != NB) {
    set_error("workspace_regions: the region names are out of step with the carving (%d/%d, %d/%d, %d/%d)", lg.n, NG, li.n, NI,
              lb.n, NB);
    return MGS_ERR_INVALID_ARG;
  }
  int n = 0;
  auto put = [&](int ws, const RegionName& r, size_t off, size_t bytes, int alias) {
    if (n < max_regions) {
      MgsWorkspaceRegion& o = out[n];
      memset(&o, 0, sizeof(o));
      strncpy(o.name, r.name, sizeof(o.name) - 1);
      o.workspace = ws; o.kind = r.kind; o.alias = alias; o.offset = off; o.bytes = bytes;
    }
    n++;
  };
  for (int i = 0; i < NG; i++) put(MGS_WORKSPACE_GEOM, kGeomRegions[i], lg.off[i], lg.bytes[i], 0);
  for (int i = 0; i < NI; i++) put(MGS_WORKSPACE_IMG, kImgRegions[i], li.off[i], li.bytes[i], 0);
  for (int i = 0; i < NB; i++) put(MGS_WORKSPACE_BINNING, kBinRegions[i], lb.off[i], lb.bytes[i], 0);
  // the direct keys (direct_region): inside the two key arrays (an alias of regions listed above) or behind the carved arrays
  MgsRasterArgs c = *a;
  c.binning = base;
  if (const uint64_t* dk = direct_region(&c, bs, s, options_of(a))) {
    const size_t off = (size_t)(reinterpret_cast<const char*>(dk) - base);
    const RegionName r = {"direct_keys", MGS_REGION_INDEX};
    put(MGS_WORKSPACE_BINNING, r, off, direct_keys_needed((size_t)s.P, s.V, s.T) * sizeof(uint64_t), off < bin_total ? 1 : 0);
  }
  *count = n;
  if (n > max_regions && max_regions > 0) { set_error("workspace_regions: %d regions, room for %d", n, max_regions); return MGS_ERR_INVALID_ARG; }
  return MGS_OK;
}

int mgs_profile_num_stages(void) { return ST_COUNT; }
const char* mgs_profile_stage_name(int i) { return (i >= 0 && i < ST_COUNT) ? kStageNames[i] : ""; }

int mgs_profile_read(double* total_ms, int32_t* counts, int reset) {
  Profiler& p = profiler();
  std::lock_guard<std::mutex> lk(p.mu);
  for (int st = 0; st < ST_COUNT; st++) {
    double sum = 0;
    int n = 0;
    for (auto& pr : p.used[st]) {
      float ms = 0.f;
      if (hipEventSynchronize(pr.second) == hipSuccess && hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) {
        sum += ms;
        n++;
      }
    }
    if (total_ms) total_ms[st] = sum;
    if (counts) counts[st] = n;
    if (reset) {
      for (auto& pr : p.used[st]) { p.pool.push_back(pr.first); p.pool.push_back(pr.second); }
      p.used[st].clear();
    }
  }
  return MGS_OK;
}

int mgs_selftest(mgs_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  int* d = nullptr;
  MGS_HIP(hipMalloc(&d, sizeof(int)), "hipMalloc");
  int h = 0;
  hipError_t e = launch_zero_bytes(d, sizeof(int), stream);
  if (e == hipSuccess) e = launch_selftest(d, stream);
  if (e == hipSuccess) e = hipMemcpyAsync(&h, d, sizeof(int), hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  (void)hipFree(d);
  MGS_HIP(e, "selftest");
  if (h != 0) { set_error("wave64 primitive self-test failed, mask 0x%x", h); return h; }
  return MGS_OK;
}

int mgs_calibration_kernel(int iters, float* sink, mgs_stream_t stream_) {
  if (iters < 1 || !sink) { set_error("calibration: iters >= 1 and a sink of 256 * 1024 floats"); return MGS_ERR_INVALID_ARG; }
  MGS_HIP(launch_calibration(iters, sink, (hipStream_t)stream_), "calibration kernel");
  return MGS_OK;
}

}  // extern "C"
