/*
 * mgsplat.h -- C ABI of libmgsplat.so, the MI355X (gfx950) Gaussian-splatting hot path.
 *
 * This is the drop-in boundary.  Each entry point names the reference interface it replaces.
 *   RAST = third_party/gaussian-splatting/submodules/diff-gaussian-rasterization  (reference tree)
 *   MG   = agents/manigaussian_bc                                                 (reference tree)
 *
 * Reference FFI today (pybind11, torch types): RAST/ext.cpp:15-19 exports
 *   rasterize_gaussians           -> RasterizeGaussiansCUDA          (RAST/rasterize_points.cu:35-128)
 *   rasterize_gaussians_backward  -> RasterizeGaussiansBackwardCUDA  (RAST/rasterize_points.cu:130-225)
 *   mark_visible                  -> markVisible                     (RAST/rasterize_points.cu:227-246)
 * which wrap CudaRasterizer::Rasterizer::{forward,backward,markVisible}
 * (RAST/cuda_rasterizer/rasterizer.h:20-92).
 *
 * Differences that the C ABI forces, all documented in INTEGRATION.md:
 *   - no torch types: plain device pointers + sizes; the CALLER owns every buffer (outputs and the
 *     three opaque workspaces geom/binning/img that the reference grows through a std::function
 *     callback, RAST/rasterize_points.cu:27-33).  Sizes come from mgs_*_bytes().
 *   - the reference's forward is split in two calls because the binning workspace is sized by
 *     num_rendered, which the reference reads back mid-call (RAST/cuda_rasterizer/rasterizer_impl.cu:284).
 *   - every call takes an explicit hipStream_t (the reference uses the legacy default stream).
 *   - F (feature channels) is a run-time value; the reference fixes it at compile time
 *     (RAST/cuda_rasterizer/config.h:16).
 * All tensors are contiguous row-major float32 unless noted, on the device the stream belongs to.
 * All functions return 0 on success, <0 on error (message via mgs_last_error(), thread-local).
 */
#ifndef MGSPLAT_H_
#define MGSPLAT_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MGS_ABI_VERSION 17

/* error codes */
#define MGS_OK 0
#define MGS_ERR_INVALID_ARG (-1)   /* bad shape / null pointer / unsupported F */
#define MGS_ERR_HIP (-2)           /* a HIP runtime call or (debug=1) a kernel failed */
#define MGS_ERR_WORKSPACE (-3)     /* a caller-provided workspace is too small */
#define MGS_ERR_NON_RGB (-4)       /* reference: "For non-RGB, provide precomputed Gaussian colors!" */
#define MGS_NEED_CAPACITY 1        /* the binning workspace holds fewer instances / chunk records than this scene needs */
#define MGS_PENDING 2              /* mgs_forward_result: the device has not reported yet */
#define MGS_RETRY_TABLE_INIT 3     /* mgs_forward_result (ABI v8): the preprocess launch's table hand-shake gave up (a workgroup
                                      made no progress for ~1 s): nothing was binned, the images are background only.  Run the
                                      forward again on the same workspaces with opt.table_init = 1 (every blocking forward does
                                      that by itself; an asynchronous one reports it here instead of a generic MGS_ERR_HIP) */

#define MGS_MAX_FEATURE_CHANNELS 64
#define MGS_MAX_VIEWS 16             /* views of a batch; also the most Gaussian sets of a set batch */

typedef void* mgs_stream_t; /* hipStream_t */

/* Per-call tuning.  Every switch selects another implementation of the same result contract; NONE of them changes the
 * layout of a workspace, so a forward and its backward may even run under different values.  There is no process-wide
 * option state: a zero-initialised MgsRasterArgs carries `set == 0`, which means "all defaults" (mgs_options_default). */
typedef struct MgsOptions {
  int32_t set;          /* 0: ignore the fields below and use the defaults                                        */
  int32_t tight_bins;   /* 1*: drop (Gaussian, tile) instances whose alpha >= 1/255 footprint misses the tile      */
  int32_t fast_exp;     /* 0*: the reference's exp, bit for bit (ocml expf); 1: v_exp_f32 (rel. error ~2e-7 |x|, -2.4 % time) */
  int32_t exact_cull;   /* 1*: exact ellipse-vs-block test on top of the bounding-box test in the render forward   */
  int32_t bin_mode;     /* 2*: per-tile tables in LDS (up to 4096 tiles; more: as 0) and the lists ordered by ONE bucket-rank
                           launch (one workgroup per tile, keys in registers / LDS: ABI v8); 1: tables in LDS, segment sort +
                           rank merge (rounds 2-5); 0: tables in memory, one atomic per instance, segment sort + rank merge --
                           any tile count.  Every mode yields the reference's per-tile order (depth bits, then index)     */
  int32_t seg;          /* 2048*: keys per LDS-sorted segment (512, 1024, 2048, 4096: for lists of >> 8192 per tile)  */
  int32_t gm_waves;     /* 12*: render backward (one workgroup per CU): 12 waves x 168 registers, two pixels per step;
                           16 / 8: the one-pixel-per-step forms of rounds 2-4 (16 x 128 / 8 x 256 registers)            */
  int32_t dbg;          /* 0*: diagnostic bits, every one of them here (A/B switches and test hooks):
                             256      phase timelines: render forward, render backward, bucket rank (mgs_debug_read_trace*)
                             512      test hook: the table-zeroing workgroup of the forward preprocess sleeps ~0.3 ms first
                             1024     test hook: it never publishes the tables, the hand-shake gives up after ~1 s
                             2048     render backward: a block's chunks 4..7 go to waves 4..7 (default: 7..4)
                             0x7000   bits 12-14 = 1 + log2 of the bucket rank's parts per tile (0: chosen by the tile count)
                             32768    direct binning off: the bin scatter launch writes the tile keys
                             1 << 16  render backward (12 waves): the extra chunks 8, 9 are not split between two waves
                             1 << 17  render forward: every chunk of a round is evaluated ahead of the round's one barrier
                                      (default: the chunks of the second slot only as far as a pixel is alive entering them)
                           512 and 1024 reach the forward preprocess only; a forward retried after a hand-shake give-up
                           runs without them                                                                               */
  int32_t table_init;   /* 0*: the forward preprocess launch zeroes its own tile tables (workgroup 0 + a bounded hand-shake:
                           one launch fewer); 1: a zero-fill launch ahead of it -- no workgroup ever waits for another.
                           debug = 1 implies 1; every blocking forward (fused with or without host_status, the two-call
                           stage 1, the view batch) whose hand-shake gave up re-runs itself with 1                          */
} MgsOptions;
void mgs_options_default(MgsOptions* o);  /* fills every field, set = 1 */

/* Per-view configuration + inputs shared by forward and backward.
 * Mirrors the argument lists of Rasterizer::forward / ::backward (RAST/cuda_rasterizer/rasterizer.h:35-91)
 * and the fields of GaussianRasterizationSettings (RAST/diff_gaussian_rasterization/__init__.py:166-179). */
typedef struct MgsRasterArgs {
  int32_t P;               /* number of Gaussians (means3D.size(0))                                   */
  int32_t D;               /* active SH degree (settings.sh_degree)                                   */
  int32_t M;               /* SH coefficients per Gaussian (sh.size(1)), 0 when colors_precomp given  */
  int32_t F;               /* feature channels (language_feature.size(1)); ignored if !include_feature */
  int32_t W, H;            /* image size                                                              */
  float tanfovx, tanfovy;  /* may be NEGATIVE (PyRep focal convention)           */
  float scale_modifier;
  int32_t prefiltered;     /* reference traps the device if a culled point shows up; here: error flag */
  int32_t debug;           /* 1: synchronise + check after every stage (RAST auxiliary.h:166-173)     */
  int32_t include_feature;
  const float* background;      /* [3]                                                                */
  const float* means3D;         /* [P,3]                                                              */
  const float* shs;             /* [P,M,3] or NULL                                                    */
  const float* colors_precomp;  /* [P,3]  or NULL (exactly one of shs / colors_precomp)               */
  const float* language_feature;/* [P,F]  or NULL when !include_feature                               */
  const float* opacities;       /* [P,1]  (forward only; backward reads it from the geom workspace)   */
  const float* scales;          /* [P,3]  or NULL                                                     */
  const float* rotations;       /* [P,4]  or NULL (r,x,y,z), used un-normalised like the reference    */
  const float* cov3D_precomp;   /* [P,6]  or NULL (exactly one of scales+rotations / cov3D_precomp)   */
  const float* viewmatrix;      /* [16] transposed world->view, m[col*4+row]                          */
  const float* projmatrix;      /* [16] transposed full projection                                    */
  const float* campos;          /* [3]                                                                */
  /* opaque workspaces, caller-allocated device memory (uint8 tensors in the reference) */
  void* geom;    size_t geom_bytes;     /* >= mgs_geom_bytes(P, M, W, H)      */
  void* binning; size_t binning_bytes;  /* >= mgs_binning_bytes2(binning_capacity, chunk_pool, W, H, F)                */
  void* img;     size_t img_bytes;      /* >= mgs_img_bytes(W, H)             */
  /* Optional: the accumulator block of a LATER backward (its scratch followed by dL_dcolors and dL_dfeature,
   * contiguous, a multiple of 16 bytes).  Forward: if non-NULL the preprocess kernel zeroes it on the side, so the
   * backward needs no fill.  Backward: accum_prezeroed != 0 promises exactly that (and that nothing touched it since). */
  void* bwd_accum; size_t bwd_accum_bytes;
  int32_t accum_prezeroed;
  /* How the binning workspace is carved; forward and backward must pass the SAME pair (it is not an option: it describes
   * the buffer).  binning_capacity = instances it holds (0: the largest count that fits binning_bytes with a worst-case
   * chunk pool, i.e. a buffer sized by mgs_binning_bytes); chunk_pool = chunk records of the render state (0: the worst
   * case for that capacity, mgs_chunk_pool_max; a caller that remembers the `chunks_used` of earlier forwards of the same
   * scene can pass a fraction of it: ~6x less memory at BASELINE configs[2]). */
  int32_t binning_capacity;
  int32_t chunk_pool;
  uint32_t status_tag;     /* low 16 bits are echoed in the status words of an asynchronous forward                    */
  int32_t async_forward;   /* mgs_rasterize_forward[_views]: 1 = enqueue and return, see below                         */
  MgsOptions opt;
} MgsRasterArgs;

int mgs_abi_version(void);
const char* mgs_last_error(void);
/* 16 hex digits: SHA-256 prefix over the sources this binary was compiled from (csrc/Makefile).  Measurements kept under
 * profiles/ carry it, so that evidence can be matched to the binary being timed -- not to a working tree. */
const char* mgs_build_id(void);

/* Process-wide DIAGNOSTICS only -- never results, kernels or layouts (those are MgsOptions, per call).  The one key is
 * "profile": 0 off, 1 hipEvents around the render backward, 2 around every stage (mgs_profile_read). */
int mgs_set_option(const char* key, int value);
int mgs_get_option(const char* key);

/* Workspace sizes.  Replace required<GeometryState/ImageState/BinningState>()
 * (RAST/cuda_rasterizer/rasterizer_impl.h:65-72, rasterizer_impl.cu:155-194). */
size_t mgs_geom_bytes(int P, int M, int W, int H);
size_t mgs_img_bytes(int W, int H);
size_t mgs_binning_bytes(int R, int W, int H, int F);  /* F = feature channels rendered (0 if none); worst-case chunk pool */
size_t mgs_binning_bytes2(int R, int chunk_pool, int W, int H, int F);  /* explicit pool (0: worst case) */
/* Optional: bytes to ADD to the binning workspace (behind mgs_binning_bytes2 / mgs_views_binning_bytes2) so that the forward
 * preprocess writes the tile keys itself and the bin scatter launch disappears (P Gaussians per view, V views, V = 1 for the
 * single-view calls): tiles x P keys of 8 bytes, 51 MB at 100 000 Gaussians on 128 x 128.  0: not offered for this shape (more
 * than 4 096 tiles, or more than 512 MB).  A workspace without them works as before; a capacity of at least tiles x P / 2
 * instances (every worst-case workspace) gets the same path without them. */
size_t mgs_binning_direct_extra(int P, int V, int W, int H);
int mgs_chunk_pool_max(int R, int W, int H);           /* chunk records of the worst case: every chunk of every 8x8 block */
size_t mgs_backward_scratch_bytes(int P, int M, int F);

/* ---- the workspace plan (ABI v15): HOW LARGE, decided once for every host binding.  Pure functions of (shape, marks,
 * head-room, budget, options): no pointer to device memory, no launch, no HIP call, no state -- they run without a device.
 * WHICH path a call takes (worst case or marks, waiting or not, decline), the marks, the budget's accounting and every
 * message stay with the caller.  The size queries above remain the primitives; the plan is arithmetic over them.
 * A FORWARD AND ITS BACKWARD MUST BE GIVEN THE SAME PLAN: the same (binning_capacity, chunk_pool, binning_bytes) carve the
 * binning workspace in both, and the backward's outputs lie where the gradient plan the forward's bwd_accum was sized from
 * puts them.  Each returns MGS_OK, or MGS_ERR_INVALID_ARG (and leaves its outputs zero) for a negative dimension, W or H < 1,
 * V or S > MGS_MAX_VIEWS, S > 0 without V > 0, or a row count (V x P, S x P) that does not fit the ABI's int. */
typedef struct MgsPlanShape {
  int32_t P, M, F;         /* Gaussians (per set), SH coefficients, feature channels rendered (0: none)              */
  int32_t W, H;
  int32_t V, S;            /* V = 0: a single view, else a batch of V views; S = 0: no set batch, else S Gaussian sets */
  int32_t colors_precomp;  /* a batch's colours are one per Gaussian (else one per (view, Gaussian))                  */
} MgsPlanShape;

/* The arena [geom | img | binning] and the worst case (every Gaussian in every tile: capacity P x tiles of all views, its
 * own chunk pool): it `fits` if the capacity is below 2^30 and its bytes are within budget_bytes. */
typedef struct MgsArenaPlan {
  size_t geom_bytes, img_bytes;  /* mgs_[views_]geom_bytes / img_bytes, each rounded up to 256                        */
  size_t worst_bytes;            /* binning bytes of the worst case (0: its capacity is 2^30 or more)                 */
  int64_t worst_capacity;
  int32_t worst_pool;            /* mgs_[views_]chunk_pool_max of it if it fits, else 0                               */
  int32_t worst_fits;
} MgsArenaPlan;
int mgs_plan_arena(const MgsPlanShape* s, int64_t budget_bytes, MgsArenaPlan* out);
/* Bytes of the binning part for (capacity, chunk_pool; 0: the worst case for the capacity).  with_direct_room: plus
 * mgs_binning_direct_extra behind it, for a NAMED capacity (MgsRasterArgs.binning_capacity > 0) that is not the worst case
 * (which covers the keys by itself).  0: bad shape, or a capacity that does not fit the ABI's int. */
size_t mgs_plan_binning_bytes(const MgsPlanShape* s, int64_t capacity, int64_t chunk_pool, int with_direct_room);

/* (capacity, chunk pool) of a forward that goes by what earlier forwards of its shape needed:
 *   MGS_SIZE_HEADROOM  no wait: the marks (R instances, `chunks` records) times the two head-room factors (in [1, 1024)), truncated,
 *                      plus 4096 instances / 64 records
 *   MGS_SIZE_COUNT     a forward that waits for the preprocess, its retry, a recovery: R (a mark, or the count the device
 *                      reported) + R / 4 + 4096; R < 0 (nothing known: first call of a shape): 4 x max(V, 1) x P + 4096.
 *                      Pool 0: the worst case for the capacity -- cannot overflow.  chunks and the factors are ignored. */
#define MGS_SIZE_HEADROOM 0
#define MGS_SIZE_COUNT 1
int mgs_plan_capacity(const MgsPlanShape* s, int how, int64_t R, int64_t chunks, double head_instances, double head_chunks,
                      int64_t* capacity, int64_t* chunk_pool);

/* Per-call options tuned from the mark R of the shape (instances binned by earlier forwards), in place: seg 2048 -> 4096
 * above 8192 instances per tile (each key is ranked in half as many segments); bin_mode 2 -> 1 above 24576 per tile (the
 * segment sort + rank merge spreads a very long list over one workgroup per segment), seg likewise.  A seg other than 2048
 * was set on purpose and stays.  R <= 0: nothing changes. */
int mgs_plan_options(const MgsPlanShape* s, int64_t R, MgsOptions* opt);

/* The backward's single allocation, offsets in FLOATS: [scratch | dL_dcolors | dL_dfeature | means3D | opacity | sh | scales
 * | rotations | cov3D | means2D | pad].  The first three regions are the accumulator block (MgsRasterArgs.bwd_accum,
 * accum_bytes of it: may reach into the next, fully rewritten, region); the gradients of the Gaussian parameters are
 * contiguous.  A batch has V x P means2D rows and, unless colors_precomp, V x P colour rows; a set batch S x P rows of
 * every per-Gaussian gradient. */
typedef struct MgsGradientPlan {
  int64_t scratch, colors, feature, means3D, opacity, sh, scales, rotations, cov3D, means2D, pad;
  int64_t total;       /* floats */
  size_t accum_bytes;
} MgsGradientPlan;
int mgs_plan_gradients(const MgsPlanShape* s, MgsGradientPlan* out);

/* ---- the report ledger (ABI v17): WHO IS OUTSTANDING, WHAT WAS LEARNED, WHAT TO SAY -- the host-side accounting of the
 * asynchronous forward (mgs_rasterize_forward with async_forward = 1, below), kept once in this library for every host binding
 * that loads it: a process that drives the rasterizer through two bindings sees one ring, one set of marks, one budget and one
 * list of outstanding forwards per device, and every overflow / hand-shake message has one wording.  Sizing (the plan, above),
 * launching, allocation and the autograd node stay with the bindings.  Plain host code: it never calls back into a binding
 * except through the `sync_fn` of a drain, and calls HIP only for that synchronisation when no `sync_fn` is given.  State is
 * per device index (0 .. MGS_LEDGER_MAX_DEVICES - 1); each device has one mutex, a leaf lock.  Unless said otherwise a
 * function returns MGS_OK or MGS_ERR_INVALID_ARG (bad device index / NULL; mgs_last_error()). */
#define MGS_LEDGER_MAX_DEVICES 64
#define MGS_LEDGER_SLOT_WORDS 4    /* 64-bit words per status slot: three used (mgs_rasterize_forward host_status), one pad */

#define MGS_MODE_SAFE 0            /* see manigaussian_amd/_state.py for what the modes and policies mean to a caller */
#define MGS_MODE_ASYNC 1
#define MGS_MODE_BLOCKING 2
#define MGS_OVERFLOW_REPAIR 0
#define MGS_OVERFLOW_RAISE 1
typedef struct MgsLedgerConfig {
  int32_t mode;                    /* MGS_MODE_*: read by the bindings, which decide the path of a call                      */
  int32_t overflow_policy;         /* MGS_OVERFLOW_*: what an overflow that a backward can still repair turns into           */
  double head_instances, head_chunks;  /* head-room of mgs_marks_guess over the marks, each in [1, 1024)                     */
  int64_t safe_bytes;              /* budget of worst-case workspaces per device; < 0: the binding's default for the device  */
} MgsLedgerConfig;
void mgs_ledger_set_config(const MgsLedgerConfig* c);
void mgs_ledger_get_config(MgsLedgerConfig* c);

/* The ring of status slots, ONE per device: `words` (nslots x MGS_LEDGER_SLOT_WORDS 64-bit words of pinned, device-mapped host
 * memory that outlives the process's use of the device, or plain memory in a host test) is adopted if the device has no ring
 * yet.  Returns the ring in force -- the caller's if it was adopted, NULL if there is none (words = NULL only asks).
 * mgs_ledger_take_slot hands out slots round-robin with a fresh 16-bit tag, skipping the slots of captured tickets;
 * MGS_ERR_INVALID_ARG "all status slots are held by captured graphs" when none is free. */
uint64_t* mgs_ledger_ring(int device, uint64_t* words, int nslots);
int mgs_ledger_ring_slots(int device);
int mgs_ledger_take_slot(int device, uint64_t** slot, uint32_t* tag);

/* The high-water marks per (device, shape): instances binned and chunk records used by earlier forwards of the shape.
 * V = 0: a single view; V >= 1: a batch of V views; S >= 1: a batch of V views of S Gaussian sets.  chunks < 0: unknown (the
 * pool must be the worst case).  get / erase / guess return 1 (found, erased, a guess) or 0; keys returns how many there are
 * and writes at most `room` of them.  learn: marks only grow (R, chunks < 0: nothing known of that one); pool_unknown resets
 * the chunk mark.  guess: none without a chunk mark, else mgs_plan_capacity(MGS_SIZE_HEADROOM) with the configured head-room. */
typedef struct MgsMarkKey { int32_t V, S, P, W, H, F, tight_bins; } MgsMarkKey;
int mgs_marks_get(int device, const MgsMarkKey* key, int64_t* R, int64_t* chunks);
int mgs_marks_set(int device, const MgsMarkKey* key, int64_t R, int64_t chunks);
int mgs_marks_erase(int device, const MgsMarkKey* key);
int mgs_marks_keys(int device, MgsMarkKey* out, int room);
int mgs_marks_learn(int device, const MgsMarkKey* key, int64_t R, int64_t chunks, int pool_unknown);
int mgs_marks_guess(int device, const MgsMarkKey* key, int64_t* capacity, int64_t* chunk_pool);

/* The budget: bytes of WORST-CASE workspaces that live forwards of the device hold.  hold reserves `bytes` if (what is held +
 * bytes) <= budget -- added first, checked, rolled back: two callers cannot both take the last room -- and returns 1, else 0
 * and nothing changed.  Whoever was granted a hold gives it back with unhold. */
int mgs_ledger_hold(int device, int64_t bytes, int64_t budget);
void mgs_ledger_unhold(int device, int64_t bytes);
int64_t mgs_ledger_held(int device);

/* A ticket: one enqueued forward whose report has not been folded into the marks.  The ledger copies `a` AS GIVEN TO THAT RUN
 * (a caller may rewrite its struct for a re-run) and holds one reference while the ticket is outstanding or captured; the
 * caller holds the other and gives it up with release.  V: 0, or the views of a batch (mgs_forward_result_views decodes).
 * RECOVERABLE: a backward will follow and can re-render; CAPTURED: recorded into a HIP graph -- it reports at every replay,
 * keeps its slot for good and is read by mgs_ledger_check_captured only.
 * poll never blocks: the code of mgs_forward_result (MGS_PENDING until both words carry the ticket's tag) and the counts that
 * have arrived (-1 before).  backward_enqueued: the backward has been enqueued on whatever the forward left -- too late to
 * repair.  superseded: a recovery ran this forward again (under a ticket of its own); this one is accounted at most once more,
 * as a warning. */
#define MGS_TICKET_RECOVERABLE 1
#define MGS_TICKET_CAPTURED 2
typedef struct MgsTicket MgsTicket;
typedef struct MgsReport { int32_t rc, num_rendered, chunks_used, ref_rendered; } MgsReport;
MgsTicket* mgs_ledger_add(int device, const MgsRasterArgs* a, int32_t V, const uint64_t* slot, const MgsMarkKey* key,
                          int flags);  /* NULL: bad argument */
int mgs_ledger_poll(MgsTicket* t, MgsReport* report);
void mgs_ledger_backward_enqueued(MgsTicket* t);
void mgs_ledger_superseded(MgsTicket* t);
void mgs_ledger_release(MgsTicket* t);
int mgs_ledger_outstanding(int device);  /* tickets not accounted yet (captured ones apart) */

/* drain: read every report that has arrived and fold it into the marks.  The device is synchronised -- once, with the
 * device's mutex NOT held, through sync_fn(ctx), or by hipDeviceSynchronize on `device` if sync_fn is NULL -- only if `wait`,
 * or if more than half the ring is outstanding; a ticket that was outstanding at the synchronisation and is still pending after
 * it fails with "finished without reporting its instance count" (tickets added meanwhile are kept).  `out`: the text the
 * caller must raise (the first one; NULL: none) and the warnings it must issue, in this thread's storage, valid until the
 * thread's next ledger call.  An overflow that its backward can still repair (RECOVERABLE, backward not enqueued, policy
 * repair) is a warning; under policy raise, or too late, an error -- once.  check_captured polls the captured tickets anew. */
typedef struct MgsLedgerOut {
  const char* error;
  int32_t n_warnings;
  const char* const* warnings;
} MgsLedgerOut;
int mgs_ledger_drain(int device, int wait, void (*sync_fn)(void*), void* ctx, MgsLedgerOut* out);
int mgs_ledger_check_captured(int device, MgsLedgerOut* out);
/* What a backward raises under policy raise when ITS forward's report (rc: MGS_NEED_CAPACITY or MGS_RETRY_TABLE_INIT) was
 * already accounted by an earlier drain. */
const char* mgs_ledger_lost_step_message(int rc);

/* Forward, stage 1: preprocess + tile-count scan (K2, K3 of SURVEY.md 2b).
 * Replaces the first half of Rasterizer::forward (RAST/cuda_rasterizer/rasterizer_impl.cu:198-284).
 * Writes radii[P] (int32) and the geom workspace; *num_rendered (HOST int) receives the number of
 * (Gaussian, tile) instances of the reference's 3-sigma tile rects -- THE REFERENCE'S INTEGER (rasterizer_impl.cu:280-284),
 * whatever MgsOptions.tight_bins says (the instances actually binned are fewer under tight_bins = 1; the count is a safe
 * size for stage 2's workspace) -- this call synchronises the stream once, exactly where the reference does its blocking
 * cudaMemcpy (rasterizer_impl.cu:284).  If the preprocess's table hand-shake gave up (MGS_RETRY_TABLE_INIT), the call
 * synchronises and runs the preprocess again with opt.table_init = 1 by itself. */
int mgs_rasterize_forward_preprocess(const MgsRasterArgs* a, int32_t* radii, int32_t* num_rendered,
                                     mgs_stream_t stream);

/* Forward, stage 2: per-tile depth-ordered instance lists (what duplicate-with-keys + radix sort + tile ranges produce in
 * the reference; here: key scatter, segment sort, rank merge) and the alpha-composite render (K4-K7).
 * Replaces rasterizer_impl.cu:286-355.  radii: the [P] int32 array stage 1 wrote.  out_color [3,H,W];
 * out_feature [F,H,W] (untouched if !include_feature).  Both are fully written (no pre-zeroing needed). */
int mgs_rasterize_forward_render(const MgsRasterArgs* a, int32_t num_rendered, const int32_t* radii,
                                 float* out_color, float* out_feature, mgs_stream_t stream);

/* Fused forward: stage 1 + stage 2 in one call with NO mid-call stream synchronisation (the reference blocks on a
 * cudaMemcpy at rasterizer_impl.cu:284; on MI355X that bubble costs more than the binning).  The binning workspace is
 * sized by the CALLER's guess (a->binning_capacity / a->chunk_pool, e.g. the high-water marks of earlier calls).
 *   host_status: 24 bytes (three 64-bit words) of PINNED, device-mapped host memory (hipHostMalloc / torch pin_memory),
 *     8-byte aligned, owned by this call until its result has been read; the device reports {tag, flags, instances binned}
 *     through word 0 and {tag, the reference's num_rendered} through word 2 as soon as the preprocess has run (word 2 is
 *     stored first: whoever sees word 0 sees word 2), and {tag, overflow, chunk records used} through word 1 when the render
 *     has finished.  The call sets the words to "pending" before enqueueing.  NULL: the call reads the counts back with a
 *     blocking copy instead (same results, slower, no chunk-pool report: a->chunk_pool must then be 0).
 *   a->async_forward == 0: returns once words 0 and 2 have arrived, i.e. it waits for the PREPROCESS only -- binning and
 *     render are enqueued and may still be running (ABI v7; v6 synchronised the stream here to read the reference's count):
 *     MGS_OK (images enqueued, *num_rendered set -- the reference's integer, see mgs_rasterize_forward_preprocess;
 *     mgs_forward_result reports the instances actually binned, which is what sizes a workspace) or MGS_NEED_CAPACITY
 *     (*num_rendered set, geom + radii valid, images NOT rendered: call mgs_rasterize_forward_render with a binning
 *     workspace of at least mgs_binning_bytes(*num_rendered, W, H, F)).  A table hand-shake that gave up is retried inside
 *     the call with opt.table_init = 1, on either path (host_status or the blocking read-back).
 *     A chunk-pool overflow (only possible with a->chunk_pool != 0) is reported by mgs_forward_result.
 *   a->async_forward == 1: enqueues everything and returns MGS_OK at once with *num_rendered = -1: no host-device
 *     synchronisation at all (the call can be captured into a HIP graph together with its backward).  If the scene outgrew
 *     the workspace the kernels render nothing valid and say so in the status words: the caller MUST look at
 *     mgs_forward_result before trusting the images -- at the latest when it next synchronises with the stream.  The
 *     backward may be enqueued (num_rendered = -1) before the result is known; it then computes on whatever the forward
 *     left and is equally invalid after an overflow. */
int mgs_rasterize_forward(const MgsRasterArgs* a, int32_t* radii, float* out_color, float* out_feature,
                          int32_t* num_rendered, uint64_t* host_status, mgs_stream_t stream);

/* Host-side decode of the status words of a forward (no HIP call, never blocks).  `a`: the arguments of that forward
 * (status_tag, binning_capacity, chunk_pool, binning_bytes and the shape are read).  Returns MGS_PENDING until both words
 * carry this call's tag; then MGS_OK, MGS_NEED_CAPACITY (instances > capacity, or the chunk pool overflowed: the images
 * and any backward of that forward are invalid), MGS_RETRY_TABLE_INIT (see the code) or MGS_ERR_INVALID_ARG (prefiltered
 * violation).  *num_rendered and
 * *chunks_used (each optional) receive the counts as soon as their word has arrived (-1 before); *ref_rendered (optional)
 * the reference's num_rendered (the 3-sigma-rect instances, RAST/cuda_rasterizer/rasterizer_impl.cu:280-284): the same
 * integer the blocking entry points return, so every path hands the caller one number. */
int mgs_forward_result(const MgsRasterArgs* a, const uint64_t* host_status, int32_t* num_rendered, int32_t* chunks_used,
                       int32_t* ref_rendered);

/* Backward (K8-K10).  Replaces Rasterizer::backward (rasterizer_impl.cu:359-463) and the output
 * allocation of RasterizeGaussiansBackwardCUDA (rasterize_points.cu:167-184).  Every non-NULL output
 * is fully written (zero where the reference leaves its zero-initialised value).
 *   dL_dout_color [3,H,W], dL_dout_feature [F,H,W] (NULL if !include_feature)
 *   dL_dmeans2D [P,3] (NDC units, z = 0), dL_dopacity [P,1], dL_dcolors [P,3], dL_dfeature [P,F],
 *   dL_dmeans3D [P,3], dL_dcov3D [P,6], dL_dsh [P,M,3], dL_dscales [P,3], dL_drotations [P,4],
 *   dL_dconic [P,4] (optional, may be NULL; reference keeps it internal).
 * scratch: >= mgs_backward_scratch_bytes(P, M, F) device bytes, contents undefined on entry.
 * a->language_feature must be 16-byte aligned (feature rows are read as float4; MGS_ERR_INVALID_ARG otherwise). */
/* num_rendered: the forward's count, or -1 if the caller has not looked yet (asynchronous forward). */
int mgs_rasterize_backward(const MgsRasterArgs* a, int32_t num_rendered, const int32_t* radii,
                           const float* dL_dout_color, const float* dL_dout_feature, float* dL_dmeans2D,
                           float* dL_dconic, float* dL_dopacity, float* dL_dcolors, float* dL_dfeature,
                           float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscales,
                           float* dL_drotations, void* scratch, size_t scratch_bytes, mgs_stream_t stream);

/* ---- multi-view batches: V views of one Gaussian set in one call (the reference renders one view per
 * call, MG/neural_rendering.py:386 `assert bs == 1`).  MgsRasterArgs carries everything shared (its viewmatrix / projmatrix /
 * campos / tanfov fields are ignored); images are [V,3,H,W] / [V,F,H,W]; radii, dL_dmeans2D, dL_dconic are [V,P,.];
 * dL_dcolors is [V,P,3] with SH colours (colours differ per view) and [P,3] with colors_precomp; every other gradient is
 * per Gaussian, summed over the views on the device.  Workspaces are sized by the mgs_views_*_bytes functions.
 * host_status is required (see mgs_rasterize_forward; async_forward and the hand-shake retry work the same).  Needs V <= 16 (any tile count; V * tiles <= 4096 keeps the
 * binning tables in LDS). */
typedef struct MgsView {
  float tanfovx, tanfovy;
  const float* viewmatrix;  /* [16] */
  const float* projmatrix;  /* [16] */
  const float* campos;      /* [3]  */
} MgsView;
size_t mgs_views_geom_bytes(int P, int M, int W, int H, int V);
size_t mgs_views_img_bytes(int W, int H, int V);
size_t mgs_views_binning_bytes(int R, int W, int H, int F, int V);
size_t mgs_views_binning_bytes2(int R, int chunk_pool, int W, int H, int F, int V);
int mgs_views_chunk_pool_max(int R, int W, int H, int V);
size_t mgs_views_backward_scratch_bytes(int P, int M, int F, int V);
int mgs_rasterize_forward_views(const MgsRasterArgs* a, int32_t V, const MgsView* views, int32_t* radii, float* out_color,
                                float* out_feature, int32_t* num_rendered, uint64_t* host_status, mgs_stream_t stream);
int mgs_forward_result_views(const MgsRasterArgs* a, int32_t V, const uint64_t* host_status, int32_t* num_rendered,
                             int32_t* chunks_used, int32_t* ref_rendered);  /* mgs_forward_result for a batch of V views */
int mgs_rasterize_backward_views(const MgsRasterArgs* a, int32_t V, const MgsView* views, int32_t num_rendered,
                                 const int32_t* radii, const float* dL_dout_color, const float* dL_dout_feature,
                                 float* dL_dmeans2D, float* dL_dconic, float* dL_dopacity, float* dL_dcolors,
                                 float* dL_dfeature, float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscales,
                                 float* dL_drotations, void* scratch, size_t scratch_bytes, mgs_stream_t stream);

/* ---- set batches (ABI v9): V views of S Gaussian sets of one size in one call.  ManiGaussian's training step renders the
 * current frame and the deformed next frame, two sets (MG/neural_rendering.py:283,324).  a->P is the number of Gaussians PER SET;
 * every attribute pointer of `a` is [S,P,.] (sets stacked along the leading dimension), view v renders set view_set[v]
 * (host array of V ints, 0 <= view_set[v] < S <= 16; a set no view renders is allowed).  Images, radii, dL_dmeans2D,
 * dL_dconic and, with SH colours, dL_dcolors are per view as in a view batch; every other gradient is [S,P,.]: row (s, i) sums
 * the views of set s, rows of a set no view renders are zero.  Each view's image and radii are those of a single-view call on
 * its set, bit for bit.  Workspaces are a V-view batch's (mgs_views_*_bytes, mgs_binning_direct_extra(P, V, ..));
 * mgs_forward_result_views reads the status words.  The accumulator block (bwd_accum) is acc16 | dL_dcolors | dL_dfeature
 * (ABI v11: the scratch holds one 64-byte row of 16 floats per (view, Gaussian) -- the six geometry sums and, with SH colours,
 * the three colour sums, which the preprocess backward copies to dL_dcolors -- where v10 had rows of 8)
 * with S x P rows for dL_dfeature and, with colors_precomp, for dL_dcolors.  With S = 1 and every view on set 0 this is
 * mgs_rasterize_forward_views / mgs_rasterize_backward_views. */
size_t mgs_sets_backward_scratch_bytes(int P, int M, int F, int V, int S);
int mgs_rasterize_forward_sets(const MgsRasterArgs* a, int32_t V, const MgsView* views, int32_t S, const int32_t* view_set,
                               int32_t* radii, float* out_color, float* out_feature, int32_t* num_rendered,
                               uint64_t* host_status, mgs_stream_t stream);
int mgs_rasterize_backward_sets(const MgsRasterArgs* a, int32_t V, const MgsView* views, int32_t S, const int32_t* view_set,
                                int32_t num_rendered, const int32_t* radii, const float* dL_dout_color,
                                const float* dL_dout_feature, float* dL_dmeans2D, float* dL_dconic, float* dL_dopacity,
                                float* dL_dcolors, float* dL_dfeature, float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh,
                                float* dL_dscales, float* dL_drotations, void* scratch, size_t scratch_bytes,
                                mgs_stream_t stream);

/* Replaces Rasterizer::markVisible (rasterizer_impl.cu:141-153).  present: uint8 [P] (torch.bool). */
int mgs_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                     uint8_t* present, mgs_stream_t stream);

/* ---- deformation field: fused input assembly and apply epilogue (MG/models_embed.py:255-304) ----
 * dyna_input[n, :] = cat(point_latent[n,0:DL], xyz[n,3], f_dc[n,3], f_rest[n,9], rot[n,4], scale[n,3],
 *                        opacity[n,1], (feature[n,3] iff feature != NULL), PE(canon_xyz[n])[39] or z_feature,
 *                        action[0, 0:DA] broadcast)                         (models_embed.py:258-287)
 * z_feature is passed precomputed ([N, DZ], models_embed.py:208-213); sh is [N,4,3] = (f_dc, f_rest).
 * Row stride of out = DL + 23 + (feature?3:0) + DZ + DA. */
int mgs_deform_assemble_forward(int N, int DL, int DZ, int DA, const float* point_latent,
                                const float* xyz, const float* sh, const float* rot, const float* scale,
                                const float* opacity, const float* feature, const float* z_feature,
                                const float* action, float* out, mgs_stream_t stream);
/* Gradient of the assembly: only point_latent and z_feature receive gradient (everything else is
 * .detach()ed in the reference).  g_out [N, stride] -> g_point_latent [N,DL], g_z_feature [N,DZ]. */
int mgs_deform_assemble_backward(int N, int DL, int DZ, int DA, int has_feature, const float* g_out,
                                 float* g_point_latent, float* g_z_feature, mgs_stream_t stream);
/* next.xyz = xyz + delta[:,0:3]; next.rot = normalize(rot + delta[:,3:7])   (models_embed.py:295-299) */
int mgs_deform_apply_forward(int N, const float* xyz, const float* rot, const float* delta /*[N,7]*/,
                             float* xyz_out, float* rot_out, mgs_stream_t stream);
/* g_delta [N,7] from g_xyz_out [N,3], g_rot_out [N,4] (xyz, rot are detached: no other gradient). */
int mgs_deform_apply_backward(int N, const float* rot, const float* delta, const float* g_xyz_out,
                              const float* g_rot_out, float* g_delta, mgs_stream_t stream);

/* ---- deformation field MLP: the elementwise passes between the GEMMs of ResnetFC, fused -----------------------------------
 * (MG/.../resnetfc.py:10-62: ResnetBlockFC  x + fc_1(relu(fc_0(relu(x)))),  :65-177 ResnetFC).  The GEMMs stay with the
 * caller's BLAS; x, act, g_* are row-major [M, N] fp32, N a multiple of 4 with N/4 dividing 256.
 * forward:  relu_out = max(x, 0);  xb_out = x + bias[N]   (either output, and bias, may be NULL) */
int mgs_mlp_relu_bias(int M, int N, const float* x, const float* bias, float* relu_out, float* xb_out,
                      mgs_stream_t stream);
/* backward: g_out = g_pre * (act > 0) [+ g_res];  colsum[n] += sum_m g_out[m][n]  (the bias gradient; NULL: not wanted;
 * the caller zeroes it).  g_out may alias g_pre or g_res. */
int mgs_mlp_relu_backward(int M, int N, const float* g_pre, const float* act, const float* g_res, float* g_out,
                          float* colsum, mgs_stream_t stream);

/* ---- Gaussian-regressor epilogue (MG/models_embed.py:233-253, MG/gaussian_renderer/__init__.py:66-68) ----
 * raw [N,26] = xyz 3 | opacity 1 | scale 3 | rot 4 | f_dc 3 | feature 3 | f_rest 9 (the split of models_embed.py:121,139-141)
 *   xyz = xyz_in + raw.xyz;  opacity = sigmoid;  scale = min(exp, 0.05);  rot = normalize (eps 1e-12);
 *   sh [N,4,3] = (f_dc, f_rest);  feature = raw.feature;  feature_n = feature / (|feature| + 1e-12)
 * backward: any g_* may be NULL (treated as zero); g_raw [N,26] is fully written. */
int mgs_regress_epilogue_forward(int N, const float* raw, const float* xyz_in, float* xyz, float* opacity, float* scale,
                                 float* rot, float* sh, float* feature, float* feature_n, mgs_stream_t stream);
int mgs_regress_epilogue_backward(int N, const float* raw, const float* g_xyz, const float* g_opacity, const float* g_scale,
                                  const float* g_rot, const float* g_sh, const float* g_feature, const float* g_feature_n,
                                  float* g_raw, mgs_stream_t stream);

/* ---- per-point latent: voxel-feature trilinear gather + positional encoding (MG/models_embed.py:147-215, MG/utils.py:133-169) ----
 * out [N, C + 3 + 6K] = [ grid_sample(voxel [C,D,H,W], canon; align_corners, zero padding) | canon | sin/cos(pi 2^k canon) ],
 * canon = (xyz - bounds[0:3]) / (bounds[3:6] - bounds[0:3]); bounds is a HOST array of 6 floats.
 * backward: g_voxel [C,D,H,W] += d out[:, 0:C] / d voxel (atomic; zero it first); g_out rows are row_stride floats apart. */
int mgs_voxel_sample_pe_forward(int N, int C, int D, int H, int W, int K, float freq_factor, const float* bounds_host,
                                const float* voxel, const float* xyz, float* out, mgs_stream_t stream);
int mgs_voxel_sample_backward(int N, int C, int D, int H, int W, const float* bounds_host, const float* xyz,
                              const float* g_out, int row_stride, float* g_voxel, mgs_stream_t stream);

/* ---- camera calibration: replaces NeuralRenderer.get_novel_calib (MG/neural_rendering.py:205-248)
 * with getWorld2View2 / getProjectionMatrix / focal2fov (MG/graphics_utils.py:17-53) folded in.
 * c2w [V,16] = the saved cam2world extrinsics, K [V,9] = intrinsics, both row-major float32.  Outputs (any may be NULL):
 * world_view_transform [V,16], full_proj_transform [V,16] (the transposed matrices the rasterizer takes),
 * camera_center [V,3], fov [V,2] = (FovX, FovY) (negative for negative focal lengths, kept), tanfov [V,2] = tan(Fov/2).
 * mgs_novel_calib: device pointers, one launch on `stream`, no host synchronisation; *singular (device int32, optional,
 * zeroed by the caller) is set to 1 if some cam2world matrix is not invertible.
 * mgs_novel_calib_host: the same routine on host arrays (what a data-loader cache calls once per camera file). */
int mgs_novel_calib(int V, const float* c2w, const float* K, int W, int H, float znear, float zfar, float trans_x,
                    float trans_y, float trans_z, float scale, float* world_view_transform, float* full_proj_transform,
                    float* camera_center, float* fov, float* tanfov, int32_t* singular, mgs_stream_t stream);
int mgs_novel_calib_host(int V, const float* c2w, const float* K, int W, int H, float znear, float zfar, float trans_x,
                         float trans_y, float trans_z, float scale, float* world_view_transform,
                         float* full_proj_transform, float* camera_center, float* fov, float* tanfov);

/* ---- rendering losses (MG/neural_rendering.py:299-329, :90-106 _embed_loss_fn, :22-27 PSNR_torch; MG/loss.py:12-23) ----
 * For V views (1 .. 16) of W x H pixels: color [V,3,H,W] and feature [V,F,H,W] (F <= 64) are the rasterizer's planar outputs,
 * contiguous; gt_rgb / gt_embed are constants addressed by ELEMENT strides {view, channel, row, column} (host arrays of 4),
 * so channel-last and channel-first tensors are read where they lie.  Per view v:
 *   mse[v]   = sum (color - gt_rgb)^2 / (3 N)                            N = W H
 *   psnr[v]  = 20 log10(1 / sqrt(mse[v])), 100 where mse[v] == 0         (computed on the device)
 *   embed[v] = MGS_EMBED_COSINE: 1 - mean_pixels cos(feature_p, gt_embed_p), the norms clamped to 1e-8 outside the graph
 *              (F.cosine_similarity); MGS_EMBED_L2: sum (feature - gt_embed)^2 / (F N); MGS_EMBED_L2_NORM: the same against
 *              (g - min g) / (max g - min g + 1e-12), min / max over the view's target; 0 when feature or gt_embed is NULL
 *   loss     = 0 + sum_v (w[v][0] mse[v] + w[v][1] embed[v]), accumulated in this order
 * weights [V,2]: weights_host (read during the call: the values are kernel arguments, frozen into a captured graph) or
 * weights_dev (read by the kernels: a captured graph follows in-place updates); both NULL: all ones.
 * Outputs: terms [V,3] = (mse, embed, psnr); *loss; g_color [V,3,H,W] / g_feature [V,F,H,W] = d loss / d color, d loss /
 * d feature (either may be NULL: not wanted).  workspace: mgs_render_loss_workspace_bytes(V, W, H) bytes, 16-byte aligned.
 * 2 launches (3 for MGS_EMBED_L2_NORM), no atomics, no host synchronisation: results are bit-identical from run to run.
 * mgs_render_loss_backward: out = *g_up (a device scalar) x unit, both buffers in one launch (a NULL out is skipped). */
#define MGS_EMBED_COSINE 0
#define MGS_EMBED_L2 1
#define MGS_EMBED_L2_NORM 2
size_t mgs_render_loss_workspace_bytes(int V, int W, int H);
int mgs_render_loss_forward(int V, int F, int W, int H, const float* color, const float* gt_rgb, const int64_t* rgb_strides,
                            const float* feature, const float* gt_embed, const int64_t* embed_strides, int embed_fn,
                            const float* weights_host, const float* weights_dev, float* g_color, float* g_feature,
                            float* terms, float* loss, void* workspace, size_t workspace_bytes, mgs_stream_t stream);
int mgs_render_loss_backward(int V, int F, int W, int H, const float* g_up, const float* unit_color, const float* unit_feature,
                             float* out_color, float* out_feature, mgs_stream_t stream);

/* ---- photometric loss: L1 + L2 + D-SSIM (MG/loss.py:9-13 l1_loss, l2_loss; :25-68 gaussian, create_window, ssim, _ssim;
 *      conf/method/ManiGaussian_BC.yaml:97-98 lambda_l1, lambda_ssim; MG/neural_rendering.py:299-307) ----
 * For V views (1 .. 16) of C channels (1 .. 64) of W x H pixels: color [V,C,H,W] is the rasterizer's planar output,
 * contiguous; target is a constant addressed by ELEMENT strides {view, channel, row, column} (a host array of 4), as the
 * rendering losses' targets are.  Per view v, with x the rendered image, y the target and N = C H W:
 *   l1[v]   = sum |x - y| / N                          (d|t|/dt at t == 0 is 0, torch's abs)
 *   l2[v]   = sum (x - y)^2 / N
 *   psnr[v] = 20 log10(1 / sqrt(l2[v])), 100 where l2[v] == 0                  (decided on the device)
 *   ssim[v] = sum m / N,  m = ((2 mx my + C1)(2 sxy + C2)) / ((mx^2 + my^2 + C1)(sx + sy + C2)),  C1 = 0.01^2, C2 = 0.03^2
 *             mx = G*x, my = G*y, sx = G*x^2 - mx^2, sy = G*y^2 - my^2, sxy = G*xy - mx my
 *   loss    = 0 + sum_v (w[v][0] l1[v] + w[v][1] l2[v] + w[v][2] (1 - ssim[v])), accumulated in this order
 * G is loss.py's window: 11 x 11, the outer product of MGS_SSIM_WINDOW with itself, zero padding of 5 (the map has the image's
 * size), applied separably -- rows, then columns.  MGS_SSIM_WINDOW holds the float32 values of loss.gaussian(11, 1.5) bit for
 * bit (exp in double, rounded to float32, divided by their float32 sum; 9 significant digits round-trip a float32).
 * weights [V,3]: weights_host (kernel arguments, frozen into a captured graph) or weights_dev (read by the kernels: a captured
 * graph follows in-place updates); both NULL: all ones.  A zero weight still reports its term and adds an exactly zero gradient.
 * Outputs: terms [V,4] = (l1, l2, ssim, psnr); *loss; unit_grad [V,C,H,W] = d loss / d color (NULL: not wanted; the gradient
 * launch and the three per-pixel maps d m / d mx, d m / d sx, d m / d sxy it convolves are then skipped).
 * workspace: mgs_photometric_workspace_bytes(V, C, W, H) bytes, 16-byte aligned (the three maps and one row of partial sums
 * per workgroup).  3 launches (2 without unit_grad), no atomics, no host synchronisation: bit-identical from run to run.
 * mgs_photometric_backward: out[v] = g_up[v * g_up_stride] x unit_grad[v] in one launch; g_up is device memory, g_up_stride
 * 0 (one scalar for every view: d / d loss) or 1 (one value per view: d / d ssim[v], with weights (0, 0, -1)). */
#define MGS_SSIM_WINDOW_SIZE 11
#define MGS_SSIM_WINDOW { 0.00102838012f, 0.00759875821f, 0.0360007733f, 0.109360687f, 0.213005528f, 0.266011715f, \
                          0.213005528f, 0.109360687f, 0.0360007733f, 0.00759875821f, 0.00102838012f }
#define MGS_PHOTOMETRIC_MAX_CHANNELS 64
size_t mgs_photometric_workspace_bytes(int V, int C, int W, int H);
int mgs_photometric_forward(int V, int C, int W, int H, const float* color, const float* target, const int64_t* target_strides,
                            const float* weights_host, const float* weights_dev, float* unit_grad, float* terms, float* loss,
                            void* workspace, size_t workspace_bytes, mgs_stream_t stream);
int mgs_photometric_backward(int V, int C, int W, int H, const float* g_up, int g_up_stride, const float* unit_grad, float* out,
                             mgs_stream_t stream);

/* ---- fused LAMB step over flat moment buffers (MG/helpers/optim/lamb.py:47-111; no bias correction, as there) ----
 * For any number of parameter tensors, fp32, in TWO launches.  Per tensor, with the hyper-parameters of its group:
 *   g' = grad_scale g;  m = m beta1 + g' (1 - beta1);  v = v beta2 + g' g' (1 - beta2)
 *   u = m / (sqrt(v) + eps) [+ weight_decay p  if weight_decay != 0]
 *   weight_norm = min(sqrt(sum p^2), 10);  adam_norm = sqrt(sum u^2)
 *   trust_ratio = 1 if weight_norm == 0 or adam_norm == 0, else weight_norm / adam_norm      (decided on the device)
 *   p = p - lr (adam ? 1 : trust_ratio) u;   stats[tensor] = {weight_norm, adam_norm, trust_ratio}
 * A tensor is cut into chunks of mgs_lamb_chunk_elems() elements (the last one shorter); a chunk never straddles tensors.
 * All tables live in DEVICE memory and are read by the kernels (the host passes pointers only):
 *   tensors   [n_tensors]  MgsLambTensor: p; g (NULL: the tensor is skipped -- no state, no decay, p and its stats untouched);
 *                          numel; state_off = its first element in exp_avg / exp_avg_sq (a multiple of 4, and the tensor's
 *                          slot there is padded to a multiple of 4 elements); group; flags (MGS_LAMB_*_ALIGNED: that pointer is
 *                          16-byte aligned -> 16-byte accesses, else element-wise; per tensor); chunk0 = its first chunk,
 *                          n_chunks = ceil(numel / chunk elements) >= 1, tensors in chunk order
 *   groups    [n_groups]   MgsLambGroup: 1 - beta is formed by the caller in double and rounded once (torch's scalar alpha);
 *                          lr_dev != NULL: the learning rate is read from that device float at run time (a captured graph
 *                          follows in-place updates), else lr
 *   chunk_map [n_chunks][2] int32 {tensor, chunk inside the tensor}
 * exp_avg, exp_avg_sq: the flat moment buffers (16-byte aligned).  stats: float [n_tensors][3].  zero_grad != 0: g is zeroed
 * after it was read.  workspace: mgs_lamb_workspace_bytes(n_chunks) bytes (one pair of partial sums per chunk).
 * The moments pass writes one partial pair per chunk; every workgroup of the apply pass adds its tensor's pairs in the same
 * fixed order.  No atomics, no host read, no allocation: bit-identical from run to run, capturable into a HIP graph. */
#define MGS_LAMB_P_ALIGNED 1
#define MGS_LAMB_G_ALIGNED 2
typedef struct MgsLambTensor {
  float* p;
  float* g;
  int64_t numel;
  int64_t state_off;
  int32_t group;
  int32_t flags;
  int32_t chunk0;
  int32_t n_chunks;
} MgsLambTensor; /* 48 bytes */
typedef struct MgsLambGroup {
  float lr, beta1, one_minus_beta1, beta2, one_minus_beta2, eps, weight_decay;
  int32_t adam;
  const float* lr_dev;
} MgsLambGroup; /* 40 bytes */
int mgs_lamb_chunk_elems(void);
size_t mgs_lamb_workspace_bytes(int64_t n_chunks);
int mgs_lamb_step(int n_tensors, int n_groups, int64_t n_chunks, const MgsLambTensor* tensors, const MgsLambGroup* groups,
                  const int32_t* chunk_map, float* exp_avg, float* exp_avg_sq, float* stats, float grad_scale, int zero_grad,
                  void* workspace, size_t workspace_bytes, mgs_stream_t stream);

/* ---- the agent's voxel grid, forward only (MG/voxel/voxel_grid.py:168-229, VoxelGrid.coords_to_bounding_voxel_grid) ----
 * Scatter-mean of B clouds of N points, [features | xyz] per point, into V^3 voxels; C = Fc + 7 channels per voxel:
 *   [0, Fc + 3)  the mean of the voxel's points (0 where there is none)      Fc + 3 .. Fc + 5  x, y, z index / V
 *   Fc + 6       occupancy, 0 or 1
 * Per batch item b and axis, every step one fp32 operation and every division correctly rounded, as the reference computes it:
 *   res = (max - min) / (float(V) + 1e-12f);  idx = floor((p - (min - res)) / (res + 1e-12f)) clamped to [0, V + 1]
 * A point with index 0 or V + 1 on some axis lies in the shell the reference crops away and is dropped: points outside the
 * bounds, NaN, +-inf, and a point exactly on the lower bound (fp32 rounding puts it at index 0 in the reference too).
 * Every voxel's points are added in ASCENDING POINT INDEX from 0.0f and divided once by float(count): the order of the
 * reference's CPU scatter_add_, so the grid equals the reference module's CPU result bit for bit and is the same from run to
 * run (no float atomics; integer atomics order nothing that reaches the result).  Any multiplicity, all N in one voxel included.
 *   coords [B,N,3], features [B,N,Fc] (NULL iff Fc == 0), bounds DEVICE [B,6] = (xmin, ymin, zmin, xmax, ymax, zmax) per item,
 *   read by the kernels; grid [B,C,V,V,V] (channels_first != 0) or [B,V,V,V,C], 16-byte aligned, every float written once.
 * _images: the same cloud read in place from n_images <= MGS_VOXELIZE_MAX_SOURCES pairs of contiguous images, coords[i]
 * [B,3,H,W] and features[i] [B,Fc,H,W] (HOST arrays of device pointers, HW = H W): point i HW + row W + col of an item is that
 * pixel of image i -- the order of flattening camera after camera, row-major -- and N = n_images HW.
 * Limits (MGS_ERR_INVALID_ARG before any launch): 1 <= B <= 65536; 0 <= N <= 2^24 (a float count is exact up to there); V >= 1;
 * B V^3 < 2^31 and B N < 2^31; 0 <= Fc <= MGS_VOXELIZE_MAX_FEATURES; non-NULL pointers; grid and workspace 16-byte aligned.
 * MGS_ERR_WORKSPACE: fewer than mgs_voxelize_workspace_bytes(B, N, V) bytes (0 for sizes outside the limits; a function of
 * B, N, V only).  The call zeroes what it needs of the workspace itself.  N = 0 writes the background grid.
 * Four launches on `stream` (clear, link, mean, write), no host read, no allocation: capturable into a HIP graph. */
#define MGS_VOXELIZE_MAX_FEATURES 64
#define MGS_VOXELIZE_MAX_SOURCES 8
size_t mgs_voxelize_workspace_bytes(int B, int64_t N, int V);
int mgs_voxelize_forward(int B, int64_t N, int V, int Fc, int channels_first, const float* coords, const float* features,
                         const float* bounds, float* grid, void* workspace, size_t workspace_bytes, mgs_stream_t stream);
int mgs_voxelize_forward_images(int B, int n_images, int64_t HW, int V, int Fc, int channels_first, const float* const* coords,
                                const float* const* features, const float* bounds, float* grid, void* workspace,
                                size_t workspace_bytes, mgs_stream_t stream);

/* ---- the Perceiver's attention, fused, fp32 (MG/agents/manigaussian_bc/perceiver_lang_io.py:102-145, class Attention) ----
 *   out[b, i, h D + .] = sum_j drop(softmax_j(q_i . k_j * D^-0.5, masked keys at -FLT_MAX))_ij v_j     D = 64 only
 * q [B,Nq,H D]; k and v rows of H D floats each, read where they lie (the two halves of a to_kv output [B,Nk,2 H D]: row stride
 * 2 H D, v = k + H D); head h is columns [h D, h D + D) of a row.  Strides are in ELEMENTS: *_stride_b between batch items,
 * *_stride_n between rows; the last dimension is unit-stride.  mask: bytes [B,Nk] (row stride mask_stride_b), 0 = the key's
 * score is -FLT_MAX (masked_fill_(~mask, -finfo.max): a row whose keys are all masked attends uniformly), or NULL.
 * Dropout on the probabilities after normalisation: element (b H + h, i, j) is kept iff word (j & 3) of
 *   Philox4x32-10(counter = (j >> 2, i, b H + h, offset & 0xffffffff), key = (seed & 0xffffffff, (seed >> 32) ^ (offset >> 32)))
 * is >= floor(dropout_p * 2^32), and kept elements are scaled by 1 / (1 - dropout_p).  rng_state: DEVICE {seed, offset}, two
 * 64-bit words read by the kernels (a captured graph follows in-place updates); may be NULL when dropout_p == 0.
 * forward: writes out (strides out_stride_*) and lse [B,H,Nq] = row maximum + log of the row sum of the undropped row.
 * backward: out, lse of the forward, d_out (strides dout_stride_*) -> dq [B,Nq,H D] (dq_stride_*) and dkv: dk in columns
 * [0, H D), dv in [H D, 2 H D) of rows of dkv_stride_n >= 2 H D floats.  workspace: the workspace-size query below (D_i).
 * dropout_mask: the keep decisions of forward and backward as bytes [B H, Nq, Nk] (a test and debug aid).
 * MGS_ERR_INVALID_ARG before any launch: D != 64; B, H, Nq or Nk < 1; B H > 65535; dropout_p outside [0, 1); a pointer the
 * kernels read or write 16 bytes at a time (q, k, v, out, d_out, dq, dkv, workspace) not 16-byte aligned; a row stride below
 * the row or a stride that is no multiple of 4.  B H Nq Nk is no limit: nothing of that size exists.
 * No atomics: bit-identical from run to run.  No host read, no allocation, no state: capturable into a HIP graph. */
typedef struct MgsAttentionArgs {
  int32_t B, H, Nq, Nk, D;
  float dropout_p;
  const float* q;
  const float* k;
  const float* v;
  const uint8_t* mask;
  const uint64_t* rng_state;
  int64_t q_stride_b, q_stride_n, k_stride_b, k_stride_n, v_stride_b, v_stride_n;
  int64_t out_stride_b, out_stride_n, dout_stride_b, dout_stride_n;
  int64_t dq_stride_b, dq_stride_n, dkv_stride_b, dkv_stride_n;
  int64_t mask_stride_b;
} MgsAttentionArgs;
size_t mgs_attention_workspace_bytes(int B, int H, int Nq, int Nk);
int mgs_attention_forward(const MgsAttentionArgs* a, float* out, float* lse, mgs_stream_t stream);
int mgs_attention_backward(const MgsAttentionArgs* a, const float* out, const float* lse, const float* d_out, float* dq,
                           float* dkv, void* workspace, size_t workspace_bytes, mgs_stream_t stream);
int mgs_attention_dropout_mask(const MgsAttentionArgs* a, uint8_t* keep, mgs_stream_t stream);

/* ---- the agent's SE(3) augmentation without a host read (MG/voxel/augmentation.py:11-377, apply_se3_augmentation and
 * apply_se3_augmentation_with_camera_pose: the rejection loop, its discretisation and the transform of clouds and camera
 * poses) -- additive exports, the ABI version stays 16 ----
 * select, ONE launch of ONE workgroup: for every (attempt a < attempts, sample b < B)
 *   draw     trans_u in [-1, 1)^3 and integer steps in [-rot_steps[i], rot_steps[i]] (0 where rot_steps[i] == 0): row (a, b)
 *            of `draws` [attempts,B,6] fp32 (trans_u, then roll, pitch, yaw steps as floats) when draws != NULL, else words of
 *            Philox4x32-10(counter = (g, a, b, offset & 0xffffffff), key as for the attention dropout), g = 0: three words
 *            -> (word >> 8) 2^-23 - 1 and one -> roll, g = 1: pitch, yaw; a step is ((word (2 k + 1)) >> 32) - k.
 *            rng_state: DEVICE {seed, offset}, read by the kernel.  mgs_se3_draws writes exactly that table.
 *   compose  fp32, as torch runs the reference: G = matrix of the xyzw quaternion gripper_pose[b, 3:7] (divided by its squared
 *            norm), S = Rx(roll) Ry(pitch) Rz(yaw), angle = float(step) * rot_step_rad, perturbed rotation G S; translation
 *            t + (max - min of the bounds row) * trans_aug_range * trans_u -- the product and the sum in fp64 rounded once to
 *            fp32 when trans_f64 != 0 (what type promotion does with the agent's float64 range tensor), else fp32 steps.
 *   discretise  fp64 on those fp32 results, as numpy and scipy do: voxel index min(floor(float(p - min) / ((max - min) /
 *            (V + 1e-12) + 1e-12)), V - 1) against bounds row (layer > 0 ? b : 0) -- negative, hence INVALID, only below the
 *            bounds; above them it is clamped and valid --; rotation -> quaternion (rounded to fp32, normalised, w >= 0) ->
 *            extrinsic xyz Euler degrees + 180, / rot_resolution, rounded half to even, rot_bins -> 0; the gripper entry is
 *            action_rot_grip[b, 3].
 *   retry    0 ("batch", the reference): the first attempt in which EVERY sample is valid is taken for all of them; none:
 *            every sample is the identity.  1 ("sample"): every sample takes its own first valid attempt, or the identity.
 * -> out_trans int64 [B,3], out_rot_grip int64 [B,4] (the inputs' values for an identity sample), info int32 [1 + B]: the
 *    first attempt valid for the whole batch, then the attempt each sample took (-1: none / identity), and in the workspace
 *    one record per sample: rotation S, pivot = gripper translation, target = clamp(pivot + fp32 shift, min over ALL rows of
 *    bounds[:, :3], max over all rows of bounds[:, 3:]).  bounds: DEVICE [bounds_rows,6], bounds_rows 1 or B.
 *    action_trans [B,3] and action_rot_grip [B,4]: int64 when action_i64 != 0, else int32.
 * apply, ONE launch for all sources: every point p of src[i] -- planar [B,3,n_points[i]], element strides stride_b[i] between
 *   samples and stride_c[i] between the three planes, points unit-stride -- becomes S^T (p - pivot) + target in dst[i],
 *   contiguous planar; every pose pose_in[i] [B,4,4] becomes (S^T R, S^T (T - pivot) + target, bottom row copied) in pose_out[i].
 *   An identity sample's points and poses are copied bit for bit.  No in-place use: dst and pose_out are other memory.
 * MGS_ERR_INVALID_ARG before any launch: B outside 1 .. MGS_SE3_MAX_BATCH, attempts outside 1 .. MGS_SE3_MAX_ATTEMPTS,
 * voxel_size < 1, bounds_rows neither 1 nor B, a negative rot_steps, retry not 0 or 1, n_sources or n_poses outside
 * 0 .. MGS_SE3_MAX_SOURCES, n_points outside 1 .. 2^24, a NULL pointer, neither draws nor rng_state.
 * MGS_ERR_WORKSPACE: fewer bytes than the workspace-size query names (0 for a B outside the limits).
 * All results are written with ordinary vector stores; no atomics on memory: the same from run to run.  No host read, no
 * allocation, no state: both calls are capturable into a HIP graph, and a replay follows in-place updates of rng_state. */
#define MGS_SE3_MAX_SOURCES 8
#define MGS_SE3_MAX_BATCH 4096
#define MGS_SE3_MAX_ATTEMPTS 32
typedef struct MgsSe3Args {
  int32_t B, attempts, retry, layer, voxel_size, bounds_rows, rot_bins, trans_f64, action_i64;
  int32_t rot_steps[3];
  float rot_step_rad;
  int32_t n_sources, n_poses, pad_;
  double rot_resolution;
  double trans_aug_range[3];
  const float* gripper_pose; /* [B,7] contiguous: translation, quaternion xyzw */
  const void* action_trans;
  const void* action_rot_grip;
  const float* bounds;
  const uint64_t* rng_state;
  const float* draws;
  const float* src[MGS_SE3_MAX_SOURCES];
  float* dst[MGS_SE3_MAX_SOURCES];
  int64_t n_points[MGS_SE3_MAX_SOURCES], stride_b[MGS_SE3_MAX_SOURCES], stride_c[MGS_SE3_MAX_SOURCES];
  const float* pose_in[MGS_SE3_MAX_SOURCES];
  float* pose_out[MGS_SE3_MAX_SOURCES];
} MgsSe3Args;
size_t mgs_se3_workspace_bytes(int B);
int mgs_se3_select(const MgsSe3Args* a, int64_t* out_trans, int64_t* out_rot_grip, int32_t* info, void* workspace,
                   size_t workspace_bytes, mgs_stream_t stream);
int mgs_se3_apply(const MgsSe3Args* a, const void* workspace, size_t workspace_bytes, mgs_stream_t stream);
int mgs_se3_draws(const MgsSe3Args* a, float* draws, mgs_stream_t stream);

/* ---- the Perceiver's aggregated features, fused, fp32 (MG/helpers/network_utils.py:927-963, class SpatialSoftmax3D, and the
 * nn.AdaptiveMaxPool3d(1) next to it at MG/agents/manigaussian_bc/perceiver_lang_io.py:384,485,504) -- ABI v12 ----
 * feature [rows, N], N = D H W, contiguous, 16-byte aligned; a row is one (batch, channel), rows = B C, row = b C + c.
 *   p = softmax(row / temperature);   keypoints[b, 3 c + (0, 1, 2)] = (sum p pos_x, sum p pos_y, sum p pos_z);   maxpool[b, c] = max(row)
 * The positions are the reference's tables, np.meshgrid(linspace(-1, 1, D), linspace(-1, 1, H), linspace(-1, 1, W)) in its default
 * 'xy' order flattened: for the flat index i = (a D + b) W + c (a < H, b < D, c < W), pos_x = lin_D[b], pos_y = lin_H[a],
 * pos_z = lin_W[c], lin_n = linspace(-1, 1, n) ([-1] for n = 1).  For D != H they do not follow the volume's axes; that is the
 * reference's behaviour.  The kernels compute them from the index; no table of N entries is read.
 * forward: ONE read of feature.  Each row is cut into slices (slices = 0: chosen from rows and N; 1..64: forced, a test aid) of
 * whole 16-byte vectors; a row that starts off a 16-byte boundary (N % 4 != 0) has its first and last elements read as scalars.
 * A launch of rows x slices workgroups writes one 32-byte record per slice to the workspace; a second, small launch folds each
 * row's records IN SLICE ORDER and writes keypoints (row stride keypoints_stride_b >= 3 C floats), maxpool (row stride
 * maxpool_stride_b >= C; may be NULL) and stats [rows, 6] = (max, sum exp((x - max) / temperature), E_x, E_y, E_z, argmax as the
 * bits of a uint32): all the backward needs.  argmax is the LOWEST flat index holding the maximum, for every split.
 * backward: one launch, one read of feature and one write of g_feature [rows, N] (16-byte aligned, every float written once):
 *   g_feature_i = p_i / temperature * sum_axis g_keypoints_axis (pos_axis(i) - E_axis) + g_max [i == argmax]
 * g_keypoints [B, 3 C] and g_max [B, C] by row stride; either may be NULL (no such upstream gradient).
 * MGS_ERR_INVALID_ARG before any launch: rows, C, D, H or W < 1; rows no multiple of C; D H W > 2^31 - 1; rows > (2^31 - 1) / 64;
 * temperature not positive and finite; slices outside [0, 64]; a NULL pointer other than the optional ones; feature, g_feature or
 * the workspace not 16-byte aligned; a row stride below its row.  MGS_ERR_WORKSPACE: fewer than
 * mgs_spatial_softmax_workspace_bytes(rows, N) bytes (64 records per row: independent of the split; 0 for sizes outside the limits).
 * A row that holds a non-finite value yields unspecified values for that row only.  Element offsets are 64-bit.
 * No atomics, no workgroup waits for another, nothing to zero: bit-identical from run to run.  No host read, no allocation, no
 * state: capturable into a HIP graph. */
size_t mgs_spatial_softmax_workspace_bytes(int64_t rows, int64_t N);
int mgs_spatial_softmax_forward(int64_t rows, int C, int D, int H, int W, float temperature, const float* feature,
                                float* keypoints, int64_t keypoints_stride_b, float* maxpool, int64_t maxpool_stride_b,
                                float* stats, void* workspace, size_t workspace_bytes, int slices, mgs_stream_t stream);
int mgs_spatial_softmax_backward(int64_t rows, int C, int D, int H, int W, float temperature, const float* feature,
                                 const float* stats, const float* g_keypoints, int64_t g_keypoints_stride_b, const float* g_max,
                                 int64_t g_max_stride_b, float* g_feature, int slices, mgs_stream_t stream);

/* ---- the Perceiver decoder's volume plumbing between its convolutions, fused, fp32 (MG/agents/manigaussian_bc/
 * perceiver_lang_io.py:488-499; MG/helpers/network_utils.py:129-171 Conv3DBlock, 374-391 Conv3DUpsampleBlock) -- ABI v13 ----
 *   out = replicate_pad(trilinear_upsample(cat(sources, 1), scale, align_corners = False), pad)
 * sources: nsrc tensors [B, C_k, D, H, W] whose spatial dimensions are contiguous: element (b, c, z, y, x) of source k lies at
 * src[k][b stride_b[k] + c stride_c[k] + (z H + y) W + x] (strides in floats, any value: a channel slice of a wider tensor is read
 * in place).  out [B, sum C_k, s D + 2 p, s H + 2 p, s W + 2 p], contiguous.  Per axis of source length n, for the padded index op:
 *   o = clamp(op - p, 0, s n - 1);  src = max((o + 0.5) / s - 0.5, 0);  i0 = floor(src);  lambda = src - i0;  i1 = min(i0 + 1, n - 1)
 * weights 1 - lambda on i0 and lambda on i1, 1 / s and lambda in fp32 (torch's arithmetic); the 3-D weight is the product of the
 * axes'.  scale == 1 is a copy, bit for bit.
 * forward: one launch; every element of out is written exactly once, 16 bytes at a time.
 * backward: g_out [as out], contiguous -> g_src[k] [B, C_k, D, H, W], contiguous, one per source.  A gather: each gradient element
 * is written once, from the padded outputs that reach it summed in ascending index order; nothing is zero-filled.  scale > 1: two
 * launches (x and y per padded z-plane into the workspace [B sum C_k, s D + 2 p, H, W], then z); scale == 1: one launch, g_out
 * read about once.  workspace: at least the workspace-size query's bytes (positive for every valid shape; 0: invalid shape).
 * MGS_ERR_INVALID_ARG before any launch: scale outside 1..8; pad outside 0..8; nsrc outside 1..4; a C_k < 1; B < 0; D, H or W < 1;
 * the padded output (hence any source) above 2^31 - 1 elements; a NULL pointer (the arguments, a used src[k], out, g_out, g_src,
 * a used g_src[k], the workspace); out, a g_src[k] or the workspace not 16-byte aligned, a src[k] or g_out not 4-byte aligned; a
 * workspace below the query's size.  B == 0: MGS_OK, nothing is launched.  Indices inside a tensor are 32-bit, a source's batch
 * and channel offsets 64-bit.  Bit-identical from run to run.  No host read, no allocation, no state: capturable into a HIP graph. */
#define MGS_VOLUME_MAX_SOURCES 4
#define MGS_VOLUME_MAX_SCALE 8
#define MGS_VOLUME_MAX_PAD 8
typedef struct MgsVolumeArgs {
  int32_t B, D, H, W;      /* batch and the sources' common spatial shape */
  int32_t scale, pad, nsrc;
  int32_t C[MGS_VOLUME_MAX_SOURCES];
  const float* src[MGS_VOLUME_MAX_SOURCES];   /* forward only */
  int64_t stride_b[MGS_VOLUME_MAX_SOURCES], stride_c[MGS_VOLUME_MAX_SOURCES];
} MgsVolumeArgs;
size_t mgs_volume_workspace_bytes(const MgsVolumeArgs* a);
int mgs_volume_resample_pad_forward(const MgsVolumeArgs* a, float* out, mgs_stream_t stream);
int mgs_volume_resample_pad_backward(const MgsVolumeArgs* a, const float* g_out, float* const* g_src, void* workspace,
                                     size_t workspace_bytes, mgs_stream_t stream);

/* ---- the rest of a Perceiver transformer block beside the attention and the GEMMs, fused, fp32 (MG/agents/manigaussian_bc/
 * perceiver_lang_io.py:56-99: PreNorm's nn.LayerNorm; FeedForward's Linear -> GEGLU -> Linear) -- ABI v14 ----
 * layernorm, rows of D floats (1 <= D <= 1024), x read by row stride x_stride >= D (floats):
 *   mean = sum x / D;  rstd = 1 / sqrt(sum (x - mean)^2 / D + eps)  (the variance from the centred values, never E[x^2] - E[x]^2);
 *   y = (x - mean) rstd weight + bias, y [rows, D] contiguous;  stats [rows, 2] = (mean, rstd): all the backward keeps beside x.
 *   One wave holds a row in registers; one launch.
 * layernorm backward, xhat = (x - mean) rstd, g [rows, D] read by row stride g_stride (0: one row for all rows, else >= D):
 *   dx = rstd (g w - mean(g w) - xhat mean(g w xhat)), dx [rows, D] contiguous;   dweight = sum_rows g xhat;   dbias = sum_rows g.
 *   Two launches: the row kernel writes dx and, per SLAB of consecutive rows, the slab's two column sums to the workspace
 *   [slabs][2][D]; the column kernel adds the slabs in ascending order.  dweight == NULL and dbias == NULL (frozen parameters):
 *   no partial sums, no second launch, no workspace needed; one of them NULL: that sum is not written.
 * bias-GEGLU, h [rows, 2 M] read by row stride h_stride >= 2 M (the first linear's product WITHOUT its bias), bias [2 M] or NULL:
 *   out[r, j] = (h[r, j] + bias[j]) gelu(h[r, M + j] + bias[M + j]),  gelu(t) = t (1 + erf(t / sqrt 2)) / 2,  out [rows, M] contiguous.
 * bias-GEGLU backward, g [rows, M] by row stride g_stride (0, or >= M); a and gate recomputed from h and bias:
 *   dh[:, :M] = g gelu(gate);   dh[:, M:] = g a gelu'(gate),  gelu'(t) = Phi(t) + t phi(t)  (1 and 0 in the tails, never NaN);
 *   dh [rows, 2 M] contiguous, both halves written in place;   dbias [2 M] = sum_rows dh by the same slab scheme, or NULL: no
 *   partial sums, no second launch, no workspace.
 * row_split: the number of slabs, 0: the library's choice, 1..64: forced (a test aid; fewer when there are fewer rows).  dx and dh
 * do not depend on it.  workspace: 16-byte aligned, at least the size query's bytes for (rows, cols), cols = D for the layernorm and
 * M for the GEGLU (64 slabs: independent of the split; 0: rows or cols < 1).
 * Every tensor is read as 16-byte aligned vectors whatever its own alignment and written as 16-byte vectors where the address
 * allows; inputs need 4-byte alignment only.  MGS_ERR_INVALID_ARG before any launch: D outside 1..1024; rows or M < 1; rows D or
 * rows 2 M above 2^31 - 1; a row stride below its row; row_split outside 0..64; a NULL pointer other than the optional ones; y, dx,
 * out, dh or a needed workspace not 16-byte aligned.  MGS_ERR_WORKSPACE: a needed workspace below the query's size.
 * No atomics; every output element is written once from a sum whose terms and order depend on the indices and the split alone:
 * bit-identical from run to run.  No host read, no allocation, no state: capturable into a HIP graph. */
size_t mgs_feedforward_workspace_bytes(int64_t rows, int64_t cols);
int mgs_layernorm_forward(int64_t rows, int D, const float* x, int64_t x_stride, const float* weight, const float* bias, float eps,
                          float* y, float* stats, mgs_stream_t stream);
int mgs_layernorm_backward(int64_t rows, int D, const float* x, int64_t x_stride, const float* weight, const float* stats,
                           const float* g, int64_t g_stride, float* dx, float* dweight, float* dbias, void* workspace,
                           size_t workspace_bytes, int row_split, mgs_stream_t stream);
int mgs_bias_geglu_forward(int64_t rows, int64_t M, const float* h, int64_t h_stride, const float* bias, float* out,
                           mgs_stream_t stream);
int mgs_bias_geglu_backward(int64_t rows, int64_t M, const float* h, int64_t h_stride, const float* bias, const float* g,
                            int64_t g_stride, float* dh, float* dbias, void* workspace, size_t workspace_bytes, int row_split,
                            mgs_stream_t stream);

/* ---- the voxel encoder stem's normalisation sites, fused, fp32 (MG/helpers/network_utils.py:219-231, class InPlaceABN:
 * nn.BatchNorm3d then an in-place nn.LeakyReLU; :297-303, the skip adds behind three of them) -- additive exports, ABI v17 ----
 * x, residual (or NULL), y, g_y, dx: [B, C, N] contiguous, 16-byte aligned, N = D H W; a row is one (batch, channel).
 *   z = (x - mean_c) invstd_c weight_c + bias_c;   y = residual + (z > 0 ? z : negative_slope z)      (negative_slope 0: ReLU)
 * training != 0: mean_c and the BIASED variance var_c over the channel's B N values, invstd_c = 1 / sqrt(var_c + eps);
 *   running_mean_c = (1 - momentum) running_mean_c + momentum mean_c, running_var_c likewise with the UNBIASED variance
 *   var_c B N / (B N - 1), both in place (both NULL: not tracked); *num_batches_tracked (int64, or NULL) += 1 by the same launch;
 *   stats [C, 2] = (mean_c, invstd_c): all the backward keeps beside x.  Two launches.  A row is cut into nsub sub-slices of whole
 *   16-byte vectors, nsub a function of N alone (1..64); the first launch reduces every sub-slice to a (count, mean, M2) record in
 *   the workspace (Chan's merge from register tiles up; never sum x^2 - (sum x)^2), the second merges a channel's B nsub records in a
 *   fixed order, in double, and writes y.  slices (0: chosen from B C and N; 1..64: forced, a test aid; never more than nsub) is
 *   the number of workgroups that share a row's sub-slices: no result depends on it, bit for bit.
 * training == 0: mean_c = running_mean_c, var_c = running_var_c; one launch, nothing is updated; stats and workspace are unused.
 * backward (of a training forward): dz = g_y (z > 0 ? 1 : negative_slope), z recomputed from x and stats by the forward's own
 *   expression (z == 0 takes the slope, as torch does);  xhat = (x - mean_c) invstd_c;
 *   dbias_c = sum dz;  dweight_c = sum dz xhat;  dx = weight_c invstd_c (dz - dbias_c / (B N) - xhat dweight_c / (B N)).
 *   Two launches: per sub-slice records of the two sums, then dx (and dweight, dbias: either may be NULL) from their merge, in the
 *   same fixed order.  The gradient towards residual is g_y itself.
 * workspace: 16-byte aligned, at least mgs_abn_workspace_bytes(B, C, N) bytes (64 records per row: independent of N and of the
 * split; 0 for sizes outside the limits).
 * MGS_ERR_INVALID_ARG before any launch: C outside 1..65536; B or N < 1; N > 2^31 - 1; B C > (2^31 - 1) / 64; negative_slope, eps or
 * momentum not finite, eps < 0; slices outside [0, 64]; B N < 2 in training mode ("Expected more than 1 value per channel when
 * training"); a NULL pointer other than the optional ones (running buffers must be both or neither, and are needed in eval mode); a
 * volume or the workspace not 16-byte aligned.  MGS_ERR_WORKSPACE: fewer bytes than the query's.  Element offsets are 64-bit.
 * No atomics, no workgroup waits for another, nothing to zero: bit-identical from run to run.  No host read, no allocation, no
 * state: capturable into a HIP graph (every replay updates the running buffers and the counter once). */
size_t mgs_abn_workspace_bytes(int64_t B, int C, int64_t N);
int mgs_abn_forward(int64_t B, int C, int64_t N, const float* x, const float* residual, const float* weight, const float* bias,
                    float* running_mean, float* running_var, int64_t* num_batches_tracked, int training, float momentum, float eps,
                    float negative_slope, float* y, float* stats, void* workspace, size_t workspace_bytes, int slices,
                    mgs_stream_t stream);
int mgs_abn_backward(int64_t B, int C, int64_t N, const float* x, const float* g_y, const float* weight, const float* bias,
                     const float* stats, float negative_slope, float* dx, float* dweight, float* dbias, void* workspace,
                     size_t workspace_bytes, int slices, mgs_stream_t stream);

/* ---- the voxel encoder stem's 3x3x3 convolutions, direct, fp32 (MG/helpers/network_utils.py:234-306: the bias-free nn.Conv3d of
 * ConvBnReLU3D and the nn.ConvTranspose3d(stride 2) of the three up sites) -- additive exports, ABI v17 ----
 * Kernel 3x3x3, padding 1, dilation 1, groups 1, no bias; the three spatial strides are equal, stride = 1 or 2; Cin, Cout = 1..64.
 * x [B, Cin, D, H, W], y and g_y [B, Cout, OD, OH, OW] with O = (I - 1) / stride + 1 per dimension (integer division), dx like x,
 * w and dw [Cout, Cin, 3, 3, 3] (nn.Conv3d's layout): all contiguous and 16-byte aligned.  D, H, W are ALWAYS the extents of the
 * convolution's input side (x, dx); the output side's are derived from them, so the two cannot disagree.
 *   forward:          y[b,co,o]     = sum_ci sum_tap w[co,ci,tap] x[b,ci,o stride + tap - 1]      (taps outside the volume read 0)
 *   backward_data:    dx[b,ci,i]    = sum_co sum_{(o,tap): o stride + tap - 1 = i} w[co,ci,tap] g_y[b,co,o]
 *   backward_weight:  dw[co,ci,tap] = sum_b sum_o g_y[b,co,o] x[b,ci,o stride + tap - 1]
 * All three gather: every output element is written once, by one thread; backward_data at stride 2 works per 2x2x2 block of dx (1, 2,
 * 4 or 8 taps per voxel by parity class), not as a scatter.  backward_weight is two launches: the forward's output tiles, in their
 * linear order, are cut into at most 64 runs whose number and length depend on the shape alone; every run is summed to one RECORD
 * [Cout, Cin, 27] in the workspace, and the second launch adds the records in ascending order, in double.  split (0: chosen from the
 * shape; 1..64: forced, a test aid; never more than the number of runs) is the number of workgroups that share the runs of one
 * (4 output channels, input channel) pair: it says which workgroup computes a record, never what the record is -- dw is the same
 * bits for every split.
 * nn.ConvTranspose3d(Cin_T, Cout_T, 3, stride 2, padding 1, output_padding 0 or 1) needs no entry point of its own: its weight
 * [Cin_T, Cout_T, 27] IS a convolution weight [Cout, Cin, 27] with Cout = Cin_T, Cin = Cout_T; its forward is backward_data with D H W
 * = its output extents 2 I_T - 1 + output_padding, its input gradient is forward, its weight gradient is backward_weight with x = the
 * gradient of its output and g_y = its input.
 * workspace: 16-byte aligned, at least as many bytes as the size query returns for the same shape (0 for sizes outside the limits).
 * MGS_ERR_INVALID_ARG before any launch: Cin or Cout outside 1..64; stride other than 1 or 2; B or an extent below 1; D H W >= 2^31
 * (elements per (batch, channel) row), or B times the number of tiles above 2^31 - 1; a NULL pointer; a pointer not 16-byte aligned;
 * split outside [0, 64].  MGS_ERR_WORKSPACE: fewer bytes than the query's.  Element offsets are 64-bit.
 * No atomics, no workgroup waits for another, nothing to zero: bit-identical from run to run.  No host read, no allocation, no
 * state: capturable into a HIP graph. */
size_t mgs_conv3d_workspace_bytes(int64_t B, int Cin, int Cout, int64_t D, int64_t H, int64_t W, int stride);
int mgs_conv3d_forward(int64_t B, int Cin, int Cout, int64_t D, int64_t H, int64_t W, int stride, const float* x, const float* w,
                       float* y, mgs_stream_t stream);
int mgs_conv3d_backward_data(int64_t B, int Cin, int Cout, int64_t D, int64_t H, int64_t W, int stride, const float* g_y,
                             const float* w, float* dx, mgs_stream_t stream);
int mgs_conv3d_backward_weight(int64_t B, int Cin, int Cout, int64_t D, int64_t H, int64_t W, int stride, const float* x,
                               const float* g_y, float* dw, void* workspace, size_t workspace_bytes, int split, mgs_stream_t stream);

/* ---- the voxel encoder stem's pointwise (1x1x1) convolution with bias (helpers/network_utils.py:248-306, conv_out =
 * nn.Conv3d(8, 64, 1, bias=True)) -- additive exports, ABI v17 ----
 * Kernel 1x1x1, stride 1, no padding, groups 1; Cin, Cout = 1..64; n = D H W, the voxels of a (batch, channel) row.
 * x and dx [B, Cin, n], y and g_y [B, Cout, n], w and dw [Cout, Cin] (nn.Conv3d's [Cout, Cin, 1, 1, 1]), bias and db [Cout]: all
 * contiguous and 16-byte aligned.
 *   forward:   y[b,co,v]  = bias[co] + sum_ci w[co,ci] x[b,ci,v]                      (bias may be NULL: no bias)
 *   backward:  dx[b,ci,v] = sum_co w[co,ci] g_y[b,co,v];  dw[co,ci] = sum_{b,v} g_y[b,co,v] x[b,ci,v];  db[co] = sum_{b,v} g_y[b,co,v]
 * Every output element is written once, by one thread; every sum's order depends on the shape alone.  The forward is one launch;
 * where n is a multiple of 4 its accesses are 16 bytes wide.  dx, dw and db may each be NULL and only what is asked for is computed:
 * dx alone is one launch without a workspace (x may then be NULL); with dw or db the voxel tiles, in their linear order over (batch,
 * voxel), are cut into at most 64 runs whose number and length depend on the shape alone, every run is summed to one RECORD
 * [Cout, Cin + 1] in the workspace by a launch that reads g_y once for dx, dw and db together when Cin <= 16 (once per 16 input channels
 * above), and a second launch adds the records in ascending order, in double.  split (0: chosen from the shape; 1..64: forced, a test
 * aid; never more than the number of runs) is the number of workgroups that share the runs: it says which workgroup computes a
 * record, never what the record is -- dw and db are the same bits for every split.
 * workspace: 16-byte aligned, at least as many bytes as the size query returns for the same shape (0 for sizes outside the limits,
 * else a multiple of 256).
 * MGS_ERR_INVALID_ARG before any launch: Cin or Cout outside 1..64; B or n below 1; n >= 2^31, or B times the number of tiles above
 * 2^31 - 1; a NULL pointer where one is required (dx, dw and db all NULL included); a pointer not 16-byte aligned; split outside
 * [0, 64].  MGS_ERR_WORKSPACE: fewer bytes than the query's.  Element offsets are 64-bit.
 * No atomics, no workgroup waits for another, nothing to zero: bit-identical from run to run.  No host read, no allocation, no
 * state: capturable into a HIP graph. */
size_t mgs_pointwise_workspace_bytes(int64_t B, int Cin, int Cout, int64_t n);
int mgs_pointwise_forward(int64_t B, int Cin, int Cout, int64_t n, const float* x, const float* w, const float* bias, float* y,
                          mgs_stream_t stream);
int mgs_pointwise_backward(int64_t B, int Cin, int Cout, int64_t n, const float* x, const float* g_y, const float* w, float* dx,
                           float* dw, float* db, void* workspace, size_t workspace_bytes, int split, mgs_stream_t stream);

/* ---- the same pointwise convolution for 65..256 output channels (conv_out at final_dim = 128: nn.Conv3d(8, 128, 1, bias=True),
 * conf/method/ManiGaussian_BC.yaml:35) -- additive exports, ABI v17 ----
 * Kernel 1x1x1, stride 1, no padding, groups 1; Cin = 1..16 (what the fused backward holds per lane, so that g_y is read once),
 * Cout = 65..256 (below 65 mgs_pointwise_* is the op); n = D H W.  Parameters, layouts, alignment, formulas and error codes are those
 * of mgs_pointwise_* above.
 * The forward and the input gradient alone are mgs_pointwise_*'s own kernels, one launch each.  With dw or db a workgroup walks its
 * run of tiles once per BLOCK of 64 output channels, in ascending order: in block c wave k owns channels 64 c + 8 k .. + 7 and
 * writes those rows of the run's one RECORD [Cout, Cin + 1]; g_y is read once, x once per block; where dx is asked for it is written
 * once per block, and in a block after the first every element's sum starts from what the same thread stored for it in the block
 * before.  That makes dx one chain over the groups of 8 output channels in ascending order, the order of the launch that computes dx
 * alone: dx is the same bits whether or not dw and db are asked for.  Records, merge launch and split as above: dw and db are the
 * same bits for every split.
 * workspace: 16-byte aligned, at least as many bytes as the size query returns for the same shape (0 for sizes outside the limits,
 * else a multiple of 256).
 * MGS_ERR_INVALID_ARG before any launch: Cin outside 1..16; Cout outside 65..256; B or n below 1; n >= 2^31, or B times the number
 * of tiles above 2^31 - 1; a NULL pointer where one is required (dx, dw and db all NULL included); a pointer not 16-byte aligned;
 * split outside [0, 64].  MGS_ERR_WORKSPACE: fewer bytes than the query's.  Element offsets are 64-bit.
 * No atomics, no workgroup waits for another, nothing to zero: bit-identical from run to run.  No host read, no allocation, no
 * state: capturable into a HIP graph. */
size_t mgs_pointwise_wide_workspace_bytes(int64_t B, int Cin, int Cout, int64_t n);
int mgs_pointwise_wide_forward(int64_t B, int Cin, int Cout, int64_t n, const float* x, const float* w, const float* bias, float* y,
                               mgs_stream_t stream);
int mgs_pointwise_wide_backward(int64_t B, int Cin, int Cout, int64_t n, const float* x, const float* g_y, const float* w, float* dx,
                                float* dw, float* db, void* workspace, size_t workspace_bytes, int split, mgs_stream_t stream);

/* ---- the Perceiver decoder's narrow-output 3x3x3 convolution with its pad folded into the addressing (SURVEY.md 2:
 * agents/manigaussian_bc/perceiver_lang_io.py:322, trans_decoder = nn.Conv3d(128, 1, 3, padding=1, padding_mode='replicate') with
 * bias) -- additive exports, ABI v17 ----
 * Kernel 3x3x3, stride 1, padding 1, dilation 1, groups 1; Cin = 1..256, Cout = 1..4; zeros_pad = 0: replicate padding, 1: zeros.
 * x and dx [B, Cin, D, H, W], y and g_y [B, Cout, D, H, W], w and dw [Cout, Cin, 3, 3, 3] (nn.Conv3d's layout), bias and db [Cout]:
 * all contiguous and 16-byte aligned.  With c(i) = clamp(i, 0, n - 1) per dimension in replicate mode (in zeros mode a tap outside
 * the volume contributes nothing):
 *   forward:   y[b,co,o]     = bias[co] + sum_ci sum_tap w[co,ci,tap] x[b,ci,c(o + tap - 1)]             (bias may be NULL: no bias)
 *   backward:  dx[b,ci,i]    = sum_co sum_{(o,tap): c(o + tap - 1) = i} w[co,ci,tap] g_y[b,co,o]
 *              dw[co,ci,tap] = sum_b sum_o g_y[b,co,o] x[b,ci,c(o + tap - 1)];   db[co] = sum_b sum_o g_y[b,co,o]
 * The padded volume is never written.  All passes gather: every output element is written once, by one thread, from a sum whose terms
 * and order depend on the shape alone; in replicate mode a border voxel of dx collects what its replicated copies received (up to 8
 * padded positions at a corner, 27 when D = H = W = 1).  The forward is one launch.  dx, dw and db may each be NULL and only what is
 * asked for is computed: dx is one launch that reads g_y and w only (no workspace; x may be NULL when dw is NULL); dw and db are two
 * launches: the tiles of 32 x 8 x 8 voxels (W x H x D), in their linear order, are cut into at most 64 runs whose number and length
 * depend on the shape alone, every run is summed to one RECORD [Cout, 27 Cin + 1] in the workspace, and the second launch adds the
 * records in ascending order, in double.  split (0: chosen from the shape; 1..64: forced, a test aid; never more than the number of
 * runs) is the number of workgroups that share the runs: it says which workgroup computes a record, never what the record is -- dw
 * and db are the same bits for every split.
 * workspace: 16-byte aligned, at least as many bytes as the size query returns for the same shape (0 for sizes outside the limits,
 * else a multiple of 256); needed only when dw or db is asked for.
 * MGS_ERR_INVALID_ARG before any launch: Cin outside 1..256; Cout outside 1..4; B or an extent below 1; D H W >= 2^31 (elements per
 * (batch, channel) row), or B times the number of tiles above 2^31 - 1; zeros_pad other than 0 or 1; a NULL pointer where one is
 * required (dx, dw and db all NULL included); a pointer not 16-byte aligned; split outside [0, 64].  MGS_ERR_WORKSPACE: fewer bytes
 * than the query's.  Element offsets are 64-bit.
 * No atomics, no workgroup waits for another, nothing to zero: bit-identical from run to run.  No host read, no allocation, no
 * state: capturable into a HIP graph. */
size_t mgs_narrow_conv3d_workspace_bytes(int64_t B, int Cin, int Cout, int64_t D, int64_t H, int64_t W);
int mgs_narrow_conv3d_forward(int64_t B, int Cin, int Cout, int64_t D, int64_t H, int64_t W, int zeros_pad, const float* x,
                              const float* w, const float* bias, float* y, mgs_stream_t stream);
int mgs_narrow_conv3d_backward(int64_t B, int Cin, int Cout, int64_t D, int64_t H, int64_t W, int zeros_pad, const float* x,
                               const float* g_y, const float* w, float* dx, float* dw, float* db, void* workspace,
                               size_t workspace_bytes, int split, mgs_stream_t stream);

/* ---- the Perceiver decoder's dense 3x3x3 / 5x5x5 convolutions with bias and leaky ReLU on the exact-f32 MFMA (SURVEY.md 2:
 * agents/manigaussian_bc/perceiver_lang_io.py, up0 = Conv3DUpsampleBlock(256, 128, 5) and final = Conv3DBlock(256, 128, 3)) --
 * additive exports, ABI v17 ----
 * Kernel k x k x k with k = 3 or 5, stride 1, NO padding (the caller's volume already carries it), dilation 1, groups 1; Cin a
 * multiple of 8 in 8..256, Cout a multiple of 32 in 32..256; every input extent at least k.  Do = Di - k + 1 and so on.
 * x and dx [B, Cin, Di, Hi, Wi], y and g_y [B, Cout, Do, Ho, Wo], w and dw [Cout, Cin, k, k, k] (nn.Conv3d's layout), bias and db
 * [Cout]: all contiguous and 16-byte aligned.  negative_slope < 0: no activation; >= 0: act(z) = z > 0 ? z : negative_slope z
 * (0: ReLU).
 *   forward:   y[b,co,o]     = act(bias[co] + sum_ci sum_tap w[co,ci,tap] x[b,ci,o + tap])                (bias may be NULL: no bias)
 *   backward:  g'            = g_y (y > 0 ? 1 : negative_slope), or g_y without an activation (y may then be NULL)
 *              dx[b,ci,i]    = sum_co sum_tap w[co,ci,tap] g'[b,co,i - tap]
 *              dw[co,ci,tap] = sum_b sum_o g'[b,co,o] x[b,ci,o + tap];   db[co] = sum_b sum_o g'[b,co,o]
 * All products run on v_mfma_f32_32x32x2_f32: k-ordered chains of fused multiply-adds in fp32.  The forward is two launches: the
 * weights are rearranged into the workspace in the order the k loop consumes them, then one implicit GEMM.  dx, dw and db may each
 * be NULL and only what is asked for is computed.  dx is three launches: g' is written into g_scratch, [B, Cout, Do + 2 (k - 1),
 * Ho + 2 (k - 1), Wo + 2 (k - 1)] zero-padded (required when dx is asked for, else it may be NULL), the flipped and transposed
 * weights into the workspace, and the forward's kernel runs on the two.  dw and db are two launches: the segments of up to 64 voxels
 * of the output rows, in their linear order, are cut into runs whose number (at most 64, and at least 8 where there are as many
 * segments) and length depend on the shape alone, every run is summed to one RECORD [Cout, Cin k^3 + 1] in the workspace (db, the
 * last column, in double), and the second launch adds the records in ascending order, in double.  split (0: chosen from the shape;
 * 1..64: forced, a test aid; never more than the number of runs) is the number of workgroups that share the runs: it says which
 * workgroup computes a record, never what the record is -- dw and db are the same bits for every split.
 * workspace: 16-byte aligned, at least as many bytes as the size query returns for the same shape (0 for shapes outside the limits,
 * else a multiple of 256); needed by both calls.
 * MGS_ERR_INVALID_ARG before any launch: k other than 3 or 5; Cin or Cout outside their limits or off their multiples; B below 1
 * or above 65535; an extent below k; (Di + k - 1)(Hi + k - 1)(Wi + k - 1) >= 2^31 (the longest (batch, channel) row there is);
 * more than 2^31 - 1 row segments; a NaN slope; a NULL pointer where one is required (dx, dw and db all NULL included); a pointer
 * not 16-byte aligned; split outside [0, 64].  MGS_ERR_WORKSPACE: fewer bytes than the query's.  Element offsets are 64-bit.
 * No atomics, no workgroup waits for another, nothing to zero: bit-identical from run to run.  No host read, no allocation, no
 * state: capturable into a HIP graph. */
size_t mgs_dense_conv3d_workspace_bytes(int64_t B, int Cin, int Cout, int k, int64_t Di, int64_t Hi, int64_t Wi);
int mgs_dense_conv3d_forward(int64_t B, int Cin, int Cout, int k, int64_t Di, int64_t Hi, int64_t Wi, float negative_slope,
                             const float* x, const float* w, const float* bias, float* y, void* workspace, size_t workspace_bytes,
                             mgs_stream_t stream);
int mgs_dense_conv3d_backward(int64_t B, int Cin, int Cout, int k, int64_t Di, int64_t Hi, int64_t Wi, float negative_slope,
                              const float* x, const float* y, const float* g_y, const float* w, float* dx, float* dw, float* db,
                              float* g_scratch, void* workspace, size_t workspace_bytes, int split, mgs_stream_t stream);

/* ---- the Perceiver's patch embedding: a Conv3d whose stride is its kernel, pad folded in (mgs_patch.hip) ----
 * patchify = Conv3DBlock(128, 128, kernel_sizes=5, strides=5, activation='relu') on [B,128,100^3] with replicate pad 2.  k is the
 * kernel AND the stride, cubic, 2..5; pad 0..k-1 on every side, zeros_pad 0: replicate (a clamp), 1: zeros (a mask); dilation 1, groups
 * 1; Cin a multiple of 8 in 8..256, Cout a multiple of 32 in 32..256.  Do = (Di + 2 pad - k) / k + 1, and so Ho, Wo; the input
 * coordinate of (output o, tap t) is i = o k + t - pad.  x and dx [B, Cin, Di, Hi, Wi], y and g_y [B, Cout, Do, Ho, Wo], w and dw
 * [Cout, Cin, k, k, k], bias and db [Cout]: all contiguous and 16-byte aligned.  negative_slope < 0: no activation; >= 0:
 * act(z) = z > 0 ? z : negative_slope z (0: ReLU).  The padded volume is never written.
 *   forward:   y[b,co,o]     = act(bias[co] + sum_ci sum_t w[co,ci,t] x[b,ci,i(o,t)])                      (bias may be NULL: no bias)
 *   backward:  g'            = g_y (y > 0 ? 1 : negative_slope), or g_y without an activation (y may then be NULL)
 *              dx[b,ci,i]    = sum over the (o,t) that map onto i, sum_co w[co,ci,t] g'[b,co,o]: one (o,t) in the interior, up to
 *                              (pad + 1)^3 taps on a replicate border, added in ascending tap order; a voxel past the last patch
 *                              belongs to no output and its dx is ZERO, written by the call itself (dx needs no zeroing)
 *              dw[co,ci,t]   = sum_b sum_o g'[b,co,o] x[b,ci,i(o,t)];   db[co] = sum_b sum_o g'[b,co,o]
 * All products run on v_mfma_f32_32x32x2_f32: k-ordered chains of fused multiply-adds in fp32, over tiles of 32 patches consecutive
 * in (od, oh, ow) order.  The forward is two launches: the weights are rearranged into the workspace in the order the k loop consumes
 * them, then one GEMM whose K dimension is not split.  dx, dw and db may each be NULL and only what is asked for is computed.  dx is
 * one launch and needs no workspace.  dw and db are two launches: the tiles of 32 patches, in their linear order, are cut into runs
 * whose number (at most 64; as many as fit 64 MB, at least 2) and length depend on the shape alone, every run is summed to one RECORD
 * [Cout, Cin k^3 + 1] in the workspace (db, the last column, in double), and the second launch adds the records in ascending order, in
 * double.  split (0: chosen from the shape; 1..64: forced, a test aid; never more than the number of runs) is the number of
 * workgroups that share the runs: it says which workgroup computes a record, never what the record is.
 * workspace: 16-byte aligned, at least as many bytes as the size query returns for the same shape (0 for shapes outside the limits,
 * else a multiple of 256); needed by the forward, and by the backward where dw or db is asked for (else it may be NULL).
 * MGS_ERR_INVALID_ARG before any launch: k outside 2..5; pad outside 0..k-1; Cin or Cout outside their limits or off their
 * multiples; B below 1 or above 65535; an extent below 1 or, padded, below k; Di Hi Wi >= 2^31; B Do Ho Wo >= 2^31; zeros_pad other
 * than 0 or 1; a NaN slope; a NULL pointer where one is required (dx, dw and db all NULL included); a pointer not 16-byte aligned;
 * split outside [0, 64].  MGS_ERR_WORKSPACE: fewer bytes than the query's.  Element offsets are 64-bit.
 * No atomics, no workgroup waits for another, nothing to zero: bit-identical from run to run; dx is the same bits whether or not dw
 * and db are asked for.  No host read, no allocation, no state: capturable into a HIP graph. */
size_t mgs_patch_conv3d_workspace_bytes(int64_t B, int Cin, int Cout, int k, int pad, int64_t Di, int64_t Hi, int64_t Wi);
int mgs_patch_conv3d_forward(int64_t B, int Cin, int Cout, int k, int pad, int64_t Di, int64_t Hi, int64_t Wi, int zeros_pad,
                             float negative_slope, const float* x, const float* w, const float* bias, float* y, void* workspace,
                             size_t workspace_bytes, mgs_stream_t stream);
int mgs_patch_conv3d_backward(int64_t B, int Cin, int Cout, int k, int pad, int64_t Di, int64_t Hi, int64_t Wi, int zeros_pad,
                              float negative_slope, const float* x, const float* y, const float* g_y, const float* w, float* dx,
                              float* dw, float* db, void* workspace, size_t workspace_bytes, int split, mgs_stream_t stream);

/* Per-stage device timing (hipEvents on the caller's stream), enabled with
 * mgs_set_option("profile", 1) (render backward only) or 2 (every stage).  mgs_profile_read waits for the
 * recorded events, writes the summed milliseconds and launch counts per stage ([mgs_profile_num_stages()]),
 * and recycles the events when reset != 0. */
int mgs_profile_num_stages(void);
const char* mgs_profile_stage_name(int stage);
int mgs_profile_read(double* total_ms, int32_t* counts, int reset);

/* Diagnostic, BLOCKING (two small device->host copies + a stream synchronise): what the forward that last ran on a's
 * workspaces left for its backward, in the units that state is kept in -- *incidences = (8x8 pixel block, Gaussian) pairs of
 * the chunks some pixel of the block visited, *chunks = those 64-survivor chunks, *pixel_chunks = (pixel, chunk) pairs visited
 * (what the per-chunk state costs).  V = 0: a single-view forward, V > 0: a batch of V views.  bench.py prices the render
 * kernels' HBM traffic with them (the reference's dataflow has no such state: RAST/cuda_rasterizer/backward.cu:399-593
 * walks the tile lists again). */
int mgs_forward_stats(const MgsRasterArgs* a, int32_t V, int64_t* incidences, int64_t* chunks, int64_t* pixel_chunks,
                      mgs_stream_t stream);

/* Diagnostic: byte offsets, inside a geom workspace of mgs_geom_bytes(P, M, W, H) bytes, of what the forward preprocess wrote
 * per Gaussian: depths f32[P]; rec f32x4[2P] = {x, y (pixels), conic.x, conic.y}{conic.z, opacity, hx, hy}; rgb f32[3P];
 * cov3D f32[6P] (the reference's GeometryState: RAST/cuda_rasterizer/rasterizer_impl.h:30-46).  The parity tests compare
 * them bit for bit with the reference kernels' values. */
int mgs_debug_geom_layout(int P, int M, int W, int H, size_t* depths, size_t* rec, size_t* rgb, size_t* cov3D);

/* Diagnostic: where the binning of a forward left its per-tile lists.  `a` = that forward's arguments (its binning_bytes /
 * binning_capacity / chunk_pool describe the carving), V = 0 for a single view or the number of views of a batch.  Byte offsets
 * inside the binning workspace of keys_unsorted u64[capacity] (depth bits << 32 | id, tile-major, unordered inside a tile) and
 * point_list u32[capacity] (sorted ids), and inside the img workspace of ranges uint2[tiles] ({first, end} of each tile's slice).
 * The parity tests check that every tile's list is its slice of keys in (depth bits, id) order -- the reference's order
 * (RAST/cuda_rasterizer/rasterizer_impl.cu:306-320). */
int mgs_debug_binning_layout(const MgsRasterArgs* a, int32_t V, size_t* keys_unsorted, size_t* point_list, size_t* img_ranges,
                             int32_t* capacity);
/* ... and, when the forward preprocess wrote the keys itself ("direct" binning: the bucket rank, bin_mode 2, on a workspace
 * that has room for tiles x P keys -- see mgs_binning_direct_extra), where: *stride = P and tile t's unordered slice lies at
 * u64[*keys / 8 + t * P ...] of the binning workspace (its length is the tile's range); *stride = 0: the bin scatter kernel wrote
 * the compact keys_unsorted above. */
int mgs_debug_direct_keys(const MgsRasterArgs* a, int32_t V, size_t* keys, int32_t* stride);

/* Diagnostic, host code only (an additive export, ABI v17): every region the geom, img and binning workspaces of a forward
 * are carved into, in carving order per workspace -- computed by the carving functions the kernels' host code uses.  `a` = the
 * forward's arguments (shape, M, the three byte counts, binning_capacity / chunk_pool, opt; its pointers are not read), V as
 * above.  kind: MGS_REGION_FLOAT if no kernel derives an address, a loop bound, an LDS index or a sort bucket from the region's
 * words when it reads them legitimately; MGS_REGION_INDEX otherwise and in doubt (the table, with each region's
 * writer, reader and what part is written).  A test that dirties workspaces may put any bytes into a FLOAT region and nothing
 * but words of the same layout into an INDEX region.  The last entry is the direct keys (mgs_debug_direct_keys) where this
 * forward's preprocess writes them: alias = 1 if they lie inside the two key arrays listed before them, 0 if behind the carved
 * arrays.  Writes min(*count, max_regions) entries; max_regions = 0 only counts. */
#define MGS_REGION_FLOAT 0
#define MGS_REGION_INDEX 1
#define MGS_WORKSPACE_GEOM 0
#define MGS_WORKSPACE_IMG 1
#define MGS_WORKSPACE_BINNING 2
typedef struct MgsWorkspaceRegion {
  char name[24];
  int32_t workspace; /* MGS_WORKSPACE_* */
  int32_t kind;      /* MGS_REGION_* */
  int32_t alias;     /* 1: overlaps regions listed before it */
  int32_t pad_;
  size_t offset;     /* bytes from the start of its workspace */
  size_t bytes;
} MgsWorkspaceRegion;
int mgs_debug_workspace_regions(const MgsRasterArgs* a, int32_t V, MgsWorkspaceRegion* out, int32_t max_regions,
                                int32_t* count);

/* Diagnostic: with MgsOptions.dbg = 256 the render forward stamps s_memtime per (workgroup < 512, wave, phase);
 * this copies the 512 * 16 * 24 uint64 stamps of the last forward to `host` (scripts/trace_fwd.py prints the timeline). */
int mgs_debug_read_trace(unsigned long long* host, size_t count);
/* ... and of the render backward: 512 * 16 * 16 stamps (first chunk of every wave; scripts/trace_bwd.py). */
int mgs_debug_read_trace_bwd(unsigned long long* host, size_t count);

/* Device self-test of the wave64 cross-lane primitives used by the render kernels (DPP rotations,
 * v_permlane16/32_swap butterflies).  Returns 0 if every primitive matches its definition. */
int mgs_selftest(mgs_stream_t stream);

/* Counter calibration (scripts/sq_counters.sh): one workgroup-per-CU launch of a kernel with a KNOWN instruction mix per
 * wave -- iters x (64 v_fma_f32 + 8 v_mfma_f32_32x32x2_f32 + 4 ds_read_b32) -- so that a rocprofv3 --pmc pass can be
 * validated against exact counts before its numbers for the render kernels are trusted.  sink: >= 256*1024 floats. */
int mgs_calibration_kernel(int iters, float* sink, mgs_stream_t stream);

/* ... and of the bucket-rank binning (bin_mode 2): 1024 workgroups x 16 stamps (scripts/trace_bin.py). */
int mgs_debug_read_trace_bin(unsigned long long* host, size_t count);

#ifdef __cplusplus
}
#endif
#endif /* MGSPLAT_H_ */
