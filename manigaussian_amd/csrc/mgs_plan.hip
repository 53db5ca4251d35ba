// mgs_plan.hip -- HOW LARGE: the workspace size queries of include/mgsplat.h and the plan both host bindings build on them
// (arena and worst case, capacities from the marks, option tuning, gradient layout).  Pure arithmetic over the carvers of
// mgs_common.h: no kernel, no HIP runtime call, no state -- this file runs on a host without a device
// (tests/test_plan.py, tests/tools/plan_walk.cpp).
#include <limits.h>

#include "mgs_common.h"

using namespace mgs;

static Pass views_shape(int W, int H, int V) { return pass_of(0, W, H, 0, V > 0 ? V : 1); }

// A shape the plan answers for, or the library's error.  Past this check P x V, P x S and every field of its Pass fit an int.
static int check_shape(const MgsPlanShape* s, const char* fn) {
  if (!s) { set_error("%s: shape is NULL", fn); return MGS_ERR_INVALID_ARG; }
  const bool dims = s->P >= 0 && s->M >= 0 && s->F >= 0 && s->W >= 1 && s->H >= 1 && s->V >= 0 && s->S >= 0;
  if (!dims || s->V > MGS_MAX_VIEWS || s->S > MGS_MAX_VIEWS || (s->S > 0 && s->V == 0)) {
    set_error("%s: bad shape P=%d M=%d F=%d W=%d H=%d V=%d S=%d (V, S <= %d; sets need views)", fn, s->P, s->M, s->F, s->W,
              s->H, s->V, s->S, MGS_MAX_VIEWS);
    return MGS_ERR_INVALID_ARG;
  }
  const int64_t rows = (int64_t)s->P * (s->V > s->S ? s->V : s->S > 0 ? s->S : 1);
  const int64_t tiles = ((s->W + (int64_t)TILE - 1) / TILE) * ((s->H + (int64_t)TILE - 1) / TILE);
  if (rows > INT_MAX || tiles * TILE * MGS_MAX_VIEWS > INT_MAX) {  // (the rows of a batch's atlas: V x tile rows x 16)
    set_error("%s: %lld rows of P=%d, V=%d, S=%d or the tiles of %d x %d do not fit an int", fn, (long long)rows, s->P, s->V,
              s->S, s->W, s->H);
    return MGS_ERR_INVALID_ARG;
  }
  return MGS_OK;
}
static Pass pass_of(const MgsPlanShape& s) { return pass_of(s.P, s.W, s.H, s.F, s.V, nullptr, s.S); }

extern "C" {

size_t mgs_geom_bytes(int P, int M, int W, int H) { return geom_bytes(pass_of(P, W, H, 0, 0), M); }
size_t mgs_img_bytes(int W, int H) { return img_bytes(pass_of(0, W, H, 0, 0), W); }
size_t mgs_binning_bytes2(int R, int chunk_pool, int W, int H, int F) { return binning_bytes_T(R, chunk_pool, num_tiles(W, H), F); }
size_t mgs_binning_bytes(int R, int W, int H, int F) { return binning_bytes_T(R, 0, num_tiles(W, H), F); }
int mgs_chunk_pool_max(int R, int W, int H) { return (int)chunk_pool_max(R > 0 ? (size_t)R : 1, num_tiles(W, H)); }
size_t mgs_backward_scratch_bytes(int P, int M, int F) { size_t t; carve_bwd(nullptr, P, M, F, &t); return t; }

size_t mgs_views_geom_bytes(int P, int M, int W, int H, int V) { return geom_bytes(pass_of(P, W, H, 0, V > 0 ? V : 1), M); }
size_t mgs_views_img_bytes(int W, int H, int V) { return img_bytes(views_shape(W, H, V), W); }
size_t mgs_views_binning_bytes(int R, int W, int H, int F, int V) { return binning_bytes_T(R, 0, views_shape(W, H, V).T, F); }
size_t mgs_views_binning_bytes2(int R, int chunk_pool, int W, int H, int F, int V) {
  return binning_bytes_T(R, chunk_pool, views_shape(W, H, V).T, F);
}
int mgs_views_chunk_pool_max(int R, int W, int H, int V) {
  return (int)chunk_pool_max(R > 0 ? (size_t)R : 1, views_shape(W, H, V).T);
}
size_t mgs_views_backward_scratch_bytes(int P, int M, int F, int V) { return mgs_backward_scratch_bytes(P * (V > 0 ? V : 1), M, F); }
// (the scratch holds the render backward's sums per (view, Gaussian) pair; the per-set accumulators are the caller's
//  dL_dcolors / dL_dfeature outputs)
size_t mgs_sets_backward_scratch_bytes(int P, int M, int F, int V, int S) {
  (void)S;
  return mgs_views_backward_scratch_bytes(P, M, F, V);
}
// Direct binning (mgs_common.h direct_keys_needed; mgs_api.hip direct_region finds the room in a call's workspace)
size_t mgs_binning_direct_extra(int P, int V, int W, int H) {
  const int v = V > 0 ? V : 1;
  const size_t need = direct_keys_needed((size_t)(P > 0 ? P : 0) * v, v, num_tiles(W, H) * v);
  return need && need <= DIRECT_MAX_KEYS ? need * sizeof(uint64_t) + 256 : 0;
}

// ---- the plan -------------------------------------------------------------------------------------------------------------
int mgs_plan_arena(const MgsPlanShape* s, int64_t budget_bytes, MgsArenaPlan* out) {
  if (!out) { set_error("mgs_plan_arena: out is NULL"); return MGS_ERR_INVALID_ARG; }
  *out = MgsArenaPlan{};
  if (int rc = check_shape(s, "mgs_plan_arena")) return rc;
  const Pass p = pass_of(*s);
  out->geom_bytes = align_up(geom_bytes(p, s->M));
  out->img_bytes = align_up(img_bytes(p, s->W));
  out->worst_capacity = (int64_t)p.Pg * p.T;
  if (out->worst_capacity < ((int64_t)1 << 30)) out->worst_bytes = binning_bytes_T((int)out->worst_capacity, 0, p.T, s->F);
  out->worst_fits = out->worst_bytes > 0 && budget_bytes >= 0 && out->worst_bytes <= (uint64_t)budget_bytes;
  if (out->worst_fits) out->worst_pool = (int32_t)chunk_pool_max(out->worst_capacity > 0 ? (size_t)out->worst_capacity : 1, p.T);
  return MGS_OK;
}

size_t mgs_plan_binning_bytes(const MgsPlanShape* s, int64_t capacity, int64_t chunk_pool, int with_direct_room) {
  if (check_shape(s, "mgs_plan_binning_bytes")) return 0;
  if (capacity < 0 || capacity > INT_MAX || chunk_pool < 0 || chunk_pool > INT_MAX) {
    set_error("mgs_plan_binning_bytes: capacity %lld / chunk pool %lld do not fit an int", (long long)capacity, (long long)chunk_pool);
    return 0;
  }
  const size_t carved = binning_bytes_T((int)capacity, (int)chunk_pool, pass_of(*s).T, s->F);
  return with_direct_room ? align_up(carved) + mgs_binning_direct_extra(s->P, s->V, s->W, s->H) : carved;
}

int mgs_plan_capacity(const MgsPlanShape* s, int how, int64_t R, int64_t chunks, double head_instances, double head_chunks,
                      int64_t* capacity, int64_t* chunk_pool) {
  if (!capacity || !chunk_pool) { set_error("mgs_plan_capacity: an output is NULL"); return MGS_ERR_INVALID_ARG; }
  *capacity = *chunk_pool = 0;
  if (int rc = check_shape(s, "mgs_plan_capacity")) return rc;
  const int64_t lim = (int64_t)1 << 52;  // counts a double holds exactly; far above anything a workspace can be sized for
  if (how == MGS_SIZE_HEADROOM && R >= 0 && R < lim && chunks >= 0 && chunks < lim && head_instances >= 1.0 &&
      head_instances < 1024.0 && head_chunks >= 1.0 && head_chunks < 1024.0) {
    *capacity = (int64_t)((double)R * head_instances) + 4096;
    *chunk_pool = (int64_t)((double)chunks * head_chunks) + 64;
  } else if (how == MGS_SIZE_COUNT && R < lim) {
    *capacity = (R >= 0 ? R + R / 4 : 4 * (int64_t)(s->V > 0 ? s->V : 1) * s->P) + 4096;  // (pool 0: the worst case for it)
  } else {
    set_error("mgs_plan_capacity: how=%d R=%lld chunks=%lld head-room %g, %g", how, (long long)R, (long long)chunks,
              head_instances, head_chunks);
    return MGS_ERR_INVALID_ARG;
  }
  return MGS_OK;
}

int mgs_plan_options(const MgsPlanShape* s, int64_t R, MgsOptions* opt) {
  if (!opt) { set_error("mgs_plan_options: opt is NULL"); return MGS_ERR_INVALID_ARG; }
  if (int rc = check_shape(s, "mgs_plan_options")) return rc;
  const int64_t T = pass_of(*s).T;
  const bool default_seg = opt->seg == 2048;
  // long per-tile lists (BASELINE configs[4]'s shape: 14 000 instances per tile = 7 segments of 2048, every key ranked in the
  // six others; sort + merge 115 us instead of 123, profiles/r04_exp_segsort.log)
  if (default_seg && R > 8192 * T) opt->seg = 4096;
  // ... and the bucket rank (bin_mode 2: a tile's slice in registers, <= 16 384 keys) hands VERY long lists -- e.g. 2 000 000
  // Gaussians on a 128 x 128 image -- to the segment sort + rank merge, whose work is spread over one workgroup per segment
  // (590 against 505 us there; the bucket rank wins at every BASELINE shape: scripts/diag/quick_binmode.py)
  if (opt->bin_mode == 2 && R > 24576 * T) {
    opt->bin_mode = 1;
    if (default_seg) opt->seg = 4096;
  }
  return MGS_OK;
}

int mgs_plan_gradients(const MgsPlanShape* s, MgsGradientPlan* out) {
  if (!out) { set_error("mgs_plan_gradients: out is NULL"); return MGS_ERR_INVALID_ARG; }
  *out = MgsGradientPlan{};
  if (int rc = check_shape(s, "mgs_plan_gradients")) return rc;
  const int64_t n = (int64_t)s->P * (s->V > 0 ? s->V : 1);  // (view, Gaussian) pairs
  const int64_t G = (int64_t)s->P * (s->S > 0 ? s->S : 1);  // (set, Gaussian) rows
  const int64_t ncol = s->colors_precomp ? G : n, M = s->M, F = s->F;
  const int64_t scratch = (int64_t)((mgs_backward_scratch_bytes((int)n, s->M, s->F) + 3) / 4);
  int64_t o = 0;
  out->scratch = o;   o += scratch;
  out->colors = o;    o += 3 * ncol;
  out->feature = o;   o += F * G;
  out->means3D = o;   o += 3 * G;
  out->opacity = o;   o += G;
  out->sh = o;        o += 3 * M * G;
  out->scales = o;    o += 3 * G;
  out->rotations = o; o += 4 * G;
  out->cov3D = o;     o += 6 * G;
  out->means2D = o;   o += 3 * n;
  out->pad = o;       o += 4;
  out->total = o;
  out->accum_bytes = (size_t)((out->means3D * 4 + 15) / 16 * 16);
  return MGS_OK;
}

}  // extern "C"
