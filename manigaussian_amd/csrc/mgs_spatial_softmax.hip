// mgs_spatial_softmax.hip -- the Perceiver's aggregated features (helpers/network_utils.py:927-963, SpatialSoftmax3D, and the
// nn.AdaptiveMaxPool3d(1) beside it in agents/manigaussian_bc/perceiver_lang_io.py:384,485,504), fused, fp32, forward and
// backward.  A row is one (batch, channel): N = D H W floats.
//
//   keypoints = sum_i p_i pos(i),  p = softmax(row / temperature);   maxpool = max(row)
//
// Forward, one read of the volume: a row is cut into `slices` pieces of whole 16-byte vectors, one 256-thread workgroup each.  A
// lane keeps a running maximum m and sum exp((x - m) / t), sum exp(..) a, .. b, .. c, where (a, b, c) are the INTEGER coordinates of
// the element (flat index i = (a D + b) W + c); a register tile of 16 values is maximised first and the sums are rescaled only
// when the tile raises m (rare after the first tiles), so every element costs one v_exp_f32.  The coordinates are advanced from
// tile to tile by the precomputed digits of the lane stride (1024 elements), never by a division per element; the affine map to
// [-1, 1] is applied once per row, in double, by the combine launch.  The first index of the maximum travels with m: ties go to
// the lower index inside a lane (ascending scan, strict >), between lanes, between waves and between slices (min of the indices),
// so the result does not depend on the split.  Each workgroup writes ONE 32-byte record into the caller's workspace;
// ss_combine_kernel (one lane per row) folds a row's records in slice order and writes keypoints, maxpool and the six row
// statistics the backward needs.  No atomics, no waiting between workgroups, nothing to zero: the same bits from run to run.
//
// Backward, one launch, one read of the volume and one write of its gradient:
//   dL/dx_i = p_i / t * sum_axis g_axis (pos_axis(i) - E_axis) + g_max [i == argmax],   p_i = exp((x_i - m) / t) / sum
// from the row statistics (m, sum, E, argmax); nothing of size N was saved.
//
// Rows start at element row * N of a 16-byte aligned volume, so for N % 4 != 0 a row's first (-row N) & 3 elements (the head)
// and the last ones behind its whole vectors (the tail) are read and written as scalars by the first and the last slice;
// vector accesses are always aligned.  The FAST instantiation (W % 4 == 0, hence no heads) knows that the four elements of a
// vector share a and b.  Element offsets are 64-bit; indices inside a row are 32-bit unsigned (N <= 2^31 - 1).
#include <float.h>
#include <math.h>

#include "mgs_common.h"

namespace mgs {

constexpr int SS_THREADS = 256;
constexpr int SS_UNROLL = 4;                // 16-byte loads a lane has in flight: a register tile of 16 values
constexpr int SS_STRIDE = SS_THREADS * 4;   // elements between two consecutive vectors of a lane
constexpr int SS_MAX_SLICES = 64;
constexpr int SS_TARGET_BLOCKS = 2048;      // 256 CUs x 8 workgroups of 4 waves
constexpr int SS_MIN_SLICE_VEC = 512;       // a slice is not cut below 2 vectors per lane
constexpr int SS_REC = 8;                   // floats per slice record: m, index, s, sa, sb, sc, 1 if the slice holds a NaN, (unused)
constexpr int SS_STATS = 6;                 // floats per row: m, sum, E_x, E_y, E_z, argmax (bits of a uint32)
constexpr uint32_t SS_NO_INDEX = 0xffffffffu;

typedef float ssf4 __attribute__((ext_vector_type(4)));

struct SsGeom {
  uint32_t N, D, H, W, DW;
  uint32_t qa, qb, qc;   // SS_STRIDE = qa D W + qb W + qc, qb < D, qc < W
  uint32_t C, slices;
  float kk;              // log2(e) / temperature
  float inv_t;           // 1 / temperature
};

struct SsPos { uint32_t a, b, c; };

__device__ __forceinline__ SsPos ss_decompose(uint32_t i, const SsGeom& g) {
  SsPos p;
  p.a = i / g.DW;
  const uint32_t r = i - p.a * g.DW;
  p.b = r / g.W;
  p.c = r - p.b * g.W;
  return p;
}
// by SS_STRIDE elements: c + qc < 2 W and b + qb + 1 < 2 D, so one conditional subtraction per digit
__device__ __forceinline__ void ss_advance(SsPos& p, const SsGeom& g) {
  p.c += g.qc;
  uint32_t w = p.c >= g.W ? 1u : 0u;
  p.c -= w ? g.W : 0u;
  p.b += g.qb + w;
  w = p.b >= g.D ? 1u : 0u;
  p.b -= w ? g.D : 0u;
  p.a += g.qa + w;
}
// by one element
__device__ __forceinline__ void ss_step(SsPos& p, const SsGeom& g) {
  ++p.c;
  const bool w = p.c == g.W;
  p.c = w ? 0u : p.c;
  p.b += w ? 1u : 0u;
  const bool w2 = p.b == g.D;
  p.b = w2 ? 0u : p.b;
  p.a += w2 ? 1u : 0u;
}

// the split of a row, the same in every kernel
struct SsRow {
  int64_t start;   // element offset of the row in the volume
  uint32_t head, nvec, tail, v0, v1;
};
template <bool FAST>
__device__ __forceinline__ SsRow ss_row(uint32_t row, uint32_t slice, const SsGeom& g) {
  SsRow r;
  r.start = (int64_t)row * (int64_t)g.N;
  r.head = FAST ? 0u : min((uint32_t)((-r.start) & 3), g.N);
  r.nvec = (g.N - r.head) >> 2;
  r.tail = g.N - r.head - 4u * r.nvec;
  const uint32_t per = (r.nvec + g.slices - 1) / g.slices;
  r.v0 = min(slice * per, r.nvec);
  r.v1 = min(r.v0 + per, r.nvec);
  return r;
}

// ---- forward -------------------------------------------------------------------------------------------------------------------
struct SsPart {
  float m;
  uint32_t idx;
  float s, sa, sb, sc;
};

__device__ __forceinline__ float ss_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// Two partial sums into one.  Written so that combine(A, B) and combine(B, A) are the same bits (no contraction into an fma).
__device__ __forceinline__ SsPart ss_combine(const SsPart& A, const SsPart& B, float kk) {
#pragma clang fp contract(off)
  SsPart r;
  r.m = fmaxf(A.m, B.m);
  const float ms = r.m == -INFINITY ? 0.f : r.m;   // (two empty parts: no -inf - -inf)
  const float fa = ss_exp2((A.m - ms) * kk), fb = ss_exp2((B.m - ms) * kk);
  r.idx = A.m > B.m ? A.idx : (B.m > A.m ? B.idx : min(A.idx, B.idx));
  r.s = A.s * fa + B.s * fb;
  r.sa = A.sa * fa + B.sa * fb;
  r.sb = A.sb * fa + B.sb * fb;
  r.sc = A.sc * fa + B.sc * fb;
  return r;
}

__device__ __forceinline__ SsPart ss_single(float x, uint32_t i, const SsGeom& g) {
  const SsPos q = ss_decompose(i, g);
  SsPart p;
  p.m = x; p.idx = i; p.s = 1.f; p.sa = (float)q.a; p.sb = (float)q.b; p.sc = (float)q.c;
  return p;
}

template <bool FAST>
__global__ __launch_bounds__(SS_THREADS) void ss_fwd_kernel(SsGeom g, const float* __restrict__ feature, float* __restrict__ records) {
  const uint32_t row = blockIdx.x / g.slices, slice = blockIdx.x - row * g.slices;
  const uint32_t tid = threadIdx.x;
  const SsRow r = ss_row<FAST>(row, slice, g);
  const float* x = feature + r.start;
  const float kk = g.kk;

  SsPart p;
  p.m = -INFINITY; p.idx = SS_NO_INDEX; p.s = p.sa = p.sb = p.sc = 0.f;
  if (!FAST && slice == 0 && tid < r.head) p = ss_single(x[tid], tid, g);

  const ssf4* xv = reinterpret_cast<const ssf4*>(x + r.head);
  uint32_t t = r.v0 + tid;
  if (t < r.v1) {
    SsPos pos = ss_decompose(r.head + 4u * t, g);
    for (; t < r.v1; t += SS_THREADS * SS_UNROLL) {
      ssf4 v[SS_UNROLL];
#pragma unroll
      for (int k = 0; k < SS_UNROLL; ++k) {
        const uint32_t tk = t + k * SS_THREADS;
        v[k] = tk < r.v1 ? xv[tk] : (ssf4)(-INFINITY);
      }
      float tm = -INFINITY;
#pragma unroll
      for (int k = 0; k < SS_UNROLL; ++k) tm = fmaxf(fmaxf(fmaxf(tm, v[k].x), fmaxf(v[k].y, v[k].z)), v[k].w);
      if (tm > p.m) {  // the tile raises the maximum: its first element that holds it, and the sums move to the new base
        uint32_t at = 0;
#pragma unroll
        for (int k = SS_UNROLL - 1; k >= 0; --k) {
          const uint32_t base = 4u * (t + k * SS_THREADS);
          at = v[k].w == tm ? base + 3u : at;
          at = v[k].z == tm ? base + 2u : at;
          at = v[k].y == tm ? base + 1u : at;
          at = v[k].x == tm ? base : at;
        }
        p.idx = r.head + at;
        const float f = ss_exp2((p.m - tm) * kk);
        p.s *= f; p.sa *= f; p.sb *= f; p.sc *= f;
        p.m = tm;
      }
      const float m = p.m;
#pragma unroll
      for (int k = 0; k < SS_UNROLL; ++k) {
        const float e0 = ss_exp2((v[k].x - m) * kk), e1 = ss_exp2((v[k].y - m) * kk);
        const float e2 = ss_exp2((v[k].z - m) * kk), e3 = ss_exp2((v[k].w - m) * kk);
        if (FAST) {  // c, c + 1, c + 2, c + 3 in one line of W
          const float e4 = (e0 + e1) + (e2 + e3);
          p.s += e4;
          p.sa = fmaf(e4, (float)pos.a, p.sa);
          p.sb = fmaf(e4, (float)pos.b, p.sb);
          p.sc += fmaf(e4, (float)pos.c, fmaf(3.f, e3, fmaf(2.f, e2, e1)));
        } else {
          SsPos q = pos;
          const float e[4] = {e0, e1, e2, e3};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            p.s += e[j];
            p.sa = fmaf(e[j], (float)q.a, p.sa);
            p.sb = fmaf(e[j], (float)q.b, p.sb);
            p.sc = fmaf(e[j], (float)q.c, p.sc);
            ss_step(q, g);
          }
        }
        ss_advance(pos, g);
      }
    }
  }
  if (!FAST && slice == g.slices - 1 && tid < r.tail) {
    const uint32_t i = r.head + 4u * r.nvec + tid;
    p = ss_combine(p, ss_single(x[i], i, g), kk);
  }

  // lanes of a wave (butterfly), then the four waves in order
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    SsPart o;
    o.m = __shfl_xor(p.m, d); o.idx = __shfl_xor(p.idx, d);
    o.s = __shfl_xor(p.s, d); o.sa = __shfl_xor(p.sa, d); o.sb = __shfl_xor(p.sb, d); o.sc = __shfl_xor(p.sc, d);
    p = ss_combine(p, o, kk);
  }
  __shared__ SsPart wave_part[SS_THREADS / 64];
  if ((tid & 63u) == 0) wave_part[tid >> 6] = p;
  // The running maximum is fmaxf's, which drops a NaN: right for the softmax, whose sums turn NaN by themselves, wrong for the
  // max-pool, which is NaN in nn.AdaptiveMaxPool3d.  The sum tells, at no cost to the pass: a slice that holds a NaN has a NaN sum
  // (so has one with a +inf: inf - inf in the exponent).  Only then the workgroup reads its slice once more and looks for a NaN.
  int has_nan = 0;
  if (__syncthreads_or(p.s != p.s ? 1 : 0)) {
    const uint32_t begin = slice == 0 ? 0u : r.head + 4u * r.v0, end = slice == g.slices - 1 ? g.N : r.head + 4u * r.v1;
    int mine = 0;
    for (uint32_t i = begin + tid; i < end; i += SS_THREADS) mine |= x[i] != x[i] ? 1 : 0;
    has_nan = __syncthreads_or(mine);
  }
  if (tid == 0) {
    p = wave_part[0];
#pragma unroll
    for (int w = 1; w < SS_THREADS / 64; ++w) p = ss_combine(p, wave_part[w], kk);
    ssf4* rec = reinterpret_cast<ssf4*>(records + (size_t)blockIdx.x * SS_REC);
    ssf4 lo, hi;
    lo.x = p.m; lo.y = __uint_as_float(p.idx); lo.z = p.s; lo.w = p.sa;
    hi.x = p.sb; hi.y = p.sc; hi.z = has_nan ? 1.f : 0.f; hi.w = 0.f;
    rec[0] = lo;
    rec[1] = hi;
  }
}

// np.linspace(-1, 1, n)[j] at the mean index `mean` (linspace's own arithmetic: start + j * step; n = 1 gives [-1])
__device__ __forceinline__ float ss_lin(double mean, uint32_t n) {
  return n > 1 ? (float)(-1.0 + mean * (2.0 / (double)(n - 1))) : -1.f;
}

// one lane per row: the row's records in slice order
__global__ __launch_bounds__(SS_THREADS) void ss_combine_kernel(SsGeom g, uint32_t rows, const float* __restrict__ records,
                                                                float* __restrict__ keypoints, int64_t kp_stride,
                                                                float* __restrict__ maxpool, int64_t mp_stride,
                                                                float* __restrict__ stats) {
  const uint32_t row = blockIdx.x * SS_THREADS + threadIdx.x;
  if (row >= rows) return;
  const float* rec = records + (size_t)row * g.slices * SS_REC;
  float m = -INFINITY;
  uint32_t idx = SS_NO_INDEX;
  double s = 0, sa = 0, sb = 0, sc = 0;
  bool has_nan = false;
  for (uint32_t j = 0; j < g.slices; ++j, rec += SS_REC) {
    const float mj = rec[0];
    has_nan |= rec[6] != 0.f;
    const uint32_t ij = __float_as_uint(rec[1]);
    const float mn = fmaxf(m, mj);
    const float ms = mn == -INFINITY ? 0.f : mn;
    const double f_old = (double)ss_exp2((m - ms) * g.kk), f_new = (double)ss_exp2((mj - ms) * g.kk);
    idx = m > mj ? idx : (mj > m ? ij : min(idx, ij));
    s = s * f_old + (double)rec[2] * f_new;
    sa = sa * f_old + (double)rec[3] * f_new;
    sb = sb * f_old + (double)rec[4] * f_new;
    sc = sc * f_old + (double)rec[5] * f_new;
    m = mn;
  }
  // pos_x follows b (linspace over D), pos_y follows a (over H), pos_z follows c (over W): np.meshgrid's 'xy' order
  const float ex = ss_lin(sb / s, g.D), ey = ss_lin(sa / s, g.H), ez = ss_lin(sc / s, g.W);
  const uint32_t b = row / g.C, c = row - b * g.C;
  float* kp = keypoints + (int64_t)b * kp_stride + 3 * (int64_t)c;
  kp[0] = ex; kp[1] = ey; kp[2] = ez;
  if (maxpool) {
    const float mp = has_nan ? __builtin_nanf("") : m;   // (the forward's flag: the maximum of a row that holds a NaN is NaN)
    maxpool[(int64_t)b * mp_stride + c] = mp;   // (the statistics keep m)
  }
  float* st = stats + (size_t)row * SS_STATS;
  st[0] = m; st[1] = (float)s; st[2] = ex; st[3] = ey; st[4] = ez; st[5] = __uint_as_float(idx);
}

// ---- backward ------------------------------------------------------------------------------------------------------------------
// float32(linspace(-1, 1, n)[j]) to one ulp: (2 j - (n - 1)) / (n - 1), the numerator exact
struct SsAxis { float off, scale, bias; };
__device__ __forceinline__ SsAxis ss_axis(uint32_t n) {
  SsAxis a;
  a.off = (float)(n - 1);
  a.scale = n > 1 ? 1.f / (float)(n - 1) : 0.f;
  a.bias = n > 1 ? 0.f : -1.f;
  return a;
}
__device__ __forceinline__ float ss_coord(uint32_t j, const SsAxis& a) { return fmaf(2.f * (float)j - a.off, a.scale, a.bias); }

struct SsBwdRow {
  float m, ps, ex, ey, ez, gx, gy, gz, gm;
  uint32_t arg;
  SsAxis ax, ay, az;
};
__device__ __forceinline__ float ss_grad(float x, const SsPos& q, const SsBwdRow& R, float kk) {
  const float w = fmaf(R.gy, ss_coord(q.a, R.ay) - R.ey, fmaf(R.gx, ss_coord(q.b, R.ax) - R.ex, R.gz * (ss_coord(q.c, R.az) - R.ez)));
  return ss_exp2((x - R.m) * kk) * R.ps * w;
}

template <bool FAST>
__global__ __launch_bounds__(SS_THREADS) void ss_bwd_kernel(SsGeom g, const float* __restrict__ feature, const float* __restrict__ stats,
                                                            const float* __restrict__ g_kp, int64_t gk_stride,
                                                            const float* __restrict__ g_max, int64_t gm_stride,
                                                            float* __restrict__ g_feature) {
  const uint32_t row = blockIdx.x / g.slices, slice = blockIdx.x - row * g.slices;
  const uint32_t tid = threadIdx.x;
  const SsRow r = ss_row<FAST>(row, slice, g);
  const float* x = feature + r.start;
  float* dx = g_feature + r.start;
  const float kk = g.kk;

  SsBwdRow R;
  {
    const float* st = stats + (size_t)row * SS_STATS;
    R.m = st[0]; R.ps = g.inv_t / st[1]; R.ex = st[2]; R.ey = st[3]; R.ez = st[4]; R.arg = __float_as_uint(st[5]);
    const uint32_t b = row / g.C, c = row - b * g.C;
    const float* gk = g_kp ? g_kp + (int64_t)b * gk_stride + 3 * (int64_t)c : nullptr;
    R.gx = gk ? gk[0] : 0.f; R.gy = gk ? gk[1] : 0.f; R.gz = gk ? gk[2] : 0.f;
    R.gm = g_max ? g_max[(int64_t)b * gm_stride + c] : 0.f;
    // A NaN or infinite keypoint gradient makes the whole row's gradient NaN in the reference: its softmax backward subtracts
    // sum_j g_j p_j, which is then inf - inf or NaN.  g (pos - E) alone would give +-inf.  (g - g is 0 for a finite g, else NaN,
    // and R.ps > 0 keeps its bits when 0 is added.)
    R.ps += (R.gx - R.gx) + (R.gy - R.gy) + (R.gz - R.gz);
    R.ax = ss_axis(g.D); R.ay = ss_axis(g.H); R.az = ss_axis(g.W);
  }

  if (!FAST && slice == 0 && tid < r.head) dx[tid] = ss_grad(x[tid], ss_decompose(tid, g), R, kk) + (tid == R.arg ? R.gm : 0.f);
  if (!FAST && slice == g.slices - 1 && tid < r.tail) {
    const uint32_t i = r.head + 4u * r.nvec + tid;
    dx[i] = ss_grad(x[i], ss_decompose(i, g), R, kk) + (i == R.arg ? R.gm : 0.f);
  }

  const ssf4* xv = reinterpret_cast<const ssf4*>(x + r.head);
  ssf4* dv = reinterpret_cast<ssf4*>(dx + r.head);
  uint32_t t = r.v0 + tid;
  if (t >= r.v1) return;
  SsPos pos = ss_decompose(r.head + 4u * t, g);
  for (; t < r.v1; t += SS_THREADS * SS_UNROLL) {
    ssf4 v[SS_UNROLL];
#pragma unroll
    for (int k = 0; k < SS_UNROLL; ++k) {
      const uint32_t tk = t + k * SS_THREADS;
      v[k] = tk < r.v1 ? xv[tk] : (ssf4)(0.f);
    }
#pragma unroll
    for (int k = 0; k < SS_UNROLL; ++k) {
      const uint32_t tk = t + k * SS_THREADS;
      ssf4 o;
      if (FAST) {
        const float wab = fmaf(R.gy, ss_coord(pos.a, R.ay) - R.ey, R.gx * (ss_coord(pos.b, R.ax) - R.ex));
        const float c2 = 2.f * (float)pos.c - R.az.off;
        const float w0 = fmaf(R.gz, fmaf(c2, R.az.scale, R.az.bias) - R.ez, wab);
        const float w1 = fmaf(R.gz, fmaf(c2 + 2.f, R.az.scale, R.az.bias) - R.ez, wab);
        const float w2 = fmaf(R.gz, fmaf(c2 + 4.f, R.az.scale, R.az.bias) - R.ez, wab);
        const float w3 = fmaf(R.gz, fmaf(c2 + 6.f, R.az.scale, R.az.bias) - R.ez, wab);
        o.x = ss_exp2((v[k].x - R.m) * kk) * R.ps * w0;
        o.y = ss_exp2((v[k].y - R.m) * kk) * R.ps * w1;
        o.z = ss_exp2((v[k].z - R.m) * kk) * R.ps * w2;
        o.w = ss_exp2((v[k].w - R.m) * kk) * R.ps * w3;
      } else {
        SsPos q = pos;
        o.x = ss_grad(v[k].x, q, R, kk); ss_step(q, g);
        o.y = ss_grad(v[k].y, q, R, kk); ss_step(q, g);
        o.z = ss_grad(v[k].z, q, R, kk); ss_step(q, g);
        o.w = ss_grad(v[k].w, q, R, kk);
      }
      const uint32_t rel = R.arg - (r.head + 4u * tk);  // the max-pool's gradient goes to the first maximum alone
      if (rel < 4u) {
        o.x += rel == 0 ? R.gm : 0.f;
        o.y += rel == 1 ? R.gm : 0.f;
        o.z += rel == 2 ? R.gm : 0.f;
        o.w += rel == 3 ? R.gm : 0.f;
      }
      if (tk < r.v1) dv[tk] = o;
      ss_advance(pos, g);
    }
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
static int ss_auto_slices(int64_t rows, int64_t N) {
  int64_t s = (SS_TARGET_BLOCKS + rows - 1) / rows;
  const int64_t by_length = (N / 4) / SS_MIN_SLICE_VEC;
  if (s > by_length) s = by_length;
  if (s > SS_MAX_SLICES) s = SS_MAX_SLICES;
  return s < 1 ? 1 : (int)s;
}

// sizes, temperature and the split, common to forward and backward -> g
static int ss_check(const char* fn, int64_t rows, int C, int D, int H, int W, float temperature, int slices, SsGeom* g) {
  if (rows < 1 || C < 1 || D < 1 || H < 1 || W < 1) {
    set_error("%s: rows = %lld, C = %d, D = %d, H = %d, W = %d (each >= 1)", fn, (long long)rows, C, D, H, W);
    return MGS_ERR_INVALID_ARG;
  }
  if (rows % C != 0) { set_error("%s: rows = %lld is no multiple of C = %d", fn, (long long)rows, C); return MGS_ERR_INVALID_ARG; }
  const int64_t N = (int64_t)D * H * W;
  if ((int64_t)D * H > 0x7fffffff || N > 0x7fffffff) {
    set_error("%s: D H W = %d x %d x %d exceeds 2^31 - 1 elements per row", fn, D, H, W);
    return MGS_ERR_INVALID_ARG;
  }
  if (rows * SS_MAX_SLICES > 0x7fffffff) {
    set_error("%s: rows = %lld (at most %d)", fn, (long long)rows, 0x7fffffff / SS_MAX_SLICES);
    return MGS_ERR_INVALID_ARG;
  }
  const double kk = 1.4426950408889634 / (double)temperature;
  if (!(temperature > 0.f) || !isfinite(temperature) || !(kk <= (double)FLT_MAX)) {
    set_error("%s: temperature = %g (must be positive and finite)", fn, (double)temperature);
    return MGS_ERR_INVALID_ARG;
  }
  if (slices < 0 || slices > SS_MAX_SLICES) {
    set_error("%s: slices = %d (0: chosen by the library, at most %d)", fn, slices, SS_MAX_SLICES);
    return MGS_ERR_INVALID_ARG;
  }
  g->N = (uint32_t)N; g->D = (uint32_t)D; g->H = (uint32_t)H; g->W = (uint32_t)W; g->DW = (uint32_t)((int64_t)D * W);
  const uint32_t stride = SS_STRIDE;
  g->qa = stride / g->DW;
  g->qb = (stride - g->qa * g->DW) / g->W;
  g->qc = stride - g->qa * g->DW - g->qb * g->W;
  g->C = (uint32_t)C;
  g->slices = (uint32_t)(slices ? slices : ss_auto_slices(rows, N));
  g->kk = (float)kk;
  g->inv_t = (float)(1.0 / (double)temperature);
  return MGS_OK;
}

}  // namespace mgs

using namespace mgs;

extern "C" {

size_t mgs_spatial_softmax_workspace_bytes(int64_t rows, int64_t N) {
  if (rows < 1 || N < 1 || N > 0x7fffffff || rows * SS_MAX_SLICES > 0x7fffffff) return 0;
  return align_up((size_t)rows * SS_MAX_SLICES * SS_REC * sizeof(float)) + ALIGN;  // one record per slice, any split
}

int mgs_spatial_softmax_forward(int64_t rows, int C, int D, int H, int W, float temperature, const float* feature,
                                float* keypoints, int64_t keypoints_stride_b, float* maxpool, int64_t maxpool_stride_b,
                                float* stats, void* workspace, size_t workspace_bytes, int slices, mgs_stream_t stream) {
  const char* fn = "spatial_softmax_forward";
  SsGeom g;
  int rc = ss_check(fn, rows, C, D, H, W, temperature, slices, &g);
  if (rc != MGS_OK) return rc;
  if (!feature || !keypoints || !stats || !workspace) {
    set_error("%s: NULL feature, keypoints, stats or workspace", fn);
    return MGS_ERR_INVALID_ARG;
  }
  if (misaligned16(feature) || misaligned16(workspace)) {
    set_error("%s: feature and the workspace must be 16-byte aligned", fn);
    return MGS_ERR_INVALID_ARG;
  }
  if (keypoints_stride_b < 3 * (int64_t)C || (maxpool && maxpool_stride_b < C)) {
    set_error("%s: row strides of keypoints (%lld: at least %d) and maxpool (%lld: at least %d)", fn,
              (long long)keypoints_stride_b, 3 * C, (long long)maxpool_stride_b, C);
    return MGS_ERR_INVALID_ARG;
  }
  const size_t need = mgs_spatial_softmax_workspace_bytes(rows, g.N);
  if (int rc = workspace_short(fn, workspace_bytes, need)) return rc;
  hipStream_t s = (hipStream_t)stream;
  float* records = reinterpret_cast<float*>(workspace);
  const dim3 grid((unsigned)(rows * g.slices));
  if (g.W % 4 == 0) hipLaunchKernelGGL((ss_fwd_kernel<true>), grid, dim3(SS_THREADS), 0, s, g, feature, records);
  else hipLaunchKernelGGL((ss_fwd_kernel<false>), grid, dim3(SS_THREADS), 0, s, g, feature, records);
  hipLaunchKernelGGL(ss_combine_kernel, dim3((unsigned)((rows + SS_THREADS - 1) / SS_THREADS)), dim3(SS_THREADS), 0, s, g,
                     (uint32_t)rows, records, keypoints, keypoints_stride_b, maxpool, maxpool_stride_b, stats);
  return launch_done(fn);
}

int mgs_spatial_softmax_backward(int64_t rows, int C, int D, int H, int W, float temperature, const float* feature,
                                 const float* stats, const float* g_keypoints, int64_t g_keypoints_stride_b, const float* g_max,
                                 int64_t g_max_stride_b, float* g_feature, int slices, mgs_stream_t stream) {
  const char* fn = "spatial_softmax_backward";
  SsGeom g;
  int rc = ss_check(fn, rows, C, D, H, W, temperature, slices, &g);
  if (rc != MGS_OK) return rc;
  if (!feature || !stats || !g_feature) { set_error("%s: NULL feature, stats or g_feature", fn); return MGS_ERR_INVALID_ARG; }
  if (misaligned16(feature) || misaligned16(g_feature)) {
    set_error("%s: feature and g_feature must be 16-byte aligned", fn);
    return MGS_ERR_INVALID_ARG;
  }
  if ((g_keypoints && g_keypoints_stride_b < 3 * (int64_t)C) || (g_max && g_max_stride_b < C)) {
    set_error("%s: row strides of g_keypoints (%lld: at least %d) and g_max (%lld: at least %d)", fn,
              (long long)g_keypoints_stride_b, 3 * C, (long long)g_max_stride_b, C);
    return MGS_ERR_INVALID_ARG;
  }
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)(rows * g.slices));
  if (g.W % 4 == 0)
    hipLaunchKernelGGL((ss_bwd_kernel<true>), grid, dim3(SS_THREADS), 0, s, g, feature, stats, g_keypoints, g_keypoints_stride_b,
                       g_max, g_max_stride_b, g_feature);
  else
    hipLaunchKernelGGL((ss_bwd_kernel<false>), grid, dim3(SS_THREADS), 0, s, g, feature, stats, g_keypoints, g_keypoints_stride_b,
                       g_max, g_max_stride_b, g_feature);
  return launch_done(fn);
}

}  // extern "C"
