// mgs_abn.hip -- the voxel encoder stem's InPlaceABN (helpers/network_utils.py:219-231: nn.BatchNorm3d in training mode followed
// by an in-place nn.LeakyReLU) and the residual add that follows three of its ten uses (:297-303), fused, fp32, forward and
// backward.  A row is one (batch, channel): N = D H W floats at element row * N of a [B, C, N] volume.
//
//   z = (x - mean_c) * invstd_c * w_c + b_c;   y = residual + (z > 0 ? z : slope * z)
//
// Statistics.  A row is cut into `nsub` SUB-SLICES of whole 16-byte vectors; nsub depends on N alone.  A sub-slice is reduced by one
// 256-thread workgroup to a (count, mean, M2) record: a lane folds register tiles of 16 values (tile mean, then the centred squares,
// then Chan's merge into its running triple), lanes, waves and sub-slices are merged with Chan's formula in an order fixed by the
// geometry.  `slices` only says how many workgroups share a row's sub-slices, so the records, and everything computed from them, are
// the same bits for every slice count.  The variance never goes through sum(x^2) - sum(x)^2.
//
// Forward, training: abn_stats_kernel writes the records; abn_apply_kernel merges a channel's B * nsub records (in double, one record
// per thread, then a fixed tree in LDS), normalises, activates, adds the skip tensor and writes y.  The workgroup of (batch 0, slice 0)
// of a channel also writes the two floats the backward keeps (mean, invstd), updates running_mean / running_var in place (unbiased
// variance) and, for channel 0, increments num_batches_tracked.  Eval: the apply launch alone, from the running buffers.
// Backward: abn_bwd_sums_kernel writes one (sum dz, sum dz xhat) record per sub-slice, dz = g * act'(z) with z recomputed by the
// forward's own expression (abn_z); abn_bwd_dx_kernel merges them the same way and writes dx, and dweight / dbias from the merged sums.
//
// No atomics, no workgroup waits for another, nothing to zero.  Rows start at element row * N of 16-byte aligned volumes, so for
// N % 4 != 0 a row's first (-row N) & 3 elements (the head) and the ones behind its whole vectors (the tail) are read and written as
// scalars; vector accesses are always aligned.  Element offsets are 64-bit; indices inside a row are 32-bit unsigned (N <= 2^31 - 1).
#include <math.h>

#include "mgs_common.h"

namespace mgs {

constexpr int ABN_THREADS = 256;
constexpr int ABN_UNROLL = 4;              // 16-byte loads per tensor a lane has in flight
constexpr int ABN_MAX_SUBS = 64;           // most sub-slices (records) per row, and most workgroups per row
constexpr int ABN_TARGET_BLOCKS = 2048;    // 256 CUs x 8 workgroups of 4 waves
constexpr int ABN_MIN_SUB_VEC = 512;       // a sub-slice is not cut below 2 vectors per lane
constexpr int ABN_MAX_C = 65536;
constexpr int ABN_REC = 4;                 // floats per record: count (bits of a uint32), mean, M2, unused | sum dz, sum dz xhat, unused x 2

typedef float abnf4 __attribute__((ext_vector_type(4)));

struct AbnGeom {
  uint32_t N, C, B;
  uint32_t nsub;     // sub-slices per row: a function of N alone
  uint32_t slices;   // workgroups per row, <= nsub
  float slope;
};

// the split of a row, the same in every kernel
struct AbnRow {
  int64_t start;     // element offset of the row in the volume
  uint32_t head, nvec, tail, per;   // per: vectors per sub-slice
  uint32_t s0, s1;   // this workgroup's sub-slices
};
__device__ __forceinline__ AbnRow abn_row(uint32_t row, uint32_t slice, const AbnGeom& g) {
  AbnRow r;
  r.start = (int64_t)row * (int64_t)g.N;
  r.head = min((uint32_t)((-r.start) & 3), g.N);
  r.nvec = (g.N - r.head) >> 2;
  r.tail = g.N - r.head - 4u * r.nvec;
  r.per = (r.nvec + g.nsub - 1) / g.nsub;
  const uint32_t spw = (g.nsub + g.slices - 1) / g.slices;
  r.s0 = min(slice * spw, g.nsub);
  r.s1 = min(r.s0 + spw, g.nsub);
  return r;
}
__device__ __forceinline__ uint32_t abn_sub_begin(const AbnRow& r, uint32_t sub) { return min(sub * r.per, r.nvec); }

// the activation's argument: ONE expression for the forward and for the backward's recomputation (both take the same side of 0)
__device__ __forceinline__ float abn_z(float x, float mean, float scale, float shift) { return fmaf(x - mean, scale, shift); }
__device__ __forceinline__ float abn_act(float z, float slope) { return z > 0.f ? z : z * slope; }
__device__ __forceinline__ float abn_dz(float z, float gy, float slope) { return z > 0.f ? gy : gy * slope; }

// ---- moments -------------------------------------------------------------------------------------------------------------------
struct AbnMom {
  uint32_t n;
  float mean, m2;
};

// Chan's merge; an empty side leaves the other's bits untouched
__device__ __forceinline__ AbnMom abn_merge(const AbnMom& a, const AbnMom& b) {
#pragma clang fp contract(off)
  AbnMom r;
  r.n = a.n + b.n;
  const float rb = (float)b.n / (float)max(r.n, 1u);
  const float d = b.mean - a.mean;
  r.mean = a.mean + d * rb;
  r.m2 = (a.m2 + b.m2) + (d * d) * ((float)a.n * rb);
  if (b.n == 0) r = a;
  if (a.n == 0) r = b;
  return r;
}

// K values into a lane's triple: their mean first, then the squares about it (the error of that mean enters squared only)
template <int K>
__device__ __forceinline__ void abn_push(AbnMom& p, const float (&v)[K]) {
#pragma clang fp contract(off)
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) s += v[k];
  const float mt = s * (1.f / (float)K);
  float q = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float e = v[k] - mt;
    q += e * e;
  }
  const float rb = p.n == 0 ? 1.f : (float)K * __builtin_amdgcn_rcpf((float)(p.n + K));
  const float d = mt - p.mean;
  p.m2 = (p.m2 + q) + (d * d) * ((float)p.n * rb);
  p.mean = p.mean + d * rb;
  p.n += K;
}

__global__ __launch_bounds__(ABN_THREADS) void abn_stats_kernel(AbnGeom g, const float* __restrict__ x, float* __restrict__ records) {
  const uint32_t row = blockIdx.x / g.slices, slice = blockIdx.x - row * g.slices;
  const uint32_t tid = threadIdx.x;
  const AbnRow r = abn_row(row, slice, g);
  const float* xr = x + r.start;
  const abnf4* xv = reinterpret_cast<const abnf4*>(xr + r.head);
  __shared__ AbnMom wave_mom[ABN_THREADS / 64];

  for (uint32_t sub = r.s0; sub < r.s1; ++sub) {
    const uint32_t v0 = abn_sub_begin(r, sub), v1 = min(v0 + r.per, r.nvec);
    AbnMom p;
    p.n = 0; p.mean = 0.f; p.m2 = 0.f;
    uint32_t t = v0 + tid;
    for (; t + (ABN_UNROLL - 1) * ABN_THREADS < v1; t += ABN_UNROLL * ABN_THREADS) {
      abnf4 q[ABN_UNROLL];
#pragma unroll
      for (int k = 0; k < ABN_UNROLL; ++k) q[k] = xv[t + k * ABN_THREADS];
      float v[4 * ABN_UNROLL];
#pragma unroll
      for (int k = 0; k < ABN_UNROLL; ++k) { v[4 * k] = q[k].x; v[4 * k + 1] = q[k].y; v[4 * k + 2] = q[k].z; v[4 * k + 3] = q[k].w; }
      abn_push<4 * ABN_UNROLL>(p, v);
    }
    for (; t < v1; t += ABN_THREADS) {
      const abnf4 q = xv[t];
      const float v[4] = {q.x, q.y, q.z, q.w};
      abn_push<4>(p, v);
    }
    if (sub == 0 && tid < r.head) {
      const float v[1] = {xr[tid]};
      abn_push<1>(p, v);
    }
    if (sub == g.nsub - 1 && tid < r.tail) {
      const float v[1] = {xr[r.head + 4u * r.nvec + tid]};
      abn_push<1>(p, v);
    }
    // lanes of a wave (lane 0 gathers 0..63 in a fixed tree), then the four waves in order
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      AbnMom o;
      o.n = __shfl_down(p.n, d); o.mean = __shfl_down(p.mean, d); o.m2 = __shfl_down(p.m2, d);
      p = abn_merge(p, o);
    }
    if ((tid & 63u) == 0) wave_mom[tid >> 6] = p;
    __syncthreads();
    if (tid == 0) {
      p = wave_mom[0];
#pragma unroll
      for (int w = 1; w < ABN_THREADS / 64; ++w) p = abn_merge(p, wave_mom[w]);
      abnf4 rec;
      rec.x = __uint_as_float(p.n); rec.y = p.mean; rec.z = p.m2; rec.w = 0.f;
      *reinterpret_cast<abnf4*>(records + ((size_t)row * g.nsub + sub) * ABN_REC) = rec;
    }
    __syncthreads();
  }
}

// Channel c's B * nsub records -> (a, b) on every thread.  MOMENTS: (mean, M2) by Chan's merge; else: the two plain sums.  In double:
// thread t takes records t, t + 256, .. in ascending order, then a fixed tree over the threads.
template <bool MOMENTS>
__device__ __forceinline__ void abn_channel_merge(const AbnGeom& g, uint32_t c, const float* __restrict__ records, double& out_a,
                                                  double& out_b) {
  __shared__ double sh_n[ABN_THREADS], sh_a[ABN_THREADS], sh_b[ABN_THREADS];
  const uint32_t tid = threadIdx.x;
  const uint32_t R = g.B * g.nsub;
  double n = 0.0, a = 0.0, b = 0.0;
  auto fold = [](double& n, double& a, double& b, double n2, double a2, double b2) {
    if (MOMENTS) {
      if (n2 == 0.0) return;
      if (n == 0.0) { n = n2; a = a2; b = b2; return; }
      const double nn = n + n2, d = a2 - a, rb = n2 / nn;
      a += d * rb;
      b += b2 + d * d * n * rb;
      n = nn;
    } else {
      a += a2;
      b += b2;
    }
  };
  for (uint32_t i = tid; i < R; i += ABN_THREADS) {
    const uint32_t bi = i / g.nsub, j = i - bi * g.nsub;
    const abnf4 rec = *reinterpret_cast<const abnf4*>(records + (((size_t)bi * g.C + c) * g.nsub + j) * ABN_REC);
    if (MOMENTS) fold(n, a, b, (double)__float_as_uint(rec.x), (double)rec.y, (double)rec.z);
    else fold(n, a, b, 0.0, (double)rec.x, (double)rec.y);
  }
  sh_n[tid] = n; sh_a[tid] = a; sh_b[tid] = b;
  for (uint32_t d = ABN_THREADS / 2; d >= 1; d >>= 1) {
    __syncthreads();
    if (tid < d) {
      fold(n, a, b, sh_n[tid + d], sh_a[tid + d], sh_b[tid + d]);
      sh_n[tid] = n; sh_a[tid] = a; sh_b[tid] = b;
    }
  }
  __syncthreads();
  out_a = sh_a[0];
  out_b = sh_b[0];
}

// ---- forward: normalise, activate, add ---------------------------------------------------------------------------------------------
struct AbnFwdArgs {
  const float *x, *residual, *weight, *bias, *records;
  float *running_mean, *running_var, *stats, *y;
  long long* num_batches_tracked;
  int training;
  float momentum, eps;
};

template <bool RES>
__global__ __launch_bounds__(ABN_THREADS) void abn_apply_kernel(AbnGeom g, AbnFwdArgs a) {
  const uint32_t row = blockIdx.x / g.slices, slice = blockIdx.x - row * g.slices;
  const uint32_t tid = threadIdx.x;
  const uint32_t b = row / g.C, c = row - b * g.C;
  const AbnRow r = abn_row(row, slice, g);

  float mean, invstd;
  if (a.training) {
    double dmean, dm2;
    abn_channel_merge<true>(g, c, a.records, dmean, dm2);
    const double n = (double)g.B * (double)g.N;
    mean = (float)dmean;
    invstd = (float)(1.0 / sqrt(dm2 / n + (double)a.eps));
    double rmean = dmean;
    if (b == 0 && slice == 0 && a.running_mean && dmean != dmean) {   // (uniform across the workgroup, and rare)
      // A merged mean is NaN for a channel that holds an infinity (inf - inf between two parts) where the plain mean the reference
      // takes is that infinity.  Everything computed FROM the mean is NaN either way; the running mean is not.  The workgroup looks.
      int seen = 0;
      for (uint32_t bb = 0; bb < g.B; ++bb) {
        const float* xc = a.x + ((int64_t)bb * g.C + c) * (int64_t)g.N;
        for (uint32_t i = tid; i < g.N; i += ABN_THREADS) {
          const float v = xc[i];
          seen |= v != v ? 4 : (v == INFINITY ? 1 : (v == -INFINITY ? 2 : 0));
        }
      }
      const int pos = __syncthreads_or(seen & 1), neg = __syncthreads_or(seen & 2), nan = __syncthreads_or(seen & 4);
      if (!nan && (pos != 0) != (neg != 0)) rmean = pos ? (double)INFINITY : -(double)INFINITY;
    }
    if (b == 0 && slice == 0 && tid == 0) {   // once per channel
      a.stats[2 * c] = mean;
      a.stats[2 * c + 1] = invstd;
      if (a.running_mean) {
        const double m = (double)a.momentum;
        a.running_mean[c] = (float)((1.0 - m) * (double)a.running_mean[c] + m * rmean);
        a.running_var[c] = (float)((1.0 - m) * (double)a.running_var[c] + m * (dm2 / (n - 1.0)));
      }
      if (a.num_batches_tracked && c == 0) a.num_batches_tracked[0] += 1;
    }
  } else {
    mean = a.running_mean[c];
    invstd = 1.f / sqrtf(a.running_var[c] + a.eps);
  }
  const float scale = invstd * a.weight[c], shift = a.bias[c], slope = g.slope;

  const float* xr = a.x + r.start;
  const float* rr = RES ? a.residual + r.start : nullptr;
  float* yr = a.y + r.start;
  if (r.s0 == 0 && r.s0 < r.s1 && tid < r.head) {
    const float v = abn_act(abn_z(xr[tid], mean, scale, shift), slope);
    yr[tid] = RES ? rr[tid] + v : v;
  }
  if (r.s1 == g.nsub && r.s0 < r.s1 && tid < r.tail) {
    const uint32_t i = r.head + 4u * r.nvec + tid;
    const float v = abn_act(abn_z(xr[i], mean, scale, shift), slope);
    yr[i] = RES ? rr[i] + v : v;
  }
  const abnf4* xv = reinterpret_cast<const abnf4*>(xr + r.head);
  const abnf4* rv = RES ? reinterpret_cast<const abnf4*>(rr + r.head) : nullptr;
  abnf4* yv = reinterpret_cast<abnf4*>(yr + r.head);
  const uint32_t v0 = abn_sub_begin(r, r.s0), v1 = abn_sub_begin(r, r.s1);
  for (uint32_t t = v0 + tid; t < v1; t += ABN_THREADS * ABN_UNROLL) {
    abnf4 q[ABN_UNROLL], s[ABN_UNROLL];
#pragma unroll
    for (int k = 0; k < ABN_UNROLL; ++k) {
      const uint32_t tk = t + k * ABN_THREADS;
      q[k] = tk < v1 ? xv[tk] : (abnf4)(0.f);
      if (RES) s[k] = tk < v1 ? rv[tk] : (abnf4)(0.f);
    }
#pragma unroll
    for (int k = 0; k < ABN_UNROLL; ++k) {
      const uint32_t tk = t + k * ABN_THREADS;
      abnf4 o;
      o.x = abn_act(abn_z(q[k].x, mean, scale, shift), slope);
      o.y = abn_act(abn_z(q[k].y, mean, scale, shift), slope);
      o.z = abn_act(abn_z(q[k].z, mean, scale, shift), slope);
      o.w = abn_act(abn_z(q[k].w, mean, scale, shift), slope);
      if (RES) o += s[k];
      if (tk < v1) yv[tk] = o;
    }
  }
}

// ---- backward ------------------------------------------------------------------------------------------------------------------
struct AbnBwdArgs {
  const float *x, *gy, *weight, *bias, *stats;
  float *records, *dx, *dweight, *dbias;
};

__device__ __forceinline__ void abn_bwd_term(float x, float gy, float mean, float invstd, float scale, float shift, float slope, float& s1,
                                             float& s2) {
  const float dz = abn_dz(abn_z(x, mean, scale, shift), gy, slope);
  s1 += dz;
  s2 = fmaf(dz, (x - mean) * invstd, s2);
}

__global__ __launch_bounds__(ABN_THREADS) void abn_bwd_sums_kernel(AbnGeom g, AbnBwdArgs a) {
  const uint32_t row = blockIdx.x / g.slices, slice = blockIdx.x - row * g.slices;
  const uint32_t tid = threadIdx.x;
  const uint32_t c = row % g.C;
  const AbnRow r = abn_row(row, slice, g);
  const float mean = a.stats[2 * c], invstd = a.stats[2 * c + 1];
  const float scale = invstd * a.weight[c], shift = a.bias[c], slope = g.slope;
  const float* xr = a.x + r.start;
  const float* gr = a.gy + r.start;
  const abnf4* xv = reinterpret_cast<const abnf4*>(xr + r.head);
  const abnf4* gv = reinterpret_cast<const abnf4*>(gr + r.head);
  __shared__ float wave_sum[ABN_THREADS / 64][2];

  for (uint32_t sub = r.s0; sub < r.s1; ++sub) {
    const uint32_t v0 = abn_sub_begin(r, sub), v1 = min(v0 + r.per, r.nvec);
    float s1 = 0.f, s2 = 0.f;
    for (uint32_t t = v0 + tid; t < v1; t += ABN_THREADS * ABN_UNROLL) {
      abnf4 q[ABN_UNROLL], u[ABN_UNROLL];
#pragma unroll
      for (int k = 0; k < ABN_UNROLL; ++k) {
        const uint32_t tk = t + k * ABN_THREADS;
        q[k] = tk < v1 ? xv[tk] : (abnf4)(0.f);
        u[k] = tk < v1 ? gv[tk] : (abnf4)(0.f);   // (an absent vector adds dz = 0)
      }
#pragma unroll
      for (int k = 0; k < ABN_UNROLL; ++k) {
        abn_bwd_term(q[k].x, u[k].x, mean, invstd, scale, shift, slope, s1, s2);
        abn_bwd_term(q[k].y, u[k].y, mean, invstd, scale, shift, slope, s1, s2);
        abn_bwd_term(q[k].z, u[k].z, mean, invstd, scale, shift, slope, s1, s2);
        abn_bwd_term(q[k].w, u[k].w, mean, invstd, scale, shift, slope, s1, s2);
      }
    }
    if (sub == 0 && tid < r.head) abn_bwd_term(xr[tid], gr[tid], mean, invstd, scale, shift, slope, s1, s2);
    if (sub == g.nsub - 1 && tid < r.tail) {
      const uint32_t i = r.head + 4u * r.nvec + tid;
      abn_bwd_term(xr[i], gr[i], mean, invstd, scale, shift, slope, s1, s2);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      s1 += __shfl_down(s1, d);
      s2 += __shfl_down(s2, d);
    }
    if ((tid & 63u) == 0) { wave_sum[tid >> 6][0] = s1; wave_sum[tid >> 6][1] = s2; }
    __syncthreads();
    if (tid == 0) {
      abnf4 rec;
      rec.x = (wave_sum[0][0] + wave_sum[1][0]) + (wave_sum[2][0] + wave_sum[3][0]);
      rec.y = (wave_sum[0][1] + wave_sum[1][1]) + (wave_sum[2][1] + wave_sum[3][1]);
      rec.z = 0.f; rec.w = 0.f;
      *reinterpret_cast<abnf4*>(a.records + ((size_t)row * g.nsub + sub) * ABN_REC) = rec;
    }
    __syncthreads();
  }
}

__device__ __forceinline__ float abn_dx(float x, float gy, float mean, float invstd, float scale, float shift, float slope, float c1,
                                        float c2) {
  const float dz = abn_dz(abn_z(x, mean, scale, shift), gy, slope);
  return scale * fmaf(-((x - mean) * invstd), c2, dz - c1);
}

__global__ __launch_bounds__(ABN_THREADS) void abn_bwd_dx_kernel(AbnGeom g, AbnBwdArgs a) {
  const uint32_t row = blockIdx.x / g.slices, slice = blockIdx.x - row * g.slices;
  const uint32_t tid = threadIdx.x;
  const uint32_t b = row / g.C, c = row - b * g.C;
  const AbnRow r = abn_row(row, slice, g);
  double sum_dz, sum_dzx;
  abn_channel_merge<false>(g, c, a.records, sum_dz, sum_dzx);
  const double n = (double)g.B * (double)g.N;
  const float c1 = (float)(sum_dz / n), c2 = (float)(sum_dzx / n);
  if (b == 0 && slice == 0 && tid == 0) {
    if (a.dweight) a.dweight[c] = (float)sum_dzx;
    if (a.dbias) a.dbias[c] = (float)sum_dz;
  }
  const float mean = a.stats[2 * c], invstd = a.stats[2 * c + 1];
  const float scale = invstd * a.weight[c], shift = a.bias[c], slope = g.slope;
  const float* xr = a.x + r.start;
  const float* gr = a.gy + r.start;
  float* dr = a.dx + r.start;
  if (r.s0 == 0 && r.s0 < r.s1 && tid < r.head) dr[tid] = abn_dx(xr[tid], gr[tid], mean, invstd, scale, shift, slope, c1, c2);
  if (r.s1 == g.nsub && r.s0 < r.s1 && tid < r.tail) {
    const uint32_t i = r.head + 4u * r.nvec + tid;
    dr[i] = abn_dx(xr[i], gr[i], mean, invstd, scale, shift, slope, c1, c2);
  }
  const abnf4* xv = reinterpret_cast<const abnf4*>(xr + r.head);
  const abnf4* gv = reinterpret_cast<const abnf4*>(gr + r.head);
  abnf4* dv = reinterpret_cast<abnf4*>(dr + r.head);
  const uint32_t v0 = abn_sub_begin(r, r.s0), v1 = abn_sub_begin(r, r.s1);
  for (uint32_t t = v0 + tid; t < v1; t += ABN_THREADS * ABN_UNROLL) {
    abnf4 q[ABN_UNROLL], u[ABN_UNROLL];
#pragma unroll
    for (int k = 0; k < ABN_UNROLL; ++k) {
      const uint32_t tk = t + k * ABN_THREADS;
      q[k] = tk < v1 ? xv[tk] : (abnf4)(0.f);
      u[k] = tk < v1 ? gv[tk] : (abnf4)(0.f);
    }
#pragma unroll
    for (int k = 0; k < ABN_UNROLL; ++k) {
      const uint32_t tk = t + k * ABN_THREADS;
      abnf4 o;
      o.x = abn_dx(q[k].x, u[k].x, mean, invstd, scale, shift, slope, c1, c2);
      o.y = abn_dx(q[k].y, u[k].y, mean, invstd, scale, shift, slope, c1, c2);
      o.z = abn_dx(q[k].z, u[k].z, mean, invstd, scale, shift, slope, c1, c2);
      o.w = abn_dx(q[k].w, u[k].w, mean, invstd, scale, shift, slope, c1, c2);
      if (tk < v1) dv[tk] = o;
    }
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
static bool abn_shape_ok(int64_t B, int64_t C, int64_t N) {
  return B >= 1 && C >= 1 && C <= ABN_MAX_C && N >= 1 && N <= 0x7fffffff && B <= 0x7fffffff / ABN_MAX_SUBS / C;
}

// sizes, the slope and the split, common to forward and backward -> g
static int abn_check(const char* fn, int64_t B, int C, int64_t N, float slope, int slices, AbnGeom* g) {
  if (C < 1 || C > ABN_MAX_C) { set_error("%s: C = %d (1 to %d)", fn, C, ABN_MAX_C); return MGS_ERR_INVALID_ARG; }
  if (B < 1 || N < 1) { set_error("%s: B = %lld, N = %lld (each >= 1)", fn, (long long)B, (long long)N); return MGS_ERR_INVALID_ARG; }
  if (N > 0x7fffffff) { set_error("%s: N = %lld exceeds 2^31 - 1 elements per row", fn, (long long)N); return MGS_ERR_INVALID_ARG; }
  if (!abn_shape_ok(B, C, N)) {
    set_error("%s: B C = %lld x %d rows (at most %d)", fn, (long long)B, C, 0x7fffffff / ABN_MAX_SUBS);
    return MGS_ERR_INVALID_ARG;
  }
  if (!isfinite(slope)) { set_error("%s: negative_slope = %g (must be finite)", fn, (double)slope); return MGS_ERR_INVALID_ARG; }
  if (slices < 0 || slices > ABN_MAX_SUBS) {
    set_error("%s: slices = %d (0: chosen by the library, at most %d)", fn, slices, ABN_MAX_SUBS);
    return MGS_ERR_INVALID_ARG;
  }
  const int64_t rows = B * C;
  int64_t nsub = (N / 4) / ABN_MIN_SUB_VEC;
  nsub = nsub < 1 ? 1 : (nsub > ABN_MAX_SUBS ? ABN_MAX_SUBS : nsub);
  int64_t s = slices ? slices : (ABN_TARGET_BLOCKS + rows - 1) / rows;
  s = s < 1 ? 1 : (s > nsub ? nsub : s);
  g->N = (uint32_t)N; g->C = (uint32_t)C; g->B = (uint32_t)B;
  g->nsub = (uint32_t)nsub; g->slices = (uint32_t)s;
  g->slope = slope;
  return MGS_OK;
}

}  // namespace mgs

using namespace mgs;

extern "C" {

size_t mgs_abn_workspace_bytes(int64_t B, int C, int64_t N) {
  if (!abn_shape_ok(B, C, N)) return 0;
  return align_up((size_t)B * (size_t)C * ABN_MAX_SUBS * ABN_REC * sizeof(float)) + ALIGN;  // one record per sub-slice, any N
}

int mgs_abn_forward(int64_t B, int C, int64_t N, const float* x, const float* residual, const float* weight, const float* bias,
                    float* running_mean, float* running_var, int64_t* num_batches_tracked, int training, float momentum, float eps,
                    float negative_slope, float* y, float* stats, void* workspace, size_t workspace_bytes, int slices,
                    mgs_stream_t stream) {
  const char* fn = "abn_forward";
  AbnGeom g;
  int rc = abn_check(fn, B, C, N, negative_slope, slices, &g);
  if (rc != MGS_OK) return rc;
  if (!isfinite(eps) || !(eps >= 0.f)) { set_error("%s: eps = %g (must be finite and not negative)", fn, (double)eps); return MGS_ERR_INVALID_ARG; }
  if (!isfinite(momentum)) { set_error("%s: momentum = %g (must be finite)", fn, (double)momentum); return MGS_ERR_INVALID_ARG; }
  if (!x || !weight || !bias || !y) { set_error("%s: NULL x, weight, bias or y", fn); return MGS_ERR_INVALID_ARG; }
  if ((running_mean == nullptr) != (running_var == nullptr)) {
    set_error("%s: NULL running_mean or running_var (both, or neither in training mode)", fn);
    return MGS_ERR_INVALID_ARG;
  }
  if (training) {
    if (!stats || !workspace) { set_error("%s: NULL stats or workspace in training mode", fn); return MGS_ERR_INVALID_ARG; }
    if (B * N < 2) {
      set_error("%s: Expected more than 1 value per channel when training (B = %lld, N = %lld)", fn, (long long)B, (long long)N);
      return MGS_ERR_INVALID_ARG;
    }
  } else if (!running_mean) {
    set_error("%s: NULL running_mean and running_var in eval mode", fn);
    return MGS_ERR_INVALID_ARG;
  }
  if (misaligned16(x) || misaligned16(y) || (residual && misaligned16(residual)) || (training && misaligned16(workspace))) {
    set_error("%s: x, residual, y and the workspace must be 16-byte aligned", fn);
    return MGS_ERR_INVALID_ARG;
  }
  if (training) {
    if (int rc = workspace_short(fn, workspace_bytes, mgs_abn_workspace_bytes(B, C, N))) return rc;
  }
  hipStream_t s = (hipStream_t)stream;
  AbnFwdArgs a;
  a.x = x; a.residual = residual; a.weight = weight; a.bias = bias; a.records = reinterpret_cast<const float*>(workspace);
  a.running_mean = running_mean; a.running_var = running_var; a.stats = stats; a.y = y;
  a.num_batches_tracked = reinterpret_cast<long long*>(num_batches_tracked);
  a.training = training ? 1 : 0; a.momentum = momentum; a.eps = eps;
  const dim3 grid((unsigned)(B * C * g.slices));
  if (training) hipLaunchKernelGGL(abn_stats_kernel, grid, dim3(ABN_THREADS), 0, s, g, x, reinterpret_cast<float*>(workspace));
  if (residual) hipLaunchKernelGGL((abn_apply_kernel<true>), grid, dim3(ABN_THREADS), 0, s, g, a);
  else hipLaunchKernelGGL((abn_apply_kernel<false>), grid, dim3(ABN_THREADS), 0, s, g, a);
  return launch_done(fn);
}

int mgs_abn_backward(int64_t B, int C, int64_t N, const float* x, const float* g_y, const float* weight, const float* bias,
                     const float* stats, float negative_slope, float* dx, float* dweight, float* dbias, void* workspace,
                     size_t workspace_bytes, int slices, mgs_stream_t stream) {
  const char* fn = "abn_backward";
  AbnGeom g;
  int rc = abn_check(fn, B, C, N, negative_slope, slices, &g);
  if (rc != MGS_OK) return rc;
  if (!x || !g_y || !weight || !bias || !stats || !dx || !workspace) {
    set_error("%s: NULL x, g_y, weight, bias, stats, dx or workspace", fn);
    return MGS_ERR_INVALID_ARG;
  }
  if (misaligned16(x) || misaligned16(g_y) || misaligned16(dx) || misaligned16(workspace)) {
    set_error("%s: x, g_y, dx and the workspace must be 16-byte aligned", fn);
    return MGS_ERR_INVALID_ARG;
  }
  if (int rc = workspace_short(fn, workspace_bytes, mgs_abn_workspace_bytes(B, C, N))) return rc;
  hipStream_t s = (hipStream_t)stream;
  AbnBwdArgs a;
  a.x = x; a.gy = g_y; a.weight = weight; a.bias = bias; a.stats = stats;
  a.records = reinterpret_cast<float*>(workspace); a.dx = dx; a.dweight = dweight; a.dbias = dbias;
  const dim3 grid((unsigned)(B * C * g.slices));
  hipLaunchKernelGGL(abn_bwd_sums_kernel, grid, dim3(ABN_THREADS), 0, s, g, a);
  hipLaunchKernelGGL(abn_bwd_dx_kernel, grid, dim3(ABN_THREADS), 0, s, g, a);
  return launch_done(fn);
}

}  // extern "C"
