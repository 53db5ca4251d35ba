// mgs_feedforward.hip -- what is left of a Perceiver transformer block beside the attention and the GEMMs
// (agents/manigaussian_bc/perceiver_lang_io.py:56-99: PreNorm's nn.LayerNorm, FeedForward's Linear -> GEGLU -> Linear), fused,
// fp32, wave64, forward and backward.
//
//   layernorm:   y = (x - mean) rstd w + b,  mean = sum x / D,  rstd = 1 / sqrt(sum (x - mean)^2 / D + eps)        rows of D <= 1024
//   bias-GEGLU:  out[r, j] = (h[r, j] + b[j]) gelu(h[r, M + j] + b[M + j]),  gelu(t) = t Phi(t) = t (1 + erf(t / sqrt 2)) / 2
//
// Memory: every thread owns whole groups of four consecutive columns, group t = columns 4 t .. 4 t + 3 of its row, whatever the
// row's address.  A group is READ as 16-byte aligned vectors always: the one or two aligned vectors that hold it are loaded and
// the four floats are picked out of them (ff_load4), so a row that starts off a 16-byte boundary -- the gate half of h for
// M % 4 != 0, a row of an odd width -- costs a second load that hits the cache line of the first, never four scalar loads.  Only
// vectors that hold at least one float of the row are touched.  A group is WRITTEN as one 16-byte store where its address is
// aligned and it is whole, else as up to four scalar stores (ff_store4).
//
// Sums: no atomics.  A layernorm row lives in the registers of ONE wave (up to 4 groups per lane); its sums are a fixed
// in-lane order followed by an xor butterfly.  The column sums of the backwards (dweight, dbias) go by SLABS: a slab is a run
// of `per` consecutive rows; each slab's partial sums are written to the workspace [slabs][2][cols], and ff_colsum_kernel adds
// the slabs in ascending order.  Inside a layernorm slab each of the workgroup's 8 waves sums a contiguous run of rows in row
// order and the waves' sums are added in wave order; a GEGLU slab goes the same way, a lane owning four columns of each half.
// Terms and order depend on the indices and the split alone: the same bits from run to run.  dx and dh do not depend on the split
// at all.
#include <math.h>

#include "mgs_common.h"

namespace mgs {

typedef float fff4 __attribute__((ext_vector_type(4)));

constexpr int FF_MAX_D = 1024;
constexpr int FF_MAX_SLABS = 64;
constexpr int LN_FWD_THREADS = 256;        // four rows per workgroup
constexpr int LN_BWD_WAVES = 8;            // one slab per workgroup
constexpr int LN_BWD_THREADS = LN_BWD_WAVES * WAVE;
constexpr int LN_SLAB_MIN_ROWS = LN_BWD_WAVES;  // the library's split keeps a row per wave
constexpr int GG_FWD_THREADS = 256;
constexpr int GG_BWD_WAVES = 8;            // a workgroup: 256 columns of each half, a slab of rows cut into eight runs
constexpr int GG_BWD_THREADS = GG_BWD_WAVES * WAVE;
constexpr int GG_BWD_UNROLL = 4;           // rows whose loads a wave has in flight together
constexpr int GG_SLAB_MIN_ROWS = GG_BWD_WAVES * GG_BWD_UNROLL;
constexpr int COL_THREADS = 64;

// p[j0 .. j0 + 3] of a row of n floats at p (4-byte aligned, j0 >= 0), zero where j0 + c >= n
__device__ __forceinline__ fff4 ff_load4(const float* __restrict__ p, int j0, int n) {
  fff4 r = (fff4)(0.f);
  if (j0 >= n) return r;
  const uintptr_t addr = reinterpret_cast<uintptr_t>(p + j0);
  const unsigned s = (unsigned)(addr >> 2) & 3u;           // floats between the aligned vector's start and p[j0]
  const fff4* q = reinterpret_cast<const fff4*>(addr - 4u * s);
  const fff4 A = q[0];                                     // holds p[j0] at [s]
  if (s == 0) {
    r = A;
  } else {
    fff4 B = (fff4)(0.f);
    if (j0 + 4 - (int)s < n) B = q[1];                     // holds p[j0 + 4 - s] at [0]
    r.x = s == 1 ? A.y : (s == 2 ? A.z : A.w);
    r.y = s == 1 ? A.z : (s == 2 ? A.w : B.x);
    r.z = s == 1 ? A.w : (s == 2 ? B.x : B.y);
    r.w = s == 1 ? B.x : (s == 2 ? B.y : B.z);
  }
  r.y = j0 + 1 < n ? r.y : 0.f;
  r.z = j0 + 2 < n ? r.z : 0.f;
  r.w = j0 + 3 < n ? r.w : 0.f;
  return r;
}

__device__ __forceinline__ void ff_store4(float* __restrict__ p, int j0, int n, fff4 v) {
  if (j0 >= n) return;
  float* d = p + j0;
  if (j0 + 3 < n && (reinterpret_cast<uintptr_t>(d) & 15u) == 0) {
    *reinterpret_cast<fff4*>(d) = v;
  } else {
    d[0] = v.x;
    if (j0 + 1 < n) d[1] = v.y;
    if (j0 + 2 < n) d[2] = v.z;
    if (j0 + 3 < n) d[3] = v.w;
  }
}

// every lane gets the same bits: a + b and b + a are
__device__ __forceinline__ float ff_wave_sum(float v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

__device__ __forceinline__ float ff_sum4(fff4 v) { return (v.x + v.y) + (v.z + v.w); }

// ---- layernorm ------------------------------------------------------------------------------------------------------------------
// lane l of a row's wave holds groups l, l + 64, .. l + 64 (NV - 1)
template <int NV>
__global__ __launch_bounds__(LN_FWD_THREADS) void ln_fwd_kernel(int64_t rows, int D, const float* __restrict__ x, int64_t xs,
                                                                const float* __restrict__ w, const float* __restrict__ b, float eps,
                                                                float* __restrict__ y, float* __restrict__ stats) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * (LN_FWD_THREADS / WAVE) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* xr = x + row * xs;
  fff4 v[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = ff_load4(xr, 4 * (lane + 64 * k), D);
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < NV; ++k) s += ff_sum4(v[k]);
  const float mean = ff_wave_sum(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int j0 = 4 * (lane + 64 * k);
    fff4 d = v[k] - mean;
    d.x = j0 < D ? d.x : 0.f;
    d.y = j0 + 1 < D ? d.y : 0.f;
    d.z = j0 + 2 < D ? d.z : 0.f;
    d.w = j0 + 3 < D ? d.w : 0.f;
    v[k] = d;
    q += ff_sum4(d * d);
  }
  const float rstd = 1.f / sqrtf(ff_wave_sum(q) / (float)D + eps);
  float* yr = y + row * (int64_t)D;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int j0 = 4 * (lane + 64 * k);
    const fff4 wv = ff_load4(w, j0, D), bv = ff_load4(b, j0, D);
    const fff4 xh = v[k] * rstd;
    fff4 o;
    o.x = fmaf(xh.x, wv.x, bv.x); o.y = fmaf(xh.y, wv.y, bv.y); o.z = fmaf(xh.z, wv.z, bv.z); o.w = fmaf(xh.w, wv.w, bv.w);
    ff_store4(yr, j0, D, o);
  }
  if (lane == 0) { stats[2 * row] = mean; stats[2 * row + 1] = rstd; }
}

// One workgroup per slab of `per` rows; wave v takes the v-th eighth of them.  PART: the slab's sums of g xhat and g per column
// go to partial[slab][0 | 1][D].
template <int NV, bool PART>
__global__ __launch_bounds__(LN_BWD_THREADS) void ln_bwd_kernel(int64_t rows, int D, int64_t per, const float* __restrict__ x, int64_t xs,
                                                                const float* __restrict__ w, const float* __restrict__ stats,
                                                                const float* __restrict__ g, int64_t gs, float* __restrict__ dx,
                                                                float* __restrict__ partial) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * per, r1 = min(r0 + per, rows);
  const int64_t pw = (r1 - r0 + LN_BWD_WAVES - 1) / LN_BWD_WAVES;
  const int64_t first = min(r0 + wave * pw, r1), last = min(first + pw, r1);
  fff4 wv[NV], aw[NV], ab[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    wv[k] = ff_load4(w, 4 * (lane + 64 * k), D);
    aw[k] = (fff4)(0.f);
    ab[k] = (fff4)(0.f);
  }
  for (int64_t row = first; row < last; ++row) {
    const float mean = stats[2 * row], rstd = stats[2 * row + 1];
    const float* xr = x + row * xs;
    const float* gr = g + row * gs;
    fff4 xh[NV], gw[NV];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int j0 = 4 * (lane + 64 * k);
      const fff4 gv = ff_load4(gr, j0, D);
      xh[k] = (ff_load4(xr, j0, D) - mean) * rstd;   // (columns past D: g and w are zero there)
      gw[k] = gv * wv[k];
      s1 += ff_sum4(gw[k]);
      s2 += ff_sum4(gw[k] * xh[k]);
      if (PART) {
        aw[k] += gv * xh[k];
        ab[k] += gv;
      }
    }
    const float c1 = ff_wave_sum(s1) / (float)D, c2 = ff_wave_sum(s2) / (float)D;
    float* dr = dx + row * (int64_t)D;
#pragma unroll
    for (int k = 0; k < NV; ++k) ff_store4(dr, 4 * (lane + 64 * k), D, rstd * (gw[k] - c1 - xh[k] * c2));
  }
  if (PART) {
    __shared__ fff4 acc[2][FF_MAX_D / 4];
    for (int v = 0; v < LN_BWD_WAVES - 1; ++v) {   // the waves in ascending order
      if (wave == v) {
#pragma unroll
        for (int k = 0; k < NV; ++k) {
          const int i = lane + 64 * k;
          acc[0][i] = v == 0 ? aw[k] : acc[0][i] + aw[k];
          acc[1][i] = v == 0 ? ab[k] : acc[1][i] + ab[k];
        }
      }
      __syncthreads();
    }
    if (wave == LN_BWD_WAVES - 1) {
      float* p0 = partial + (int64_t)blockIdx.x * 2 * D;
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        const int i = lane + 64 * k;
        ff_store4(p0, 4 * i, D, acc[0][i] + aw[k]);
        ff_store4(p0 + D, 4 * i, D, acc[1][i] + ab[k]);
      }
    }
  }
}

// out0[c] = sum over slabs of partial[slab][0][c], out1[c] = ... [1][c], the slabs in ascending order (blockIdx.y: which)
__global__ __launch_bounds__(COL_THREADS) void ff_colsum_kernel(int slabs, int64_t cols, const float* __restrict__ partial,
                                                                float* __restrict__ out0, float* __restrict__ out1) {
  const int64_t c = (int64_t)blockIdx.x * COL_THREADS + threadIdx.x;
  float* out = blockIdx.y ? out1 : out0;
  if (!out || c >= cols) return;
  const float* p = partial + (int64_t)blockIdx.y * cols + c;
  float s = p[0];
#pragma unroll 16
  for (int i = 1; i < slabs; ++i) s += p[(int64_t)i * 2 * cols];
  out[c] = s;
}

// ---- bias-GEGLU -----------------------------------------------------------------------------------------------------------------
constexpr float FF_RSQRT2 = 0.70710678118654752440f;
constexpr float FF_RSQRT2PI = 0.39894228040143267794f;

__device__ __forceinline__ float ff_gelu(float t) { return t * (0.5f * (1.f + erff(t * FF_RSQRT2))); }

// one thread per group of four columns of one row
__global__ __launch_bounds__(GG_FWD_THREADS) void geglu_fwd_kernel(int64_t groups, int per_row, int M, const float* __restrict__ h,
                                                                   int64_t hs, const float* __restrict__ bias, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * GG_FWD_THREADS + threadIdx.x;
  if (i >= groups) return;
  const int64_t row = i / per_row;
  const int j0 = 4 * (int)(i - row * per_row);
  const float* hr = h + row * hs;
  fff4 a = ff_load4(hr, j0, M), t = ff_load4(hr + M, j0, M);
  if (bias) {
    a += ff_load4(bias, j0, M);
    t += ff_load4(bias + M, j0, M);
  }
  fff4 o;
  o.x = a.x * ff_gelu(t.x); o.y = a.y * ff_gelu(t.y); o.z = a.z * ff_gelu(t.z); o.w = a.w * ff_gelu(t.w);
  ff_store4(out + row * (int64_t)M, j0, M, o);
}

// d/da and d/dgate of g a gelu(gate): (g gelu(gate), g a gelu'(gate)), gelu'(t) = Phi(t) + t phi(t).  In the tails erff is +-1 and
// expf is 0 exactly: gelu'(40) = 1, gelu'(-40) = 0.
struct FfPair { float da, dt; };
__device__ __forceinline__ FfPair ff_geglu_grad(float a, float t, float g) {
  const float Phi = 0.5f * (1.f + erff(t * FF_RSQRT2));
  const float phi = expf(-0.5f * t * t) * FF_RSQRT2PI;
  FfPair r;
  r.da = g * (t * Phi);
  r.dt = g * a * (Phi + t * phi);
  return r;
}

// workgroup (slab, tile): columns 256 tile .. 256 tile + 255 of both halves; wave v takes the v-th eighth of the slab's rows, in row
// order, a lane four columns of each half.  PART: the waves' column sums are added in wave order into partial[slab][0 | 1][M].
template <bool PART>
__global__ __launch_bounds__(GG_BWD_THREADS) void geglu_bwd_kernel(int64_t rows, int M, int tiles, int64_t per, const float* __restrict__ h,
                                                                   int64_t hs, const float* __restrict__ bias, const float* __restrict__ g,
                                                                   int64_t gs, float* __restrict__ dh, float* __restrict__ partial) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t slab = blockIdx.x / tiles;
  const int tile = (int)(blockIdx.x - slab * tiles);
  const int j0 = 4 * (tile * WAVE + lane);   // (a lane past M loads zeros and stores nothing)
  const int64_t s0 = slab * per, s1 = min(s0 + per, rows);
  const int64_t pw = (s1 - s0 + GG_BWD_WAVES - 1) / GG_BWD_WAVES;
  const int64_t r0 = min(s0 + wave * pw, s1), r1 = min(r0 + pw, s1);
  fff4 ba = (fff4)(0.f), bt = (fff4)(0.f);
  if (bias) {
    ba = ff_load4(bias, j0, M);
    bt = ff_load4(bias + M, j0, M);
  }
  fff4 sa = (fff4)(0.f), st = (fff4)(0.f);
  for (int64_t row = r0; row < r1; row += GG_BWD_UNROLL) {
    fff4 a[GG_BWD_UNROLL], t[GG_BWD_UNROLL], gv[GG_BWD_UNROLL];
#pragma unroll
    for (int u = 0; u < GG_BWD_UNROLL; ++u) {
      if (row + u < r1) {
        const float* hr = h + (row + u) * hs;
        a[u] = ff_load4(hr, j0, M);
        t[u] = ff_load4(hr + M, j0, M);
        gv[u] = ff_load4(g + (row + u) * gs, j0, M);
      }
    }
#pragma unroll
    for (int u = 0; u < GG_BWD_UNROLL; ++u) {
      if (row + u < r1) {
        const fff4 av = a[u] + ba, tv = t[u] + bt;
        fff4 da, dt;
        const FfPair p0 = ff_geglu_grad(av.x, tv.x, gv[u].x), p1 = ff_geglu_grad(av.y, tv.y, gv[u].y);
        const FfPair p2 = ff_geglu_grad(av.z, tv.z, gv[u].z), p3 = ff_geglu_grad(av.w, tv.w, gv[u].w);
        da.x = p0.da; da.y = p1.da; da.z = p2.da; da.w = p3.da;
        dt.x = p0.dt; dt.y = p1.dt; dt.z = p2.dt; dt.w = p3.dt;
        float* dr = dh + (row + u) * 2 * (int64_t)M;
        ff_store4(dr, j0, M, da);
        ff_store4(dr + M, j0, M, dt);
        if (PART) {   // (columns past M: g is zero there)
          sa += da;
          st += dt;
        }
      }
    }
  }
  if (PART) {
    __shared__ fff4 acc[2][WAVE];
    for (int v = 0; v < GG_BWD_WAVES - 1; ++v) {   // the waves in ascending order
      if (wave == v) {
        acc[0][lane] = v == 0 ? sa : acc[0][lane] + sa;
        acc[1][lane] = v == 0 ? st : acc[1][lane] + st;
      }
      __syncthreads();
    }
    if (wave == GG_BWD_WAVES - 1) {
      float* p0 = partial + slab * 2 * (int64_t)M;
      ff_store4(p0, j0, M, acc[0][lane] + sa);
      ff_store4(p0 + M, j0, M, acc[1][lane] + st);
    }
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
static bool misaligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) != 0; }

// rows of a slab for `rows` rows: row_split forced (1..64), or the library's (0): at most 64 slabs of at least min_rows rows
static int64_t ff_rows_per_slab(int64_t rows, int row_split, int min_rows) {
  int64_t slabs = row_split;
  if (slabs == 0) {
    slabs = (rows + min_rows - 1) / min_rows;
    if (slabs > FF_MAX_SLABS) slabs = FF_MAX_SLABS;
  }
  return (rows + slabs - 1) / slabs;
}

static size_t ff_workspace(int64_t cols) { return align_up((size_t)FF_MAX_SLABS * 2 * (size_t)cols * sizeof(float)) + ALIGN; }

static int ln_check(const char* fn, int64_t rows, int D, int64_t x_stride) {
  if (rows < 1 || D < 1 || D > FF_MAX_D) {
    set_error("%s: rows = %lld (at least 1), D = %d (1..%d)", fn, (long long)rows, D, FF_MAX_D);
    return MGS_ERR_INVALID_ARG;
  }
  if (rows * (int64_t)D > 0x7fffffffLL) {
    set_error("%s: rows x D = %lld x %d exceeds 2^31 - 1 elements", fn, (long long)rows, D);
    return MGS_ERR_INVALID_ARG;
  }
  if (x_stride < D) {
    set_error("%s: row stride of x = %lld (at least D = %d)", fn, (long long)x_stride, D);
    return MGS_ERR_INVALID_ARG;
  }
  return MGS_OK;
}

static int gg_check(const char* fn, int64_t rows, int64_t M, int64_t h_stride) {
  if (rows < 1 || M < 1) {
    set_error("%s: rows = %lld, M = %lld (each at least 1)", fn, (long long)rows, (long long)M);
    return MGS_ERR_INVALID_ARG;
  }
  if (M > 0x3fffffffLL || rows * 2 * M > 0x7fffffffLL) {
    set_error("%s: rows x 2 M = %lld x %lld exceeds 2^31 - 1 elements", fn, (long long)rows, (long long)(2 * M));
    return MGS_ERR_INVALID_ARG;
  }
  if (h_stride < 2 * M) {
    set_error("%s: row stride of h = %lld (at least 2 M = %lld)", fn, (long long)h_stride, (long long)(2 * M));
    return MGS_ERR_INVALID_ARG;
  }
  return MGS_OK;
}

// the checks the two backwards share: the upstream gradient's stride, the split, and the workspace when column sums are wanted
static int bwd_check(const char* fn, int64_t g_stride, int64_t row, int row_split, bool sums, const void* workspace,
                     size_t workspace_bytes, int64_t cols) {
  if (g_stride != 0 && g_stride < row) {
    set_error("%s: row stride of the upstream gradient = %lld (0: one row for all, or at least %lld)", fn, (long long)g_stride,
              (long long)row);
    return MGS_ERR_INVALID_ARG;
  }
  if (row_split < 0 || row_split > FF_MAX_SLABS) {
    set_error("%s: row_split = %d (0: chosen by the library, at most %d)", fn, row_split, FF_MAX_SLABS);
    return MGS_ERR_INVALID_ARG;
  }
  if (!sums) return MGS_OK;
  if (!workspace || misaligned16(workspace)) {
    set_error("%s: the workspace is NULL or not 16-byte aligned", fn);
    return MGS_ERR_INVALID_ARG;
  }
  return workspace_short(fn, workspace_bytes, ff_workspace(cols));
}

template <bool PART>
static void ln_bwd_launch(int nv, dim3 grid, hipStream_t s, int64_t rows, int D, int64_t per, const float* x, int64_t xs, const float* w,
                          const float* stats, const float* g, int64_t gs, float* dx, float* partial) {
  const dim3 block(LN_BWD_THREADS);
  switch (nv) {
    case 1: hipLaunchKernelGGL((ln_bwd_kernel<1, PART>), grid, block, 0, s, rows, D, per, x, xs, w, stats, g, gs, dx, partial); break;
    case 2: hipLaunchKernelGGL((ln_bwd_kernel<2, PART>), grid, block, 0, s, rows, D, per, x, xs, w, stats, g, gs, dx, partial); break;
    case 3: hipLaunchKernelGGL((ln_bwd_kernel<3, PART>), grid, block, 0, s, rows, D, per, x, xs, w, stats, g, gs, dx, partial); break;
    default: hipLaunchKernelGGL((ln_bwd_kernel<4, PART>), grid, block, 0, s, rows, D, per, x, xs, w, stats, g, gs, dx, partial); break;
  }
}

static void colsum_launch(hipStream_t s, int64_t slabs, int64_t cols, const float* partial, float* out0, float* out1) {
  hipLaunchKernelGGL(ff_colsum_kernel, dim3((unsigned)((cols + COL_THREADS - 1) / COL_THREADS), 2), dim3(COL_THREADS), 0, s, (int)slabs,
                     cols, partial, out0, out1);
}

}  // namespace mgs

using namespace mgs;

extern "C" {

size_t mgs_feedforward_workspace_bytes(int64_t rows, int64_t cols) {
  if (rows < 1 || cols < 1 || cols > 0x3fffffffLL) return 0;
  return ff_workspace(cols);
}

int mgs_layernorm_forward(int64_t rows, int D, const float* x, int64_t x_stride, const float* weight, const float* bias, float eps,
                          float* y, float* stats, mgs_stream_t stream) {
  const char* fn = "layernorm_forward";
  if (int rc = ln_check(fn, rows, D, x_stride)) return rc;
  if (!x || !weight || !bias || !y || !stats) { set_error("%s: NULL x, weight, bias, y or stats", fn); return MGS_ERR_INVALID_ARG; }
  if (misaligned4(x) || misaligned4(weight) || misaligned4(bias) || misaligned4(stats) || misaligned16(y)) {
    set_error("%s: y must be 16-byte aligned, the other tensors 4-byte aligned", fn);
    return MGS_ERR_INVALID_ARG;
  }
  hipStream_t s = (hipStream_t)stream;
  const int per = LN_FWD_THREADS / WAVE;
  const dim3 grid((unsigned)((rows + per - 1) / per)), block(LN_FWD_THREADS);
  switch ((D + 255) / 256) {
    case 1: hipLaunchKernelGGL((ln_fwd_kernel<1>), grid, block, 0, s, rows, D, x, x_stride, weight, bias, eps, y, stats); break;
    case 2: hipLaunchKernelGGL((ln_fwd_kernel<2>), grid, block, 0, s, rows, D, x, x_stride, weight, bias, eps, y, stats); break;
    case 3: hipLaunchKernelGGL((ln_fwd_kernel<3>), grid, block, 0, s, rows, D, x, x_stride, weight, bias, eps, y, stats); break;
    default: hipLaunchKernelGGL((ln_fwd_kernel<4>), grid, block, 0, s, rows, D, x, x_stride, weight, bias, eps, y, stats); break;
  }
  return launch_done(fn);
}

int mgs_layernorm_backward(int64_t rows, int D, const float* x, int64_t x_stride, const float* weight, const float* stats,
                           const float* g, int64_t g_stride, float* dx, float* dweight, float* dbias, void* workspace,
                           size_t workspace_bytes, int row_split, mgs_stream_t stream) {
  const char* fn = "layernorm_backward";
  if (int rc = ln_check(fn, rows, D, x_stride)) return rc;
  if (!x || !weight || !stats || !g || !dx) { set_error("%s: NULL x, weight, stats, g or dx", fn); return MGS_ERR_INVALID_ARG; }
  if (misaligned4(x) || misaligned4(weight) || misaligned4(stats) || misaligned4(g) || misaligned4(dweight) || misaligned4(dbias) ||
      misaligned16(dx)) {
    set_error("%s: dx must be 16-byte aligned, the other tensors 4-byte aligned", fn);
    return MGS_ERR_INVALID_ARG;
  }
  const bool sums = dweight || dbias;
  if (int rc = bwd_check(fn, g_stride, D, row_split, sums, workspace, workspace_bytes, D)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int nv = (D + 255) / 256;
  if (!sums) {   // frozen parameters: dx alone, a row per wave, no partial sums and no second launch
    const int64_t per = LN_BWD_WAVES;
    ln_bwd_launch<false>(nv, dim3((unsigned)((rows + per - 1) / per)), s, rows, D, per, x, x_stride, weight, stats, g, g_stride, dx, nullptr);
    return launch_done(fn);
  }
  const int64_t per = ff_rows_per_slab(rows, row_split, LN_SLAB_MIN_ROWS), slabs = (rows + per - 1) / per;
  float* partial = reinterpret_cast<float*>(workspace);
  ln_bwd_launch<true>(nv, dim3((unsigned)slabs), s, rows, D, per, x, x_stride, weight, stats, g, g_stride, dx, partial);
  colsum_launch(s, slabs, D, partial, dweight, dbias);
  return launch_done(fn);
}

int mgs_bias_geglu_forward(int64_t rows, int64_t M, const float* h, int64_t h_stride, const float* bias, float* out,
                           mgs_stream_t stream) {
  const char* fn = "bias_geglu_forward";
  if (int rc = gg_check(fn, rows, M, h_stride)) return rc;
  if (!h || !out) { set_error("%s: NULL h or out", fn); return MGS_ERR_INVALID_ARG; }
  if (misaligned4(h) || misaligned4(bias) || misaligned16(out)) {
    set_error("%s: out must be 16-byte aligned, h and bias 4-byte aligned", fn);
    return MGS_ERR_INVALID_ARG;
  }
  const int64_t per_row = (M + 3) / 4, groups = rows * per_row;
  hipLaunchKernelGGL(geglu_fwd_kernel, dim3((unsigned)((groups + GG_FWD_THREADS - 1) / GG_FWD_THREADS)), dim3(GG_FWD_THREADS), 0,
                     (hipStream_t)stream, groups, (int)per_row, (int)M, h, h_stride, bias, out);
  return launch_done(fn);
}

int mgs_bias_geglu_backward(int64_t rows, int64_t M, const float* h, int64_t h_stride, const float* bias, const float* g,
                            int64_t g_stride, float* dh, float* dbias, void* workspace, size_t workspace_bytes, int row_split,
                            mgs_stream_t stream) {
  const char* fn = "bias_geglu_backward";
  if (int rc = gg_check(fn, rows, M, h_stride)) return rc;
  if (!h || !g || !dh) { set_error("%s: NULL h, g or dh", fn); return MGS_ERR_INVALID_ARG; }
  if (misaligned4(h) || misaligned4(bias) || misaligned4(g) || misaligned4(dbias) || misaligned16(dh)) {
    set_error("%s: dh must be 16-byte aligned, the other tensors 4-byte aligned", fn);
    return MGS_ERR_INVALID_ARG;
  }
  const bool sums = dbias != nullptr;
  if (int rc = bwd_check(fn, g_stride, M, row_split, sums, workspace, workspace_bytes, M)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int64_t tiles = (M + 4 * WAVE - 1) / (4 * WAVE);
  if (!sums) {   // no bias gradient wanted: no partial sums and no second launch; a few rows per wave
    const int64_t per = GG_SLAB_MIN_ROWS, slabs = (rows + per - 1) / per;
    hipLaunchKernelGGL((geglu_bwd_kernel<false>), dim3((unsigned)(slabs * tiles)), dim3(GG_BWD_THREADS), 0, s, rows, (int)M, (int)tiles,
                       per, h, h_stride, bias, g, g_stride, dh, (float*)nullptr);
    return launch_done(fn);
  }
  const int64_t per = ff_rows_per_slab(rows, row_split, GG_SLAB_MIN_ROWS), slabs = (rows + per - 1) / per;
  float* partial = reinterpret_cast<float*>(workspace);
  hipLaunchKernelGGL((geglu_bwd_kernel<true>), dim3((unsigned)(slabs * tiles)), dim3(GG_BWD_THREADS), 0, s, rows, (int)M, (int)tiles, per,
                     h, h_stride, bias, g, g_stride, dh, partial);
  colsum_launch(s, slabs, M, partial, dbias, dbias + M);
  return launch_done(fn);
}

}  // extern "C"
