// mgs_attention.hip -- the Perceiver's attention (agents/manigaussian_bc/perceiver_lang_io.py:102-145), fused, fp32 throughout:
// softmax(q k^T * D^-0.5, masked keys at -FLT_MAX) -> dropout -> . v, forward and backward, head dimension D = 64 only.
// Nothing of size Nq x Nk exists: a wave keeps 16 query rows (forward, dQ) or 16 key rows (dK, dV) in registers, the other
// side streams through LDS in tiles of 64 rows, and the backward recomputes the probabilities from the row log-sum-exp.
//
// Instruction: v_mfma_f32_16x16x4_f32 (exact fp32 products and sums, the fp32 vector peak).  The score block is computed
// TRANSPOSED, S^T = K Q^T, so that the accumulator layout of one MFMA (lane l holds rows 4 (l / 16) + r, r = 0..3, of column
// l % 16) is already the B-operand layout of the next one (P^T as the "k x n" operand of O^T = V^T P^T, the four k slots of
// step r being keys 4 (l / 16) + r): the probabilities never pass through LDS, and every lane owns ONE query column, so the
// running maximum and sum are one register each and cost two cross-lane steps per tile.
//
//   attn_fwd_kernel    a workgroup of NW waves owns NW x 16 queries of one (batch, head); online softmax over key tiles
//   attn_delta_kernel  D_i = sum_d dO . O
//   attn_dq_kernel     the forward's geometry again: P from lse, dS = P (dP - D_i), dQ = dS K * scale
//   attn_dkv_kernel    a workgroup owns NW x 16 keys and loops over query tiles: dV = Pdrop^T dO, dK = dS^T Q * scale
//   attn_mask_kernel   the keep decisions as bytes (test and debug aid)
// No atomics anywhere: every output float is written once, by one lane, from sums taken in a fixed order -- bit-identical from
// run to run, and independent of NW (a wave's arithmetic does not depend on its workgroup).  Seed and offset of the dropout are
// read from device memory by the kernels; no host read, no allocation: capturable into a HIP graph.
#include <float.h>
#include <math.h>

#include "mgs_common.h"
#include "mgs_device.h"

namespace mgs {

constexpr int ATT_D = 64;    // head dimension (the only one compiled)
constexpr int ATT_T = 64;    // rows of an LDS tile (keys in the forward and dQ, queries in dK/dV)
constexpr int ATT_LD = 68;   // floats per LDS row: 16-byte aligned rows; both operand patterns (row l % 16, column 4 t + l / 16 and
                             // row 4 (l / 16) + r, column 16 c + l % 16) touch 64 different banks
constexpr int ATT_WQ = 16;   // rows a wave owns
constexpr int ATT_CUS = 256; // below one 4-wave workgroup per CU the one-wave form is launched (four times the workgroups)

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct AttnK {
  int B, H, Nq, Nk;
  const float *q, *k, *v;
  const uint8_t* mask;
  int64_t q_sb, q_sn, k_sb, k_sn, v_sb, v_sn, o_sb, o_sn, do_sb, do_sn, dq_sb, dq_sn, dkv_sb, dkv_sn, mask_sb;
  float* out;
  float* lse;
  const float* o_in;   // backward: the forward's out
  const float* d_out;
  float* dq;
  float* dkv;
  float* delta;
  const unsigned long long* rng;  // device {seed, offset}
  uint32_t thr;                   // keep iff word >= thr
  float inv_keep, scale, inv_nk;
};

// ---- dropout: Philox4x32-10 (mgs_device.h), counter (j >> 2, i, b H + h, offset low), key (seed low, seed high ^ offset
// high); element (b H + h, i, j) takes word j & 3 and is kept iff word >= floor(p 2^32).

// ---- tile loads: rows [row0, row0 + 64) of a [*, n_rows, stride] array, 64 floats from column `col`, zero beyond n_rows
template <int NT>
__device__ __forceinline__ void load_tile(float* __restrict__ dst, const float* __restrict__ src, int64_t stride, int row0,
                                          int n_rows, int tid) {
#pragma unroll
  for (int it = 0; it < ATT_T * 16 / NT; it++) {
    const int idx = tid + it * NT, row = idx >> 4, c4 = idx & 15;
    float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row0 + row < n_rows) val = *reinterpret_cast<const float4*>(src + (int64_t)(row0 + row) * stride + 4 * c4);
    *reinterpret_cast<float4*>(dst + row * ATT_LD + 4 * c4) = val;
  }
}

// state of a key: 1 live, 0 masked (score -FLT_MAX), 2 beyond Nk (no score at all)
__device__ __forceinline__ uint8_t key_state(const AttnK& a, int b, int j) {
  if (j >= a.Nk) return 2;
  return a.mask ? (a.mask[(int64_t)b * a.mask_sb + j] != 0 ? 1 : 0) : 1;
}

// rows [q0 + l % 16] of a [B, N, *] array as the B operand of 16 MFMA steps: element d = 4 t + l / 16
__device__ __forceinline__ void load_frag(float (&f)[16], const float* __restrict__ base, int64_t stride, int row, int n_rows,
                                          int lg) {
  if (row < n_rows) {
    const float* __restrict__ p = base + (int64_t)row * stride + lg;
#pragma unroll
    for (int t = 0; t < 16; t++) f[t] = p[4 * t];
  } else {
#pragma unroll
    for (int t = 0; t < 16; t++) f[t] = 0.f;
  }
}

// c[x] (16 x 16, x = 0..3) += A_x B: A_x = rows 16 x + l % 16 of an LDS tile (columns 4 t + l / 16), B = a register fragment
__device__ __forceinline__ void mma_rows(f32x4 (&c)[4], const float* __restrict__ tile, const float (&f)[16], int lq, int lg) {
#pragma unroll
  for (int t = 0; t < 16; t++) {
#pragma unroll
    for (int x = 0; x < 4; x++)
      c[x] = __builtin_amdgcn_mfma_f32_16x16x4f32(tile[(16 * x + lq) * ATT_LD + 4 * t + lg], f[t], c[x], 0, 0, 0);
  }
}

// acc[c] (d = 16 c + ., column l % 16) += sum over the tile's rows 16 x + 4 (l / 16) + r of tile[row][d] * w[x][r]
__device__ __forceinline__ void mma_cols(f32x4 (&acc)[4], const float* __restrict__ tile, const f32x4 (&w)[4], int lq, int lg) {
#pragma unroll
  for (int x = 0; x < 4; x++) {
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const float* __restrict__ row = tile + (16 * x + 4 * lg + r) * ATT_LD + lq;
#pragma unroll
      for (int c = 0; c < 4; c++) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(row[16 * c], w[x][r], acc[c], 0, 0, 0);
    }
  }
}

__device__ __forceinline__ float xor_max(float v) {
  v = fmaxf(v, __shfl_xor(v, 16, WAVE));
  return fmaxf(v, __shfl_xor(v, 32, WAVE));
}
__device__ __forceinline__ float xor_sum(float v) {
  v += __shfl_xor(v, 16, WAVE);
  return v + __shfl_xor(v, 32, WAVE);
}

// probability of a key of state st whose scaled score is sv, in a row of log-sum-exp lse.  A masked key's score is -FLT_MAX:
// exp(-FLT_MAX - lse) is 0 for every row with a live key, and a row of masked keys only has lse = -FLT_MAX + log Nk = -FLT_MAX
// in fp32 and attends uniformly (the forward's 1 / Nk)
__device__ __forceinline__ float prob_of(uint32_t st, float sv, float lse, float inv_nk) {
  if (st == 1u) return expf(sv - lse);
  return (st == 0u && lse <= -FLT_MAX) ? inv_nk : 0.f;
}

// =====================================================================================================================
template <int NW, bool DROP>
__global__ void __launch_bounds__(NW * 64) attn_fwd_kernel(AttnK a) {
  constexpr int NT = NW * 64;
  __shared__ __attribute__((aligned(16))) float Ks[ATT_T * ATT_LD];
  __shared__ __attribute__((aligned(16))) float Vs[ATT_T * ATT_LD];
  __shared__ __attribute__((aligned(16))) uint8_t St[ATT_T];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lq = lane & 15, lg = lane >> 4;
  const int bh = blockIdx.y, b = bh / a.H, h = bh - b * a.H;
  const int qi = blockIdx.x * (NW * ATT_WQ) + wave * ATT_WQ + lq;
  float qf[16];
  load_frag(qf, a.q + (int64_t)b * a.q_sb + h * ATT_D, a.q_sn, qi, a.Nq, lg);
  const float* __restrict__ kb_ = a.k + (int64_t)b * a.k_sb + h * ATT_D;
  const float* __restrict__ vb_ = a.v + (int64_t)b * a.v_sb + h * ATT_D;
  Philox ph = {};
  if (DROP) ph = philox_init(a.rng);
  float m_i = -INFINITY, l_i = 0.f;
  f32x4 acc[4];
#pragma unroll
  for (int c = 0; c < 4; c++) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int kt = 0; kt < a.Nk; kt += ATT_T) {
    __syncthreads();
    load_tile<NT>(Ks, kb_, a.k_sn, kt, a.Nk, tid);
    load_tile<NT>(Vs, vb_, a.v_sn, kt, a.Nk, tid);
    if (tid < ATT_T) St[tid] = key_state(a, b, kt + tid);
    __syncthreads();
    f32x4 s[4];
#pragma unroll
    for (int x = 0; x < 4; x++) s[x] = f32x4{0.f, 0.f, 0.f, 0.f};
    mma_rows(s, Ks, qf, lq, lg);  // s[x][r] = q_(lq) . k_(kt + 16 x + 4 lg + r)
    float mx = -INFINITY;
#pragma unroll
    for (int x = 0; x < 4; x++) {
      const uint32_t st4 = *reinterpret_cast<const uint32_t*>(St + 16 * x + 4 * lg);
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const uint32_t st = (st4 >> (8 * r)) & 0xffu;
        const float sv = st == 1u ? s[x][r] * a.scale : st == 0u ? -FLT_MAX : -INFINITY;
        s[x][r] = sv;
        mx = fmaxf(mx, sv);
      }
    }
    const float m_new = fmaxf(m_i, xor_max(mx));  // finite: every tile holds a key below Nk, whose score is >= -FLT_MAX
    const float alpha = expf(m_i - m_new);
    float rs = 0.f;
#pragma unroll
    for (int x = 0; x < 4; x++) {
      uint4 w = make_uint4(0u, 0u, 0u, 0u);
      if (DROP) w = philox4(ph, (uint32_t)(kt + 16 * x + 4 * lg) >> 2, (uint32_t)qi, (uint32_t)bh);
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const float p = expf(s[x][r] - m_new);
        rs += p;
        s[x][r] = DROP ? (word_of(w, r) >= a.thr ? p * a.inv_keep : 0.f) : p;
      }
    }
    l_i = l_i * alpha + xor_sum(rs);
    m_i = m_new;
#pragma unroll
    for (int c = 0; c < 4; c++) acc[c] *= alpha;
    mma_cols(acc, Vs, s, lq, lg);  // acc[c][r] = out_(lq)[16 c + 4 lg + r]
  }
  if (qi < a.Nq) {
    const float inv = 1.f / l_i;
    float* __restrict__ o = a.out + (int64_t)b * a.o_sb + (int64_t)qi * a.o_sn + h * ATT_D + 4 * lg;
#pragma unroll
    for (int c = 0; c < 4; c++)
      *reinterpret_cast<float4*>(o + 16 * c) = make_float4(acc[c][0] * inv, acc[c][1] * inv, acc[c][2] * inv, acc[c][3] * inv);
    if (lg == 0) a.lse[(int64_t)bh * a.Nq + qi] = m_i + logf(l_i);
  }
}

// D_i = sum_d dO . O of one (batch, head, query) per thread, d ascending
__global__ void __launch_bounds__(256) attn_delta_kernel(AttnK a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)a.B * a.H * a.Nq) return;
  const int bh = (int)(i / a.Nq), n = (int)(i - (int64_t)bh * a.Nq), b = bh / a.H, h = bh - b * a.H;
  const float4* __restrict__ o = reinterpret_cast<const float4*>(a.o_in + (int64_t)b * a.o_sb + (int64_t)n * a.o_sn + h * ATT_D);
  const float4* __restrict__ g = reinterpret_cast<const float4*>(a.d_out + (int64_t)b * a.do_sb + (int64_t)n * a.do_sn + h * ATT_D);
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < 16; c++) {
    const float4 x = o[c], y = g[c];
    s += x.x * y.x; s += x.y * y.y; s += x.z * y.z; s += x.w * y.w;
  }
  a.delta[i] = s;
}

template <int NW, bool DROP>
__global__ void __launch_bounds__(NW * 64) attn_dq_kernel(AttnK a) {
  constexpr int NT = NW * 64;
  __shared__ __attribute__((aligned(16))) float Ks[ATT_T * ATT_LD];
  __shared__ __attribute__((aligned(16))) float Vs[ATT_T * ATT_LD];
  __shared__ __attribute__((aligned(16))) uint8_t St[ATT_T];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lq = lane & 15, lg = lane >> 4;
  const int bh = blockIdx.y, b = bh / a.H, h = bh - b * a.H;
  const int qi = blockIdx.x * (NW * ATT_WQ) + wave * ATT_WQ + lq;
  float qf[16], gf[16];
  load_frag(qf, a.q + (int64_t)b * a.q_sb + h * ATT_D, a.q_sn, qi, a.Nq, lg);
  load_frag(gf, a.d_out + (int64_t)b * a.do_sb + h * ATT_D, a.do_sn, qi, a.Nq, lg);
  const float lse = qi < a.Nq ? a.lse[(int64_t)bh * a.Nq + qi] : INFINITY;
  const float dlt = qi < a.Nq ? a.delta[(int64_t)bh * a.Nq + qi] : 0.f;
  const float* __restrict__ kb_ = a.k + (int64_t)b * a.k_sb + h * ATT_D;
  const float* __restrict__ vb_ = a.v + (int64_t)b * a.v_sb + h * ATT_D;
  Philox ph = {};
  if (DROP) ph = philox_init(a.rng);
  f32x4 acc[4];
#pragma unroll
  for (int c = 0; c < 4; c++) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int kt = 0; kt < a.Nk; kt += ATT_T) {
    __syncthreads();
    load_tile<NT>(Ks, kb_, a.k_sn, kt, a.Nk, tid);
    load_tile<NT>(Vs, vb_, a.v_sn, kt, a.Nk, tid);
    if (tid < ATT_T) St[tid] = key_state(a, b, kt + tid);
    __syncthreads();
    f32x4 s[4], dp[4];
#pragma unroll
    for (int x = 0; x < 4; x++) { s[x] = f32x4{0.f, 0.f, 0.f, 0.f}; dp[x] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    mma_rows(s, Ks, qf, lq, lg);
    mma_rows(dp, Vs, gf, lq, lg);  // dp[x][r] = dO_(lq) . v_(kt + 16 x + 4 lg + r)
#pragma unroll
    for (int x = 0; x < 4; x++) {
      const uint32_t st4 = *reinterpret_cast<const uint32_t*>(St + 16 * x + 4 * lg);
      uint4 w = make_uint4(0u, 0u, 0u, 0u);
      if (DROP) w = philox4(ph, (uint32_t)(kt + 16 * x + 4 * lg) >> 2, (uint32_t)qi, (uint32_t)bh);
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const uint32_t st = (st4 >> (8 * r)) & 0xffu;
        const float p = prob_of(st, s[x][r] * a.scale, lse, a.inv_nk);
        float g = dp[x][r];
        if (DROP) g = word_of(w, r) >= a.thr ? g * a.inv_keep : 0.f;
        s[x][r] = st == 1u ? p * (g - dlt) : 0.f;  // a masked score is a constant: no gradient passes through it
      }
    }
    mma_cols(acc, Ks, s, lq, lg);
  }
  if (qi < a.Nq) {
    float* __restrict__ o = a.dq + (int64_t)b * a.dq_sb + (int64_t)qi * a.dq_sn + h * ATT_D + 4 * lg;
#pragma unroll
    for (int c = 0; c < 4; c++)
      *reinterpret_cast<float4*>(o + 16 * c) =
          make_float4(acc[c][0] * a.scale, acc[c][1] * a.scale, acc[c][2] * a.scale, acc[c][3] * a.scale);
  }
}

template <int NW, bool DROP>
__global__ void __launch_bounds__(NW * 64) attn_dkv_kernel(AttnK a) {
  constexpr int NT = NW * 64;
  __shared__ __attribute__((aligned(16))) float Qs[ATT_T * ATT_LD];
  __shared__ __attribute__((aligned(16))) float Gs[ATT_T * ATT_LD];
  __shared__ __attribute__((aligned(16))) float Ls[ATT_T];
  __shared__ __attribute__((aligned(16))) float Ds[ATT_T];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lq = lane & 15, lg = lane >> 4;
  const int bh = blockIdx.y, b = bh / a.H, h = bh - b * a.H;
  const int kj = blockIdx.x * (NW * ATT_WQ) + wave * ATT_WQ + lq;
  float kf[16], vf[16];
  load_frag(kf, a.k + (int64_t)b * a.k_sb + h * ATT_D, a.k_sn, kj, a.Nk, lg);
  load_frag(vf, a.v + (int64_t)b * a.v_sb + h * ATT_D, a.v_sn, kj, a.Nk, lg);
  const uint32_t st = key_state(a, b, kj);
  const float* __restrict__ qb_ = a.q + (int64_t)b * a.q_sb + h * ATT_D;
  const float* __restrict__ gb_ = a.d_out + (int64_t)b * a.do_sb + h * ATT_D;
  Philox ph = {};
  if (DROP) ph = philox_init(a.rng);
  f32x4 ak[4], av[4];
#pragma unroll
  for (int c = 0; c < 4; c++) { ak[c] = f32x4{0.f, 0.f, 0.f, 0.f}; av[c] = f32x4{0.f, 0.f, 0.f, 0.f}; }

  for (int qt = 0; qt < a.Nq; qt += ATT_T) {
    __syncthreads();
    load_tile<NT>(Qs, qb_, a.q_sn, qt, a.Nq, tid);
    load_tile<NT>(Gs, gb_, a.do_sn, qt, a.Nq, tid);
    if (tid < ATT_T) {
      const bool ok = qt + tid < a.Nq;
      Ls[tid] = ok ? a.lse[(int64_t)bh * a.Nq + qt + tid] : INFINITY;  // a query beyond Nq: probability 0
      Ds[tid] = ok ? a.delta[(int64_t)bh * a.Nq + qt + tid] : 0.f;
    }
    __syncthreads();
    f32x4 s[4], dp[4];
#pragma unroll
    for (int x = 0; x < 4; x++) { s[x] = f32x4{0.f, 0.f, 0.f, 0.f}; dp[x] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    mma_rows(s, Qs, kf, lq, lg);   // s[x][r] = q_(qt + 16 x + 4 lg + r) . k_(lq)
    mma_rows(dp, Gs, vf, lq, lg);  // dp[x][r] = dO_(the same query) . v_(lq)
#pragma unroll
    for (int x = 0; x < 4; x++) {
      const f32x4 l4 = *reinterpret_cast<const f32x4*>(Ls + 16 * x + 4 * lg);
      const f32x4 d4 = *reinterpret_cast<const f32x4*>(Ds + 16 * x + 4 * lg);
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const float p = prob_of(st, s[x][r] * a.scale, l4[r], a.inv_nk);
        float g = dp[x][r], pd = p;
        if (DROP) {
          const uint4 w = philox4(ph, (uint32_t)kj >> 2, (uint32_t)(qt + 16 * x + 4 * lg + r), (uint32_t)bh);
          const bool keep = word_of(w, kj & 3) >= a.thr;
          g = keep ? g * a.inv_keep : 0.f;
          pd = keep ? p * a.inv_keep : 0.f;
        }
        dp[x][r] = pd;
        s[x][r] = st == 1u ? p * (g - d4[r]) : 0.f;
      }
    }
    mma_cols(av, Gs, dp, lq, lg);
    mma_cols(ak, Qs, s, lq, lg);
  }
  if (kj < a.Nk) {
    float* __restrict__ o = a.dkv + (int64_t)b * a.dkv_sb + (int64_t)kj * a.dkv_sn + h * ATT_D + 4 * lg;
    float* __restrict__ ov = o + a.H * ATT_D;
#pragma unroll
    for (int c = 0; c < 4; c++) {
      *reinterpret_cast<float4*>(o + 16 * c) =
          make_float4(ak[c][0] * a.scale, ak[c][1] * a.scale, ak[c][2] * a.scale, ak[c][3] * a.scale);
      *reinterpret_cast<float4*>(ov + 16 * c) = make_float4(av[c][0], av[c][1], av[c][2], av[c][3]);
    }
  }
}

__global__ void __launch_bounds__(256) attn_mask_kernel(AttnK a, uint8_t* __restrict__ keep) {
  const Philox ph = philox_init(a.rng);
  const int64_t row = blockIdx.x;  // (b H + h) Nq + i
  const int bh = (int)(row / a.Nq), i = (int)(row - (int64_t)bh * a.Nq);
  const int j = blockIdx.y * 256 + threadIdx.x;
  if (j >= a.Nk) return;
  const uint4 w = philox4(ph, (uint32_t)j >> 2, (uint32_t)i, (uint32_t)bh);
  keep[row * a.Nk + j] = word_of(w, j & 3) >= a.thr ? 1 : 0;
}

// =====================================================================================================================
static bool bad_stride(int64_t sn, int64_t sb, int64_t row) { return sn < row || (sn & 3) != 0 || (sb & 3) != 0 || sb < 0; }

static int attn_check(const char* fn, const MgsAttentionArgs* a) {
  if (!a) { set_error("%s: NULL arguments", fn); return MGS_ERR_INVALID_ARG; }
  if (a->D != ATT_D) { set_error("%s: head dimension %d (only %d is compiled)", fn, a->D, ATT_D); return MGS_ERR_INVALID_ARG; }
  if (a->B < 1 || a->H < 1 || a->Nq < 1 || a->Nk < 1 || (int64_t)a->B * a->H > 65535) {
    set_error("%s: B = %d, H = %d, Nq = %d, Nk = %d (each >= 1, B H <= 65535)", fn, a->B, a->H, a->Nq, a->Nk);
    return MGS_ERR_INVALID_ARG;
  }
  if (!(a->dropout_p >= 0.f && a->dropout_p < 1.f)) {
    set_error("%s: dropout_p = %g outside [0, 1)", fn, (double)a->dropout_p);
    return MGS_ERR_INVALID_ARG;
  }
  if (a->dropout_p > 0.f && !a->rng_state) { set_error("%s: dropout_p > 0 needs rng_state", fn); return MGS_ERR_INVALID_ARG; }
  if (a->rng_state && (reinterpret_cast<uintptr_t>(a->rng_state) & 7u)) {
    set_error("%s: rng_state must be 8-byte aligned", fn);
    return MGS_ERR_INVALID_ARG;
  }
  return MGS_OK;
}

static int attn_check_qkv(const char* fn, const MgsAttentionArgs* a) {
  if (!a->q || !a->k || !a->v) { set_error("%s: NULL q, k or v", fn); return MGS_ERR_INVALID_ARG; }
  if (misaligned16(a->q) || misaligned16(a->k) || misaligned16(a->v)) {
    set_error("%s: q, k and v must be 16-byte aligned", fn);
    return MGS_ERR_INVALID_ARG;
  }
  const int64_t row = (int64_t)a->H * ATT_D;
  if (bad_stride(a->q_stride_n, a->q_stride_b, row) || bad_stride(a->k_stride_n, a->k_stride_b, row) ||
      bad_stride(a->v_stride_n, a->v_stride_b, row)) {
    set_error("%s: row strides of q, k, v (%lld, %lld, %lld) must be multiples of 4 and at least the row of %lld floats", fn,
              (long long)a->q_stride_n, (long long)a->k_stride_n, (long long)a->v_stride_n, (long long)row);
    return MGS_ERR_INVALID_ARG;
  }
  if (a->mask && a->mask_stride_b < a->Nk) {
    set_error("%s: mask stride %lld shorter than its row of %d", fn, (long long)a->mask_stride_b, a->Nk);
    return MGS_ERR_INVALID_ARG;
  }
  return MGS_OK;
}

static AttnK attn_args(const MgsAttentionArgs* a) {
  AttnK k = {};
  k.B = a->B; k.H = a->H; k.Nq = a->Nq; k.Nk = a->Nk;
  k.q = a->q; k.k = a->k; k.v = a->v; k.mask = a->mask;
  k.q_sb = a->q_stride_b; k.q_sn = a->q_stride_n; k.k_sb = a->k_stride_b; k.k_sn = a->k_stride_n;
  k.v_sb = a->v_stride_b; k.v_sn = a->v_stride_n; k.o_sb = a->out_stride_b; k.o_sn = a->out_stride_n;
  k.do_sb = a->dout_stride_b; k.do_sn = a->dout_stride_n; k.dq_sb = a->dq_stride_b; k.dq_sn = a->dq_stride_n;
  k.dkv_sb = a->dkv_stride_b; k.dkv_sn = a->dkv_stride_n; k.mask_sb = a->mask_stride_b;
  k.rng = reinterpret_cast<const unsigned long long*>(a->rng_state);
  const double thr = floor((double)a->dropout_p * 4294967296.0);
  k.thr = (uint32_t)thr;
  k.inv_keep = 1.f / (1.f - a->dropout_p);
  k.scale = 0.125f;  // 64 ** -0.5
  k.inv_nk = 1.f / (float)a->Nk;
  return k;
}

// rows = queries (forward, dQ) or keys (dK/dV) each (batch, head) splits among workgroups
static bool wide(const MgsAttentionArgs* a, int rows) {
  return (int64_t)a->B * a->H * ((rows + 4 * ATT_WQ - 1) / (4 * ATT_WQ)) >= ATT_CUS;
}

#define ATT_LAUNCH(kernel, rows, drop, s, k)                                                                              \
  do {                                                                                                                    \
    if (wide(a, rows)) {                                                                                                  \
      const dim3 g((rows + 4 * ATT_WQ - 1) / (4 * ATT_WQ), a->B * a->H);                                                  \
      if (drop) hipLaunchKernelGGL((kernel<4, true>), g, dim3(256), 0, s, k);                                             \
      else hipLaunchKernelGGL((kernel<4, false>), g, dim3(256), 0, s, k);                                                 \
    } else {                                                                                                              \
      const dim3 g((rows + ATT_WQ - 1) / ATT_WQ, a->B * a->H);                                                            \
      if (drop) hipLaunchKernelGGL((kernel<1, true>), g, dim3(64), 0, s, k);                                              \
      else hipLaunchKernelGGL((kernel<1, false>), g, dim3(64), 0, s, k);                                                  \
    }                                                                                                                     \
  } while (0)

}  // namespace mgs

using namespace mgs;

extern "C" {

size_t mgs_attention_workspace_bytes(int B, int H, int Nq, int Nk) {
  if (B < 1 || H < 1 || Nq < 1 || Nk < 1) return 0;
  return align_up((size_t)B * (size_t)H * (size_t)Nq * sizeof(float)) + ALIGN;  // D_i
}

int mgs_attention_forward(const MgsAttentionArgs* a, float* out, float* lse, mgs_stream_t stream) {
  const char* fn = "attention_forward";
  int rc = attn_check(fn, a);
  if (rc == MGS_OK) rc = attn_check_qkv(fn, a);
  if (rc != MGS_OK) return rc;
  if (!out || !lse || misaligned16(out) || bad_stride(a->out_stride_n, a->out_stride_b, (int64_t)a->H * ATT_D)) {
    set_error("%s: out and lse must be given, out 16-byte aligned with a row stride (%lld) that is a multiple of 4 and at least "
              "the row", fn, (long long)a->out_stride_n);
    return MGS_ERR_INVALID_ARG;
  }
  AttnK k = attn_args(a);
  k.out = out; k.lse = lse;
  hipStream_t s = (hipStream_t)stream;
  const bool drop = a->dropout_p > 0.f;
  ATT_LAUNCH(attn_fwd_kernel, a->Nq, drop, s, k);
  return launch_done(fn);
}

int mgs_attention_backward(const MgsAttentionArgs* a, const float* out, const float* lse, const float* d_out, float* dq,
                           float* dkv, void* workspace, size_t workspace_bytes, mgs_stream_t stream) {
  const char* fn = "attention_backward";
  int rc = attn_check(fn, a);
  if (rc == MGS_OK) rc = attn_check_qkv(fn, a);
  if (rc != MGS_OK) return rc;
  const int64_t row = (int64_t)a->H * ATT_D;
  if (!out || !lse || !d_out || !dq || !dkv || !workspace) { set_error("%s: NULL pointer", fn); return MGS_ERR_INVALID_ARG; }
  if (misaligned16(out) || misaligned16(d_out) || misaligned16(dq) || misaligned16(dkv) || misaligned16(workspace)) {
    set_error("%s: out, d_out, dq, dkv and the workspace must be 16-byte aligned", fn);
    return MGS_ERR_INVALID_ARG;
  }
  if (bad_stride(a->out_stride_n, a->out_stride_b, row) || bad_stride(a->dout_stride_n, a->dout_stride_b, row) ||
      bad_stride(a->dq_stride_n, a->dq_stride_b, row) || bad_stride(a->dkv_stride_n, a->dkv_stride_b, 2 * row)) {
    set_error("%s: row strides of out, d_out, dq (%lld, %lld, %lld: at least %lld) and dkv (%lld: at least %lld) must be "
              "multiples of 4", fn, (long long)a->out_stride_n, (long long)a->dout_stride_n, (long long)a->dq_stride_n,
              (long long)row, (long long)a->dkv_stride_n, (long long)(2 * row));
    return MGS_ERR_INVALID_ARG;
  }
  const size_t need = mgs_attention_workspace_bytes(a->B, a->H, a->Nq, a->Nk);
  if (int rc = workspace_short(fn, workspace_bytes, need)) return rc;
  AttnK k = attn_args(a);
  k.o_in = out; k.lse = const_cast<float*>(lse); k.d_out = d_out; k.dq = dq; k.dkv = dkv;
  k.delta = reinterpret_cast<float*>(workspace);
  hipStream_t s = (hipStream_t)stream;
  const bool drop = a->dropout_p > 0.f;
  const int64_t rows = (int64_t)a->B * a->H * a->Nq;
  hipLaunchKernelGGL(attn_delta_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, k);
  ATT_LAUNCH(attn_dq_kernel, a->Nq, drop, s, k);
  ATT_LAUNCH(attn_dkv_kernel, a->Nk, drop, s, k);
  return launch_done(fn);
}

int mgs_attention_dropout_mask(const MgsAttentionArgs* a, uint8_t* keep, mgs_stream_t stream) {
  const char* fn = "attention_dropout_mask";
  int rc = attn_check(fn, a);
  if (rc != MGS_OK) return rc;
  if (!keep || !a->rng_state) { set_error("%s: keep and rng_state must be given", fn); return MGS_ERR_INVALID_ARG; }
  if ((int64_t)a->B * a->H * a->Nq > 0x7fffffff || a->Nk > 65535 * 256) {
    set_error("%s: B H Nq = %lld rows of %d (at most 2^31 - 1 rows of 2^24 - 256 for this debug aid)", fn,
              (long long)a->B * a->H * a->Nq, a->Nk);
    return MGS_ERR_INVALID_ARG;
  }
  AttnK k = attn_args(a);
  hipLaunchKernelGGL(attn_mask_kernel, dim3((unsigned)(a->B * a->H * a->Nq), (a->Nk + 255) / 256), dim3(256), 0,
                     (hipStream_t)stream, k, keep);
  return launch_done(fn);
}

}  // extern "C"
