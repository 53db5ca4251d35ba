// mgs_dense.hip -- the Perceiver decoder's dense 3x3x3 / 5x5x5 convolutions (agents/manigaussian_bc/perceiver_lang_io.py: up0 =
// Conv3DUpsampleBlock(256, 128, 5), final = Conv3DBlock(256, 128, 3), both lrelu) as implicit GEMMs on the exact-f32 MFMA
// (v_mfma_f32_32x32x2_f32), with bias and leaky ReLU in the epilogue.  Stride 1, no padding ("valid"), dilation 1, groups 1, fp32,
// NCDHW; Cin a multiple of 8 in 8..256, Cout a multiple of 32 in 32..256, k = 3 or 5.  With z the pre-activation and
// act(z) = z > 0 ? z : slope z (or the identity):
//   forward          y[b,co,o]     = act(bias[co] + sum_ci sum_tap w[co,ci,tap] x[b,ci,o + tap])
//   g'               = g_y (z > 0 ? 1 : slope), read off y: y > 0 exactly when z is (slope >= 0)
//   backward-data    dx[b,ci,i]    = sum_co sum_tap w[co,ci,tap] g'[b,co,i - tap]
//   backward-weight  dw[co,ci,tap] = sum_b sum_o g'[b,co,o] x[b,ci,o + tap]            db[co] = sum_b sum_o g'[b,co,o]
//
// The MFMA.  One v_mfma_f32_32x32x2_f32 multiplies A [32 x 2] by B [2 x 32]: lane l gives A[l & 31][l >> 5] and B[l >> 5][l & 31] and
// holds C[(r & 3) + 8 (r >> 2) + 4 (l >> 5)][l & 31] in register r of 16.  It is a k-ordered chain of fused multiply-adds: exact
// on small integers.  C's column lies on the lane, so the operand whose index runs along memory in the RESULT is B: a register of
// C is then 32 consecutive floats of one row.
//
// Forward (dc_fwd_kernel).  Per batch entry C [Cout x voxels] = W [Cout x Cin k^3] X [Cin k^3 x voxels].  A workgroup of 4 waves
// takes DC_NT = 128 output channels x DC_MT = 128 output voxels, consecutive in linear (d, h, w) order (a 100-wide row wastes only
// the last tile); wave (wm, wn) keeps the 2 x 2 accumulators of channels 64 wm.. and voxels 64 wn.. (64 registers).  The k loop
// runs over STAGES of one tap and DC_KS = 8 input channels (4 MFMA k-steps; the two k-values of a step are two channels at the
// same tap).  B is a plain 4-byte global load per lane from where the lane's voxel's window starts (worked out once; a tail voxel
// reads the last voxel's window and is not stored) plus a wave-uniform tap offset plus a channel stride; the next stage's 8 values
// are in flight while this stage's 16 MFMAs run.  A comes from the weights a prep launch rearranged into [stage][8][Cout padded to
// 128] in the workspace (zeros in the padding), one 16-byte load per thread and stage, through two LDS slabs of 8 rows of 160
// floats (the two lane halves' rows then lie 32 banks apart): one barrier per stage.  Sub-tiles of 32 channels beyond Cout are
// skipped (uniform across the wave).
//
// Backward-data is the same kernel: a launch writes g' into a buffer zero-padded by k - 1 on every side (dc_pad_kernel), the prep
// launch writes the flipped, channel-transposed weights, and the forward kernel on those two -- Cout input channels, Cin output
// channels, no bias, no activation -- is dx.  No border case reaches the hot loop.
//
// Backward-weight and -bias (dc_bwd_weight_kernel; merge: mgs_records.hip).  C [Cout x (ci, tap)] = G' [Cout x voxels] X~ [voxels x (ci,
// tap)]: k is the voxel index, which runs along memory in both operands, so both go through LDS.  A k-slab is a SEGMENT of up to
// DC_SEG = 64 voxels of one output row: g' (masked on the way in) lies as 128 rows of 65 floats and is read across the channels;
// of x the k^2 halo rows of the N-tile's channels lie as rows of DC_SEG + k - 1 floats and a lane reads them at its column's own tap
// offset, decoded once.  An N-tile is DC_WN = 128 columns: 4 channels x 27 taps padded to 32 (k = 3) or 1 channel x 125 taps padded to
// 128 (k = 5).  The segments, in their linear order, are cut into nrec <= MAX_REC runs whose number and length depend on the
// shape alone; a run's sums go to its RECORD [Cout, Cin k^3 + 1] in the workspace (the last column, db, by the workgroups of the
// first N-tile, summed in double), and the merge launch adds the records in ascending order in double.  `split` is the number of
// workgroups that share an N-tile's runs: it decides who computes a record, never what it holds.
//
// No atomics, no workgroup waits for another, nothing to zero.  Element offsets are 64-bit; indices inside a (batch, channel) row are
// 32-bit.
#include "mgs_common.h"

namespace mgs {

typedef float dc_f32x16 __attribute__((ext_vector_type(16)));

constexpr int DC_THREADS = 256;
constexpr int DC_MT = 128;        // forward: output voxels per workgroup
constexpr int DC_NT = 128;        // forward: output channels per workgroup (and the weight gradient's M-tile)
constexpr int DC_KS = 8;          // forward: input channels per stage (one tap)
constexpr int DC_WROW = DC_NT + 32;   // floats of a slab row in LDS
constexpr int DC_SEG = 64;        // weight gradient: most voxels of an output row per k-slab
constexpr int DC_GROW = DC_SEG + 1;   // floats of a row of g' in LDS
constexpr int DC_WN = 128;        // weight gradient: columns of an N-tile
constexpr size_t DC_REC_BYTES = (size_t)128 << 20;   // ... and as many as fit these bytes (at least 8)
constexpr int DC_MIN_C = 8, DC_MAX_C = 256;

struct DcGeom {
  int Cin, Cout, CoutPad;      // of the GEMM that runs (backward-data: exchanged)
  int Hi, Wi, Ho, Wo;
  int M;                       // output voxels of a batch entry
  int64_t vin, vout;           // elements of an input and an output (batch, channel) row
  int act;
  float slope;
};

template <int K>
__device__ __forceinline__ int dc_tap_offset(int tap, int Hi, int Wi) {
  const int kd = tap / (K * K), r = tap - kd * (K * K), kh = r / K, kw = r - kh * K;
  return (kd * Hi + kh) * Wi + kw;
}

// ---- the weights in the order the k loop consumes them ------------------------------------------------------------------------------
// wp[(stage * 8 + j) * CoutPad + co], stage = (ci / 8) * k^3 + tap, j = ci % 8; zeros for co >= Cout.  flipped: the weights of
// backward-data, w'[ci][co][tap] = w[co][ci][k^3 - 1 - tap], for the GEMM whose input channels are w's output channels.
__global__ __launch_bounds__(DC_THREADS) void dc_prep_kernel(int K3, int CinG, int CoutG, int CoutPad, int flipped, uint32_t total,
                                                             const float* __restrict__ w, float* __restrict__ wp) {
  const uint32_t e = blockIdx.x * (uint32_t)DC_THREADS + threadIdx.x;
  if (e >= total) return;
  const int row = (int)(e / (uint32_t)CoutPad), co = (int)(e - (uint32_t)row * (uint32_t)CoutPad);
  const int st = row >> 3, j = row & 7, cs = st / K3, tap = st - cs * K3, ci = cs * DC_KS + j;
  float v = 0.f;
  if (co < CoutG) v = flipped ? w[((int64_t)ci * CoutG + co) * K3 + (K3 - 1 - tap)] : w[((int64_t)co * CinG + ci) * K3 + tap];
  // Backward-data multiplies every weight by the zero padding of g': a NaN or infinite weight would put a NaN into every dx the
  // padding connects it to.  It goes into the GEMM as a zero, and dc_dx_nonfinite_kernel adds what it does contribute.
  if (flipped && !(fabsf(v) < INFINITY)) v = 0.f;
  wp[e] = v;
}

// dx += w[co][ci][tap] g'[b][co][i - tap] for the weights that are NaN or infinite, over the voxels i whose i - tap is an output voxel.
// grid = (Cin, B): a workgroup looks through its input channel's Cout k^3 weights and leaves if all are finite (every training step).
// int indices: dc_shape admits rows of fewer than 2^31 elements (vin, and Cout k^3 <= 256 x 125); offsets across rows are 64-bit.
__global__ __launch_bounds__(DC_THREADS) void dc_dx_nonfinite_kernel(int K, int Cin, int Cout, int Di, int Hi, int Wi, int act, float slope,
                                                                     const float* __restrict__ w, const float* __restrict__ gy,
                                                                     const float* __restrict__ y, float* __restrict__ dx) {
  const int ci = (int)blockIdx.x, b = (int)blockIdx.y, K3 = K * K * K, n = Cout * K3;
  int any = 0;
  for (int e = (int)threadIdx.x; e < n; e += DC_THREADS) {
    const int co = e / K3, tap = e - co * K3;
    any |= !(fabsf(w[((int64_t)co * Cin + ci) * K3 + tap]) < INFINITY);
  }
  if (!__syncthreads_or(any)) return;
  const int Do = Di - K + 1, Ho = Hi - K + 1, Wo = Wi - K + 1, vin = Di * Hi * Wi;
  const int64_t vout = (int64_t)Do * Ho * Wo;
  float* dr = dx + ((int64_t)b * Cin + ci) * vin;
  for (int e = 0; e < n; ++e) {   // (uniform; a thread owns the same voxels for every weight: no two threads add to one element)
    const int co = e / K3, tap = e - co * K3;
    const float wv = w[((int64_t)co * Cin + ci) * K3 + tap];
    if (fabsf(wv) < INFINITY) continue;
    const int kd = tap / (K * K), r = tap - kd * (K * K), kh = r / K, kw = r - kh * K;
    const int64_t row = ((int64_t)b * Cout + co) * vout;
    for (int i = (int)threadIdx.x; i < vin; i += DC_THREADS) {
      const int d = i / (Hi * Wi), r2 = i - d * (Hi * Wi), h = r2 / Wi, c = r2 - h * Wi;
      const int od = d - kd, oh = h - kh, ow = c - kw;
      if ((unsigned)od >= (unsigned)Do || (unsigned)oh >= (unsigned)Ho || (unsigned)ow >= (unsigned)Wo) continue;
      const int64_t idx = row + ((int64_t)od * Ho + oh) * Wo + ow;
      float gv = gy[idx];
      if (act) gv = y[idx] > 0.f ? gv : gv * slope;
      dr[i] += wv * gv;
    }
  }
}

// ---- forward (and backward-data) ---------------------------------------------------------------------------------------------------
// grid = (M-tiles, N-tiles, B)
template <int K>
__global__ __launch_bounds__(DC_THREADS, 2) void dc_fwd_kernel(DcGeom g, const float* __restrict__ x, const float* __restrict__ wp,
                                                               const float* __restrict__ bias, float* __restrict__ y) {
  constexpr int K3 = K * K * K;
  __shared__ __attribute__((aligned(16))) float ws[2][DC_KS * DC_WROW];
  const int t = threadIdx.x, lane = t & 63, lj = lane & 31, kh = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6), wm = wave & 1, wn = wave >> 1;
  const int n0 = (int)blockIdx.y * DC_NT, b = (int)blockIdx.z;
  const int m0 = (int)blockIdx.x * DC_MT + wn * 64;

  int voff[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int v = min(m0 + s * 32 + lj, g.M - 1);
    const int od = v / (g.Ho * g.Wo), r = v - od * (g.Ho * g.Wo), oh = r / g.Wo, ow = r - oh * g.Wo;
    voff[s] = (od * g.Hi + oh) * g.Wi + ow;
  }
  bool live[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) live[s] = n0 + wm * 64 + s * 32 < g.Cout;   // (uniform across the wave)
  const float* xl = x + ((int64_t)b * g.Cin + kh) * g.vin;
  const int srow = t >> 5, scol = (t & 31) * 4;
  const float* wsrc = wp + (int64_t)srow * g.CoutPad + n0 + scol;
  const int64_t wstage = (int64_t)DC_KS * g.CoutPad;
  const int nst = (g.Cin / DC_KS) * K3;

  dc_f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  float bc[4][2], bn[4][2];
  auto load_b = [&](float (&bv)[4][2], int st) {
    const int cs = st / K3, tap = st - cs * K3;
    const float* base = xl + (int64_t)cs * DC_KS * g.vin + dc_tap_offset<K>(tap, g.Hi, g.Wi);
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int s = 0; s < 2; ++s) bv[p][s] = base[(int64_t)(2 * p) * g.vin + voff[s]];
  };
  float4 wv = *reinterpret_cast<const float4*>(wsrc);
  load_b(bc, 0);
  *reinterpret_cast<float4*>(&ws[0][srow * DC_WROW + scol]) = wv;
  __syncthreads();
  for (int st = 0; st < nst; ++st) {
    const int cur = st & 1;
    const bool more = st + 1 < nst;
    if (more) {   // the next stage's operands, in flight while this stage is used
      wv = *reinterpret_cast<const float4*>(wsrc + (int64_t)(st + 1) * wstage);
      load_b(bn, st + 1);
    }
    const float* wrow = &ws[cur][kh * DC_WROW + wm * 64 + lj];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const float a0 = wrow[2 * p * DC_WROW], a1 = wrow[2 * p * DC_WROW + 32];
      if (live[0]) {
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bc[p][0], acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bc[p][1], acc[0][1], 0, 0, 0);
      }
      if (live[1]) {
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bc[p][0], acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bc[p][1], acc[1][1], 0, 0, 0);
      }
    }
    if (more) *reinterpret_cast<float4*>(&ws[cur ^ 1][srow * DC_WROW + scol]) = wv;
    __syncthreads();
    if (more) {
#pragma unroll
      for (int p = 0; p < 4; ++p) { bc[p][0] = bn[p][0]; bc[p][1] = bn[p][1]; }
    }
  }

  // bias, activation, store: a register of C is 32 consecutive voxels of one channel
#pragma unroll
  for (int sm = 0; sm < 2; ++sm) {
    if (!live[sm]) continue;
#pragma unroll
    for (int sn = 0; sn < 2; ++sn) {
      const int v = m0 + sn * 32 + lj;
      if (v >= g.M) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = n0 + wm * 64 + sm * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
        if (co >= g.Cout) continue;
        float val = acc[sm][sn][r] + (bias ? bias[co] : 0.f);
        if (g.act) val = val > 0.f ? val : val * g.slope;
        y[((int64_t)b * g.Cout + co) * g.vout + v] = val;
      }
    }
  }
}

// ---- g' = g_y (y > 0 ? 1 : slope), zero-padded by P on every side ---------------------------------------------------------------------
// grid = (blocks over a padded row, rows (b, co) -- walked with the grid's stride)
__global__ __launch_bounds__(DC_THREADS) void dc_pad_kernel(int P, int rows, int Do, int Ho, int Wo, int act, float slope,
                                                            const float* __restrict__ gy, const float* __restrict__ y,
                                                            float* __restrict__ gp) {
  const int Dp = Do + 2 * P, Hp = Ho + 2 * P, Wp = Wo + 2 * P;
  const uint32_t volp = (uint32_t)Dp * (uint32_t)Hp * (uint32_t)Wp;
  const uint32_t e = blockIdx.x * (uint32_t)DC_THREADS + threadIdx.x;
  if (e >= volp) return;
  const int d = (int)(e / (uint32_t)(Hp * Wp)), r = (int)(e - (uint32_t)d * (uint32_t)(Hp * Wp)), h = r / Wp, c = r - h * Wp;
  const int od = d - P, oh = h - P, ow = c - P;
  const bool inside = (unsigned)od < (unsigned)Do && (unsigned)oh < (unsigned)Ho && (unsigned)ow < (unsigned)Wo;
  const int64_t vol = (int64_t)Do * Ho * Wo;
  const int64_t o = inside ? ((int64_t)od * Ho + oh) * Wo + ow : 0;
  for (int row = blockIdx.y; row < rows; row += gridDim.y) {
    float v = 0.f;
    if (inside) {
      v = gy[(int64_t)row * vol + o];
      if (act) v = y[(int64_t)row * vol + o] > 0.f ? v : v * slope;
    }
    gp[(int64_t)row * volp + e] = v;
  }
}

// ---- backward-weight and -bias -------------------------------------------------------------------------------------------------------
struct DcWGeom {
  int Cin, Cout;
  int Do, Ho, Wo, Hi, Wi;
  int spr_row;                 // segments per output row
  uint32_t nseg, nrec, spr;    // segments, records, segments per record
  int64_t vin, vout;
  int act, want_dw;
  float slope;
};

// grid = (N-tiles -- or 1 when dw is not wanted: then x is not read --, M-tiles, workgroups that share the runs)
template <int K>
__global__ __launch_bounds__(DC_THREADS, 2) void dc_bwd_weight_kernel(DcWGeom g, const float* __restrict__ x, const float* __restrict__ y,
                                                                      const float* __restrict__ gy, float* __restrict__ records) {
  constexpr int K3 = K * K * K, KK = K * K;
  constexpr int CH = K == 3 ? 4 : 1;            // channels of an N-tile
  constexpr int XW = DC_SEG + K - 1;            // floats of a halo row
  constexpr int XN = CH * KK * XW;
  static_assert(CH * (K == 3 ? 32 : 128) == DC_WN, "an N-tile is the channels' padded taps");
  __shared__ float gs[DC_NT * DC_GROW];
  __shared__ float xs[XN];
  const int t = threadIdx.x, lane = t & 63, lj = lane & 31, kh = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6), wm = wave & 1, wn = wave >> 1;
  const int ci0 = (int)blockIdx.x * CH, co0 = (int)blockIdx.y * DC_NT;
  const int cols = g.Cin * K3 + 1;

  // the lane's two columns: (channel of the tile, tap), where they read the halo rows, and where they go in a record's row
  int xoff[2], col[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int n = wn * 64 + s * 32 + lj;
    const int chl = K == 3 ? n >> 5 : 0, tap = K == 3 ? n & 31 : n;
    const bool valid = tap < K3;
    const int kd = tap / KK, r = tap - kd * KK, k2 = r / K, kw = r - k2 * K;
    xoff[s] = valid ? (chl * KK + kd * K + k2) * XW + kw : 0;
    col[s] = valid ? (ci0 + chl) * K3 + tap : -1;
  }
  const int aoff = (wm * 64 + lj) * DC_GROW;
  bool live[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) live[s] = co0 + wm * 64 + s * 32 < g.Cout;   // (uniform across the wave)
  const bool sums_b = blockIdx.x == 0 && t < DC_NT;

  for (uint32_t rec = blockIdx.z; rec < g.nrec; rec += gridDim.z) {
    dc_f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    double bsum = 0.0;
    const uint32_t s0 = rec * g.spr, s1 = min(s0 + g.spr, g.nseg);
    for (uint32_t seg = s0; seg < s1; ++seg) {
      uint32_t q = seg;
      const int sw = (int)(q % (uint32_t)g.spr_row); q /= (uint32_t)g.spr_row;
      const int oh = (int)(q % (uint32_t)g.Ho); q /= (uint32_t)g.Ho;
      const int od = (int)(q % (uint32_t)g.Do);
      const int b = (int)(q / (uint32_t)g.Do);
      const int w0 = sw * DC_SEG, nv = min(DC_SEG, g.Wo - w0);
      __syncthreads();   // (the last segment is no longer read)
      {   // g' of the segment: row co, zeros for a channel or a voxel that is not there
        const int v = t & 63;
        const int64_t o = ((int64_t)od * g.Ho + oh) * g.Wo + w0 + v;
#pragma unroll 8
        for (int i = 0; i < DC_NT / 4; ++i) {
          const int c = (t >> 6) + 4 * i, co = co0 + c;
          float val = 0.f;
          if (co < g.Cout && v < nv) {
            const int64_t idx = ((int64_t)b * g.Cout + co) * g.vout + o;
            val = gy[idx];
            if (g.act) val = y[idx] > 0.f ? val : val * g.slope;
          }
          gs[c * DC_GROW + v] = val;
        }
      }
      if (g.want_dw) {   // the halo rows of x: zeros past the segment's last tap (uniform across the launch)
        for (int e = t; e < XN; e += DC_THREADS) {
          const int rowi = e / XW, c = e - rowi * XW, chl = rowi / KK, rr = rowi - chl * KK, kd = rr / K, k2 = rr - kd * K;
          float val = 0.f;
          if (c < nv + K - 1)
            val = x[((int64_t)b * g.Cin + ci0 + chl) * g.vin + ((int64_t)(od + kd) * g.Hi + oh + k2) * g.Wi + w0 + c];
          xs[e] = val;
        }
      }
      __syncthreads();
      if (sums_b) {
        double s = 0.0;
        for (int v = 0; v < nv; ++v) s += (double)gs[t * DC_GROW + v];
        bsum += s;
      }
      if (g.want_dw) {
        const int ks = (nv + 1) >> 1;   // (an odd segment's last step multiplies a zero of g' ...)
        for (int k = 0; k < ks; ++k) {
          const int v = 2 * k + kh;
          const float a0 = gs[aoff + v], a1 = gs[aoff + 32 * DC_GROW + v];
          // (... by a zero, not by the next voxel's x: 0 x NaN or 0 x inf would put a NaN into sums that voxel has no part in)
          const bool there = v < nv;
          const float b0 = there ? xs[xoff[0] + v] : 0.f, b1 = there ? xs[xoff[1] + v] : 0.f;
          if (live[0]) {
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
          }
          if (live[1]) {
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
          }
        }
      }
    }
    // the run's record
    float* rp = records + (int64_t)rec * g.Cout * cols;
    if (g.want_dw) {
#pragma unroll
      for (int sm = 0; sm < 2; ++sm) {
        if (!live[sm]) continue;
#pragma unroll
        for (int sn = 0; sn < 2; ++sn) {
          if (col[sn] < 0) continue;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int co = co0 + wm * 64 + sm * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
            if (co < g.Cout) rp[(int64_t)co * cols + col[sn]] = acc[sm][sn][r];
          }
        }
      }
    }
    if (sums_b && co0 + t < g.Cout) rp[(int64_t)(co0 + t) * cols + cols - 1] = (float)bsum;
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
struct DcShape {
  int64_t B, Di, Hi, Wi, Do, Ho, Wo, vin, vout, vpad;
  int Cin, Cout, K, K3;
  int64_t mtiles, mtiles_dx;
  int64_t spr_row, nseg, nrec, spr;   // the segments and records of dw | db
  size_t wp_bytes, rec_bytes;
};

static int dc_pad_to(int c) { return (c + DC_NT - 1) / DC_NT * DC_NT; }

static bool dc_shape(int64_t B, int Cin, int Cout, int K, int64_t Di, int64_t Hi, int64_t Wi, DcShape* sh, const char** why) {
  if (K != 3 && K != 5) { *why = "k must be 3 or 5"; return false; }
  if (Cin < DC_MIN_C || Cin > DC_MAX_C || Cin % 8) { *why = "Cin must be a multiple of 8 in 8 to 256"; return false; }
  if (Cout < 32 || Cout > DC_MAX_C || Cout % 32) { *why = "Cout must be a multiple of 32 in 32 to 256"; return false; }
  if (B < 1) { *why = "B must be at least 1"; return false; }
  if (Di < K || Hi < K || Wi < K) { *why = "every extent must be at least k"; return false; }
  // (backward-data pads the output gradient to extents of Di + k - 1: that row is the longest one there is)
  const int64_t Dp = Di + K - 1, Hp = Hi + K - 1, Wp = Wi + K - 1;
  if (row_too_long(Dp, Hp, Wp)) {
    *why = "a (batch, channel) row, padded by k - 1, must hold fewer than 2^31 elements";
    return false;
  }
  if (B > 65535) { *why = "B exceeds the 65535 tiles of a grid's third dimension"; return false; }
  sh->B = B; sh->Di = Di; sh->Hi = Hi; sh->Wi = Wi; sh->Cin = Cin; sh->Cout = Cout; sh->K = K; sh->K3 = K * K * K;
  sh->Do = Di - K + 1; sh->Ho = Hi - K + 1; sh->Wo = Wi - K + 1;
  sh->vin = Di * Hi * Wi; sh->vout = sh->Do * sh->Ho * sh->Wo; sh->vpad = Dp * Hp * Wp;
  sh->mtiles = (sh->vout + DC_MT - 1) / DC_MT;
  sh->mtiles_dx = (sh->vin + DC_MT - 1) / DC_MT;
  sh->spr_row = (sh->Wo + DC_SEG - 1) / DC_SEG;
  if (B * sh->Do > (int64_t)0x7fffffff / (sh->Ho * sh->spr_row)) { *why = "the number of row segments (tiles of the weight gradient) exceeds 2^31 - 1"; return false; }
  sh->nseg = B * sh->Do * sh->Ho * sh->spr_row;
  sh->rec_bytes = (size_t)Cout * ((size_t)Cin * sh->K3 + 1) * sizeof(float);
  int64_t want = (int64_t)(DC_REC_BYTES / sh->rec_bytes);
  want = want < 8 ? 8 : (want > MAX_REC ? MAX_REC : want);
  const Runs runs = cut_runs(sh->nseg, want);
  sh->nrec = runs.n; sh->spr = runs.per;
  const size_t fwd = (size_t)Cin * sh->K3 * dc_pad_to(Cout), bwd = (size_t)Cout * sh->K3 * dc_pad_to(Cin);
  sh->wp_bytes = align_up((fwd > bwd ? fwd : bwd) * sizeof(float));
  return true;
}

static int dc_check(const char* fn, int64_t B, int Cin, int Cout, int K, int64_t Di, int64_t Hi, int64_t Wi, float slope, DcShape* sh) {
  const char* why = "";
  if (!dc_shape(B, Cin, Cout, K, Di, Hi, Wi, sh, &why)) {
    set_error("%s: B = %lld, Cin = %d, Cout = %d, k = %d, Di Hi Wi = %lld x %lld x %lld: %s", fn, (long long)B, Cin, Cout, K,
              (long long)Di, (long long)Hi, (long long)Wi, why);
    return MGS_ERR_INVALID_ARG;
  }
  if (slope != slope) { set_error("%s: negative_slope is NaN (below 0: no activation)", fn); return MGS_ERR_INVALID_ARG; }
  return MGS_OK;
}

// the implicit GEMM of `cin` input channels on [B, cin, Hi.., Wi..] -> [B, cout, ...]; wp: the prepared weights
static void dc_launch_gemm(int K, int64_t B, int cin, int cout, int64_t Di, int64_t Hi, int64_t Wi, int act, float slope, const float* x,
                           const float* wp, const float* bias, float* y, hipStream_t s) {
  DcGeom g;
  g.Cin = cin; g.Cout = cout; g.CoutPad = dc_pad_to(cout);
  g.Hi = (int)Hi; g.Wi = (int)Wi; g.Ho = (int)(Hi - K + 1); g.Wo = (int)(Wi - K + 1);
  g.vin = Di * Hi * Wi; g.vout = (Di - K + 1) * (int64_t)g.Ho * g.Wo; g.M = (int)g.vout;
  g.act = act; g.slope = slope;
  const dim3 grid((unsigned)((g.vout + DC_MT - 1) / DC_MT), (unsigned)(g.CoutPad / DC_NT), (unsigned)B);
  if (K == 3) hipLaunchKernelGGL((dc_fwd_kernel<3>), grid, dim3(DC_THREADS), 0, s, g, x, wp, bias, y);
  else hipLaunchKernelGGL((dc_fwd_kernel<5>), grid, dim3(DC_THREADS), 0, s, g, x, wp, bias, y);
}

static void dc_launch_prep(int K3, int cin, int cout, int flipped, const float* w, float* wp, hipStream_t s) {
  const int pad = dc_pad_to(cout);
  const uint32_t total = (uint32_t)cin * (uint32_t)K3 * (uint32_t)pad;
  hipLaunchKernelGGL(dc_prep_kernel, dim3((total + DC_THREADS - 1) / DC_THREADS), dim3(DC_THREADS), 0, s, K3, cin, cout, pad, flipped, total, w,
                     wp);
}

}  // namespace mgs

using namespace mgs;

extern "C" {

size_t mgs_dense_conv3d_workspace_bytes(int64_t B, int Cin, int Cout, int k, int64_t Di, int64_t Hi, int64_t Wi) {
  DcShape sh;
  const char* why;
  if (!dc_shape(B, Cin, Cout, k, Di, Hi, Wi, &sh, &why)) return 0;
  return sh.wp_bytes + align_up((size_t)sh.nrec * sh.rec_bytes) + ALIGN;
}

int mgs_dense_conv3d_forward(int64_t B, int Cin, int Cout, int k, int64_t Di, int64_t Hi, int64_t Wi, float negative_slope, const float* x,
                             const float* w, const float* bias, float* y, void* workspace, size_t workspace_bytes, mgs_stream_t stream) {
  const char* fn = "dense_conv3d_forward";
  DcShape sh;
  if (int rc = dc_check(fn, B, Cin, Cout, k, Di, Hi, Wi, negative_slope, &sh)) return rc;
  if (!x || !w || !y || !workspace) { set_error("%s: NULL x, w, y or workspace", fn); return MGS_ERR_INVALID_ARG; }
  if (misaligned16(x) || misaligned16(w) || misaligned16(y) || misaligned16(bias) || misaligned16(workspace)) {
    set_error("%s: x, w, bias, y and the workspace must be 16-byte aligned", fn);
    return MGS_ERR_INVALID_ARG;
  }
  if (int rc = workspace_short(fn, workspace_bytes, mgs_dense_conv3d_workspace_bytes(B, Cin, Cout, k, Di, Hi, Wi))) return rc;
  hipStream_t s = (hipStream_t)stream;
  float* wp = reinterpret_cast<float*>(workspace);
  dc_launch_prep(sh.K3, Cin, Cout, 0, w, wp, s);
  dc_launch_gemm(k, B, Cin, Cout, Di, Hi, Wi, negative_slope >= 0.f, negative_slope, x, wp, bias, y, s);
  return launch_done(fn);
}

int mgs_dense_conv3d_backward(int64_t B, int Cin, int Cout, int k, int64_t Di, int64_t Hi, int64_t Wi, float negative_slope, const float* x,
                              const float* y, const float* g_y, const float* w, float* dx, float* dw, float* db, float* g_scratch,
                              void* workspace, size_t workspace_bytes, int split, mgs_stream_t stream) {
  const char* fn = "dense_conv3d_backward";
  DcShape sh;
  if (int rc = dc_check(fn, B, Cin, Cout, k, Di, Hi, Wi, negative_slope, &sh)) return rc;
  if (int rc = split_check(fn, split)) return rc;
  const int act = negative_slope >= 0.f;
  if (!dx && !dw && !db) { set_error("%s: NULL dx, dw and db: no gradient is asked for", fn); return MGS_ERR_INVALID_ARG; }
  if (!g_y || (act && !y) || (dx && (!w || !g_scratch)) || (dw && !x) || !workspace) {
    set_error("%s: NULL g_y, y (needed with an activation), w or g_scratch (needed for dx), x (needed for dw) or workspace", fn);
    return MGS_ERR_INVALID_ARG;
  }
  if (misaligned16(x) || misaligned16(y) || misaligned16(g_y) || misaligned16(w) || misaligned16(dx) || misaligned16(dw) || misaligned16(db) ||
      misaligned16(g_scratch) || misaligned16(workspace)) {
    set_error("%s: x, y, g_y, w, dx, dw, db, g_scratch and the workspace must be 16-byte aligned", fn);
    return MGS_ERR_INVALID_ARG;
  }
  if (int rc = workspace_short(fn, workspace_bytes, mgs_dense_conv3d_workspace_bytes(B, Cin, Cout, k, Di, Hi, Wi))) return rc;
  hipStream_t s = (hipStream_t)stream;
  float* wp = reinterpret_cast<float*>(workspace);
  float* records = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + sh.wp_bytes);
  if (dx) {
    const int P = k - 1;
    const int64_t rows = B * Cout;
    const dim3 grid((unsigned)((sh.vpad + DC_THREADS - 1) / DC_THREADS), (unsigned)(rows < 256 ? rows : 256));
    hipLaunchKernelGGL(dc_pad_kernel, grid, dim3(DC_THREADS), 0, s, P, (int)rows, (int)sh.Do, (int)sh.Ho, (int)sh.Wo, act, negative_slope,
                       g_y, y, g_scratch);
    dc_launch_prep(sh.K3, Cout, Cin, 1, w, wp, s);
    dc_launch_gemm(k, B, Cout, Cin, Di + P, Hi + P, Wi + P, 0, 0.f, g_scratch, wp, nullptr, dx, s);
    hipLaunchKernelGGL(dc_dx_nonfinite_kernel, dim3((unsigned)Cin, (unsigned)B), dim3(DC_THREADS), 0, s, k, Cin, Cout, (int)Di, (int)Hi,
                       (int)Wi, act, negative_slope, w, g_y, y, dx);
  }
  if (dw || db) {
    DcWGeom g;
    g.Cin = Cin; g.Cout = Cout;
    g.Do = (int)sh.Do; g.Ho = (int)sh.Ho; g.Wo = (int)sh.Wo; g.Hi = (int)Hi; g.Wi = (int)Wi;
    g.spr_row = (int)sh.spr_row; g.nseg = (uint32_t)sh.nseg; g.nrec = (uint32_t)sh.nrec; g.spr = (uint32_t)sh.spr;
    g.vin = sh.vin; g.vout = sh.vout;
    g.act = act; g.want_dw = dw != nullptr; g.slope = negative_slope;
    const int64_t wgs = split_clamp(split, sh.nrec, sh.nrec);
    const int ch = k == 3 ? 4 : 1;
    const dim3 grid((unsigned)(g.want_dw ? Cin / ch : 1), (unsigned)(dc_pad_to(Cout) / DC_NT), (unsigned)wgs);
    if (k == 3) hipLaunchKernelGGL((dc_bwd_weight_kernel<3>), grid, dim3(DC_THREADS), 0, s, g, x, y, g_y, records);
    else hipLaunchKernelGGL((dc_bwd_weight_kernel<5>), grid, dim3(DC_THREADS), 0, s, g, x, y, g_y, records);
    launch_records_merge(sh.nrec, Cout, Cin * sh.K3 + 1, Cin * sh.K3, records, dw, db, s);
  }
  return launch_done(fn);
}

}  // extern "C"
