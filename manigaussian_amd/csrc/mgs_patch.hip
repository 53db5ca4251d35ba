// mgs_patch.hip -- the Perceiver's patch embedding (agents/manigaussian_bc/perceiver_lang_io.py:235: patchify = Conv3DBlock(128, 128,
// kernel_sizes=5, strides=5, activation='relu') on [B,128,100^3], replicate pad 2): a Conv3d whose stride is its kernel, with its pad
// folded into the addressing and bias and ReLU / leaky ReLU in the epilogue, on the exact-f32 MFMA (v_mfma_f32_32x32x2_f32; operand
// layout: mgs_dense.hip).  k = stride, cubic, 2..5; pad 0..k-1 on every side, replicate (a clamp) or zeros (a mask); dilation 1, groups
// 1, fp32, NCDHW; Cin a multiple of 8 in 8..256, Cout a multiple of 32 in 32..256.  O = (D + 2 pad - k) / k + 1 per dimension, input
// coordinate of (output o, tap t): i = o k + t - pad.  With z the pre-activation and act(z) = z > 0 ? z : slope z (or the identity):
//   forward          y[b,co,o]     = act(bias[co] + sum_ci sum_t w[co,ci,t] x[b,ci,i(o,t)])
//   g'               = g_y (y > 0 ? 1 : slope), read off y
//   backward-data    dx[b,ci,i]    = sum over the (o,t) that map onto i, sum_co w[co,ci,t] g'[b,co,o]
//   backward-weight  dw[co,ci,t]   = sum_b sum_o g'[b,co,o] x[b,ci,i(o,t)]            db[co] = sum_b sum_o g'[b,co,o]
//
// No input voxel belongs to two patches, so all three passes are plain GEMMs over the PATCHES.  Every kernel takes its patches PC_MT =
// 32 at a time, consecutive in linear (od, oh, ow) order inside one batch entry (a 20-wide row of patches wastes only the last tile):
// narrow column tiles, not a split of K -- at [1,128,100^3] that is 250 tiles x 128 channels for the forward, one workgroup per CU,
// and no partial sum ever has to be combined.
//
// Forward (pc_fwd_kernel).  C [Cout x patches] = W [Cout x Cin k^3] X [Cin k^3 x patches].  A workgroup of 4 waves takes PC_NT = 128
// output channels x 32 patches, one 32 x 32 accumulator per wave.  The k loop runs over STAGES of PC_KS = 8 input channels at one
// (kd, kh): 8 k rows of the k taps along W.  Thread p k + kw loads patch p's tap kw of the 8 channels -- consecutive threads read
// consecutive floats of a W-row, clamped or masked -- into an LDS slab [8 k][32]; the weights come from the workspace, where a prep
// launch laid them out [stage][8 k][Cout padded to 128], 16 bytes per thread and load, through a slab [8 k][160] (the two lane
// halves' rows lie 32 banks apart in both slabs).  The next stage's values are in flight while this stage's 4 k MFMAs run; one
// barrier per stage.
//
// Backward-data (pc_bwd_data_kernel).  C [(ci, tap) x patches] = W^T [(ci, tap) x Cout] G' [Cout x patches].  A workgroup takes 32
// patches and up to PC_CG = 32 input channels; g' of its patches lies in LDS [Cout][32] for the whole kernel; A is read from w where
// it lies (the taps of one (co, ci) are consecutive: a lane half reads 128 contiguous bytes).  128 rows at a time -- the k^3 taps,
// padded to a multiple of 32, of 1 (k = 5), 2 (k = 4) or 4 (k = 2, 3) channels -- go through an LDS tile [128][40], and then the
// workgroup walks the voxels ITS patches own, W-row by W-row, and writes each once: the sum of its taps in ascending tap order (one
// tap in the interior, up to (pad + 1)^3 on a replicate border) or zero for a voxel past the last patch.  Patch o owns, per
// dimension, the voxels from o k - pad (0 for the first) to (o + 1) k - pad - 1 (D - 1 for the last): a partition, so nothing is
// zeroed beforehand and nothing is added across workgroups.
//
// Backward-weight and -bias (pc_bwd_weight_kernel; merge: mgs_records.hip).  C [Cout x (ci, tap)] = G' [Cout x patches] X~ [patches x
// (ci, tap)].  A workgroup takes 128 output channels x 128 columns (the padded taps of 1, 2 or 4 input channels), 2 x 2 accumulators
// per wave; a k slab is one tile of 32 patches: g' as [128][33], the patches' voxels as [(channel, tap)][33].  The tiles, in their
// linear order, are cut into nrec <= MAX_REC runs whose number and length depend on the shape alone; a run's sums go to its RECORD
// [Cout, Cin k^3 + 1] (the last column, db, by the workgroups of the first N-tile, summed in double) and the merge launch adds the
// records in ascending order in double.  `split` is the number of workgroups that share an N-tile's runs.
//
// No atomics, no workgroup waits for another, nothing to zero.  Element offsets are 64-bit; indices inside a (batch, channel) row are
// 32-bit.
#include "mgs_common.h"

namespace mgs {

typedef float pc_f32x16 __attribute__((ext_vector_type(16)));
typedef float pc_f32x4 __attribute__((ext_vector_type(4)));

constexpr int PC_THREADS = 256;
constexpr int PC_MT = 32;          // patches per tile (every pass)
constexpr int PC_NT = 128;         // forward and weight gradient: output channels per workgroup
constexpr int PC_KS = 8;           // forward: input channels per stage
constexpr int PC_WROW = PC_NT + 32;    // forward: floats of a weight slab row in LDS
constexpr int PC_CG = 32;          // backward-data: most input channels per workgroup
constexpr int PC_ROWS = 128;       // backward-data: rows (channel, tap) of one LDS tile; weight gradient: columns of an N-tile
constexpr int PC_RP = 40;          // backward-data: floats of a row of that tile
constexpr int PC_GP = PC_MT + 1;   // weight gradient: floats of a row of g' and of the voxels in LDS
constexpr size_t PC_REC_BYTES = (size_t)64 << 20;   // the records' workspace: as many as fit these bytes (at least 2, at most MAX_REC)
constexpr int PC_MIN_K = 2, PC_MAX_K = 5, PC_MAX_C = 256;

constexpr int pc_taps_padded(int K) { return (K * K * K + 31) / 32 * 32; }

struct PcGeom {
  int Cin, Cout, CoutPad;
  int pad, zeros;
  int D, H, W, Do, Ho, Wo;
  int M;                       // patches of a batch entry
  int64_t vin;                 // elements of an input (batch, channel) row
  int act;
  float slope;
  // the weight gradient's runs
  int want_dw;
  uint32_t tpb, nitems, nrec, per;   // tiles per batch entry, tiles, records, tiles per record
};

// the voxels patch o of O owns along a dimension of D
__device__ __forceinline__ int pc_own_lo(int o, int K, int pad) { return o == 0 ? 0 : o * K - pad; }
__device__ __forceinline__ int pc_own_hi(int o, int O, int D, int K, int pad) { return o == O - 1 ? D - 1 : (o + 1) * K - pad - 1; }
// the taps of its owner o that map onto voxel i: [lo, hi], empty (1, 0) for a voxel past the last patch
__device__ __forceinline__ void pc_taps(int i, int o, int D, int K, int pad, int zeros, int* lo, int* hi) {
  const int t0 = i + pad - o * K;
  if (t0 >= K) { *lo = 1; *hi = 0; return; }
  *lo = (!zeros && i == 0) ? 0 : t0;
  *hi = (!zeros && i == D - 1) ? K - 1 : t0;
}

// ---- the weights in the order the forward's k loop consumes them -----------------------------------------------------------------
// wp[(stage * 8 k + kk) * CoutPad + co], stage = ((ci / 8) * k + kd) * k + kh, kk = (ci % 8) * k + kw; zeros for co >= Cout
__global__ __launch_bounds__(PC_THREADS) void pc_prep_kernel(int K, int Cin, int Cout, int CoutPad, uint32_t total,
                                                             const float* __restrict__ w, float* __restrict__ wp) {
  const uint32_t e = blockIdx.x * (uint32_t)PC_THREADS + threadIdx.x;
  if (e >= total) return;
  const int KR = PC_KS * K, K3 = K * K * K;
  const int row = (int)(e / (uint32_t)CoutPad), co = (int)(e - (uint32_t)row * (uint32_t)CoutPad);
  const int st = row / KR, kk = row - st * KR, cil = kk / K, kw = kk - cil * K;
  const int cg = st / (K * K), r = st - cg * (K * K), kd = r / K, kh = r - kd * K;
  const int ci = cg * PC_KS + cil, tap = (kd * K + kh) * K + kw;
  wp[e] = co < Cout ? w[((int64_t)co * Cin + ci) * K3 + tap] : 0.f;
}

// ---- forward -----------------------------------------------------------------------------------------------------------------------
// grid = (patch tiles, N-tiles, B)
template <int K>
__global__ __launch_bounds__(PC_THREADS, 2) void pc_fwd_kernel(PcGeom g, const float* __restrict__ x, const float* __restrict__ wp,
                                                               const float* __restrict__ bias, float* __restrict__ y) {
  constexpr int KR = PC_KS * K;   // k rows of a stage
  __shared__ __attribute__((aligned(16))) float ws[2][KR * PC_WROW];
  __shared__ float xs[2][KR * PC_MT];
  const int t = threadIdx.x, lane = t & 63, lj = lane & 31, kh2 = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int n0 = (int)blockIdx.y * PC_NT, b = (int)blockIdx.z, m0 = (int)blockIdx.x * PC_MT;
  const bool live = n0 + wave * 32 < g.Cout;   // (uniform across the wave)

  // the thread's column of the voxel slab: patch p, tap kw along W
  const bool xcol = t < PC_MT * K;
  const int p = xcol ? t / K : 0, kw = xcol ? t - p * K : 0;
  int d0, h0, iw;
  bool wok;
  {
    const int v = min(m0 + p, g.M - 1);   // (a patch past the last one reads the last one's voxels and is not stored)
    const int od = v / (g.Ho * g.Wo), r = v - od * (g.Ho * g.Wo), oh = r / g.Wo, ow = r - oh * g.Wo;
    d0 = od * K - g.pad; h0 = oh * K - g.pad;
    iw = ow * K + kw - g.pad;
    wok = (unsigned)iw < (unsigned)g.W;
    iw = min(max(iw, 0), g.W - 1);
  }
  const float* xb = x + (int64_t)b * g.Cin * g.vin;
  const int srow = t >> 5, scol = (t & 31) * 4;
  const float* wsrc = wp + (int64_t)srow * g.CoutPad + n0 + scol;
  const int64_t wstage = (int64_t)KR * g.CoutPad;
  const int nst = (g.Cin / PC_KS) * K * K;

  pc_f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  float xv[PC_KS];
  pc_f32x4 wv[K];
  auto load = [&](int st) {
    const float* wl = wsrc + (int64_t)st * wstage;
#pragma unroll
    for (int i = 0; i < K; ++i) wv[i] = *reinterpret_cast<const pc_f32x4*>(wl + (int64_t)(8 * i) * g.CoutPad);
    if (xcol) {
      const int cg = st / (K * K), r = st - cg * (K * K), kd = r / K, kh = r - kd * K;
      int id = d0 + kd, ih = h0 + kh;
      const bool ok = wok && (unsigned)id < (unsigned)g.D && (unsigned)ih < (unsigned)g.H;
      id = min(max(id, 0), g.D - 1); ih = min(max(ih, 0), g.H - 1);
      const float* src = xb + (int64_t)cg * PC_KS * g.vin + ((int64_t)id * g.H + ih) * g.W + iw;
      const bool drop = g.zeros && !ok;
#pragma unroll
      for (int c = 0; c < PC_KS; ++c) {
        const float val = src[(int64_t)c * g.vin];
        xv[c] = drop ? 0.f : val;
      }
    }
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int i = 0; i < K; ++i) *reinterpret_cast<pc_f32x4*>(&ws[buf][(srow + 8 * i) * PC_WROW + scol]) = wv[i];
    if (xcol) {
#pragma unroll
      for (int c = 0; c < PC_KS; ++c) xs[buf][(c * K + kw) * PC_MT + p] = xv[c];
    }
  };
  load(0);
  store(0);
  __syncthreads();
  for (int st = 0; st < nst; ++st) {
    const int cur = st & 1;
    const bool more = st + 1 < nst;
    if (more) load(st + 1);   // the next stage's operands, in flight while this stage is used
    if (live) {
      const float* wrow = &ws[cur][kh2 * PC_WROW + wave * 32 + lj];
      const float* xrow = &xs[cur][kh2 * PC_MT + lj];
#pragma unroll
      for (int s = 0; s < KR / 2; ++s)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wrow[2 * s * PC_WROW], xrow[2 * s * PC_MT], acc, 0, 0, 0);
    }
    if (more) store(cur ^ 1);
    __syncthreads();
  }

  // bias, activation, store: a register of C is 32 consecutive patches of one channel
  const int v = m0 + lj;
  if (!live || v >= g.M) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int co = n0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh2;
    float val = acc[r] + (bias ? bias[co] : 0.f);
    if (g.act) val = val > 0.f ? val : val * g.slope;
    y[((int64_t)b * g.Cout + co) * g.M + v] = val;
  }
}

// ---- backward-data -------------------------------------------------------------------------------------------------------------------
// grid = (patch tiles, groups of PC_CG input channels, B)
template <int K>
__global__ __launch_bounds__(PC_THREADS, 2) void pc_bwd_data_kernel(PcGeom g, const float* __restrict__ gy, const float* __restrict__ y,
                                                                    const float* __restrict__ w, float* __restrict__ dx) {
  constexpr int K3 = K * K * K, TP = pc_taps_padded(K), CPB = PC_ROWS / TP, BX = 2 * K - 1;
  __shared__ float gs[PC_MAX_C * PC_MT];
  __shared__ float rs[PC_ROWS * PC_RP];
  const int t = threadIdx.x, lane = t & 63, lj = lane & 31, kh2 = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int b = (int)blockIdx.z, m0 = (int)blockIdx.x * PC_MT, np = min(PC_MT, g.M - m0);
  const int c_begin = (int)blockIdx.y * PC_CG, c_end = min(g.Cin, c_begin + PC_CG);

  {   // g' of the tile: row co, zeros for a patch that is not there
    const int p = t & 31;
    for (int co = t >> 5; co < g.Cout; co += PC_THREADS / 32) {
      float val = 0.f;
      if (p < np) {
        const int64_t idx = ((int64_t)b * g.Cout + co) * g.M + m0 + p;
        val = gy[idx];
        if (g.act) val = y[idx] > 0.f ? val : val * g.slope;
      }
      gs[co * PC_MT + p] = val;
    }
  }
  __syncthreads();

  // the lane's row of a tile: (channel of the tile, tap); a padding row reads tap 0 and is never looked at
  const int row = wave * 32 + lj, chl_a = row / TP, tap_a = row - chl_a * TP;
  const int64_t wstep = (int64_t)2 * g.Cin * K3;   // two output channels on
  const int ns = g.Cout / 2;                       // (a multiple of 16)
  // the rows of patches the tile touches
  const int q0 = m0 / g.Wo, q1 = (m0 + np - 1) / g.Wo;
  const int nseg = (q1 - q0 + 1) * BX * BX * CPB;

  for (int cb = c_begin; cb < c_end; cb += CPB) {
    pc_f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const float* wl = w + ((int64_t)kh2 * g.Cin + cb + chl_a) * K3 + (tap_a < K3 ? tap_a : 0);
    const float* gl = &gs[kh2 * PC_MT + lj];
    float ac[8], an[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) ac[j] = wl[(int64_t)j * wstep];
    for (int s0 = 0; s0 < ns; s0 += 8) {
      const bool more = s0 + 8 < ns;
      if (more) {
#pragma unroll
        for (int j = 0; j < 8; ++j) an[j] = wl[(int64_t)(s0 + 8 + j) * wstep];
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ac[j], gl[2 * (s0 + j) * PC_MT], acc, 0, 0, 0);
      if (more) {
#pragma unroll
        for (int j = 0; j < 8; ++j) ac[j] = an[j];
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) rs[(wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh2) * PC_RP + lj] = acc[r];
    __syncthreads();

    // the voxels the tile's patches own, a W-row of one channel per wave and turn
    for (int s = wave; s < nseg; s += PC_THREADS / 64) {
      const int chl = s % CPB;
      int u = s / CPB;
      const int hh = u % BX; u /= BX;
      const int dd = u % BX;
      const int q = q0 + u / BX;
      const int od = q / g.Ho, oh = q - od * g.Ho;
      const int d = pc_own_lo(od, K, g.pad) + dd, h = pc_own_lo(oh, K, g.pad) + hh;
      if (d > pc_own_hi(od, g.Do, g.D, K, g.pad) || h > pc_own_hi(oh, g.Ho, g.H, K, g.pad)) continue;
      const int oa = max(m0, q * g.Wo) - q * g.Wo, ob = min(m0 + np - 1, q * g.Wo + g.Wo - 1) - q * g.Wo;
      const int wbeg = pc_own_lo(oa, K, g.pad), wend = pc_own_hi(ob, g.Wo, g.W, K, g.pad);
      int dlo, dhi, hlo, hhi;
      pc_taps(d, od, g.D, K, g.pad, g.zeros, &dlo, &dhi);
      pc_taps(h, oh, g.H, K, g.pad, g.zeros, &hlo, &hhi);
      float* out = dx + ((int64_t)b * g.Cin + cb + chl) * g.vin + ((int64_t)d * g.H + h) * g.W;
      const float* rc = &rs[chl * TP * PC_RP];
      for (int wi = wbeg + lane; wi <= wend; wi += 64) {
        const int ow = min((wi + g.pad) / K, g.Wo - 1);
        int wlo, whi;
        pc_taps(wi, ow, g.W, K, g.pad, g.zeros, &wlo, &whi);
        const int col = q * g.Wo + ow - m0;
        float sum = 0.f;
        for (int td = dlo; td <= dhi; ++td)
          for (int th = hlo; th <= hhi; ++th)
            for (int tw = wlo; tw <= whi; ++tw) sum += rc[((td * K + th) * K + tw) * PC_RP + col];
        out[wi] = sum;
      }
    }
    __syncthreads();
  }
}

// ---- backward-weight and -bias -------------------------------------------------------------------------------------------------------
// grid = (N-tiles -- or 1 when dw is not wanted: then x is not read --, M-tiles, workgroups that share the runs)
template <int K>
__global__ __launch_bounds__(PC_THREADS, 2) void pc_bwd_weight_kernel(PcGeom g, const float* __restrict__ x, const float* __restrict__ y,
                                                                      const float* __restrict__ gy, float* __restrict__ records) {
  constexpr int K3 = K * K * K, TP = pc_taps_padded(K), CPB = PC_ROWS / TP;
  __shared__ float gs[PC_NT * PC_GP];
  __shared__ float xs[CPB * K3 * PC_GP];
  const int t = threadIdx.x, lane = t & 63, lj = lane & 31, kh2 = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6), wm = wave & 1, wn = wave >> 1;
  const int ci0 = (int)blockIdx.x * CPB, co0 = (int)blockIdx.y * PC_NT;
  const int cols = g.Cin * K3 + 1;

  // the lane's two columns: (channel of the tile, tap), where they lie in the voxel slab, and where they go in a record's row
  int xoff[2], col[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int n = wn * 64 + s * 32 + lj, chl = n / TP, tap = n - chl * TP;
    const bool valid = tap < K3;
    xoff[s] = valid ? (chl * K3 + tap) * PC_GP : 0;
    col[s] = valid ? (ci0 + chl) * K3 + tap : -1;
  }
  const int aoff = (wm * 64 + lj) * PC_GP;
  bool live[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) live[s] = co0 + wm * 64 + s * 32 < g.Cout;   // (uniform across the wave)
  const bool sums_b = blockIdx.x == 0 && t < PC_NT;
  const bool xcol = t < PC_MT * K;
  const int p = xcol ? t / K : 0, kw = xcol ? t - p * K : 0;

  for (uint32_t rec = blockIdx.z; rec < g.nrec; rec += gridDim.z) {
    pc_f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    double bsum = 0.0;
    const uint32_t i0 = rec * g.per, i1 = min(i0 + g.per, g.nitems);
    for (uint32_t item = i0; item < i1; ++item) {
      const int b = (int)(item / g.tpb), m0 = (int)(item - (uint32_t)b * g.tpb) * PC_MT, np = min(PC_MT, g.M - m0);
      __syncthreads();   // (the last tile is no longer read)
      {   // g' of the tile: row co, zeros for a channel or a patch that is not there
        const int pp = t & 31;
#pragma unroll 4
        for (int i = 0; i < PC_NT / 8; ++i) {
          const int c = (t >> 5) + 8 * i, co = co0 + c;
          float val = 0.f;
          if (co < g.Cout && pp < np) {
            const int64_t idx = ((int64_t)b * g.Cout + co) * g.M + m0 + pp;
            val = gy[idx];
            if (g.act) val = y[idx] > 0.f ? val : val * g.slope;
          }
          gs[c * PC_GP + pp] = val;
        }
      }
      if (g.want_dw && xcol) {   // the patches' voxels, zeros for a patch that is not there (uniform across the launch)
        const bool there = p < np;
        const int v = min(m0 + p, g.M - 1);
        const int od = v / (g.Ho * g.Wo), r = v - od * (g.Ho * g.Wo), oh = r / g.Wo, ow = r - oh * g.Wo;
        int iw = ow * K + kw - g.pad;
        const bool wok = (unsigned)iw < (unsigned)g.W;
        iw = min(max(iw, 0), g.W - 1);
        for (int chl = 0; chl < CPB; ++chl) {
          const float* xc = x + ((int64_t)b * g.Cin + ci0 + chl) * g.vin + iw;
#pragma unroll
          for (int kd = 0; kd < K; ++kd) {
            int id = od * K + kd - g.pad;
            const bool dok = (unsigned)id < (unsigned)g.D;
            id = min(max(id, 0), g.D - 1);
#pragma unroll
            for (int kh = 0; kh < K; ++kh) {
              int ih = oh * K + kh - g.pad;
              const bool ok = wok && dok && (unsigned)ih < (unsigned)g.H;
              ih = min(max(ih, 0), g.H - 1);
              const float val = xc[((int64_t)id * g.H + ih) * g.W];
              xs[(chl * K3 + (kd * K + kh) * K + kw) * PC_GP + p] = (!there || (g.zeros && !ok)) ? 0.f : val;
            }
          }
        }
      }
      __syncthreads();
      if (sums_b) {
        double s = 0.0;
        for (int v = 0; v < np; ++v) s += (double)gs[t * PC_GP + v];
        bsum += s;
      }
      if (g.want_dw) {
        const int ks = (np + 1) >> 1;   // (an odd tile's last step multiplies a zero of g')
        for (int k = 0; k < ks; ++k) {
          const int v = 2 * k + kh2;
          const float a0 = gs[aoff + v], a1 = gs[aoff + 32 * PC_GP + v];
          const float b0 = xs[xoff[0] + v], b1 = xs[xoff[1] + v];
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
            const int co = co0 + wm * 64 + sm * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh2;
            if (co < g.Cout) rp[(int64_t)co * cols + col[sn]] = acc[sm][sn][r];
          }
        }
      }
    }
    if (sums_b && co0 + t < g.Cout) rp[(int64_t)(co0 + t) * cols + cols - 1] = (float)bsum;
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
struct PcShape {
  int64_t B, Do, Ho, Wo, M, vin, tpb, nitems, nrec, per;
  int K3;
  size_t wp_bytes, rec_bytes;
};

static int pc_pad_to(int c) { return (c + PC_NT - 1) / PC_NT * PC_NT; }

static bool pc_shape(int64_t B, int Cin, int Cout, int K, int pad, int64_t Di, int64_t Hi, int64_t Wi, PcShape* sh, const char** why) {
  if (K < PC_MIN_K || K > PC_MAX_K) { *why = "k (the kernel and the stride) must be 2 to 5"; return false; }
  if (pad < 0 || pad >= K) { *why = "pad must be 0 to k - 1"; return false; }
  if (Cin < PC_KS || Cin > PC_MAX_C || Cin % PC_KS) { *why = "Cin must be a multiple of 8 in 8 to 256"; return false; }
  if (Cout < 32 || Cout > PC_MAX_C || Cout % 32) { *why = "Cout must be a multiple of 32 in 32 to 256"; return false; }
  if (B < 1) { *why = "B must be at least 1"; return false; }
  if (Di < 1 || Hi < 1 || Wi < 1) { *why = "every extent must be at least 1"; return false; }
  if (row_too_long(Di, Hi, Wi)) { *why = "a (batch, channel) row must hold fewer than 2^31 elements"; return false; }
  if (Di + 2 * pad < K || Hi + 2 * pad < K || Wi + 2 * pad < K) { *why = "every padded extent must be at least k: there is no patch"; return false; }
  if (B > 65535) { *why = "B exceeds the 65535 tiles of a grid's third dimension"; return false; }
  sh->B = B; sh->K3 = K * K * K;
  sh->Do = (Di + 2 * pad - K) / K + 1; sh->Ho = (Hi + 2 * pad - K) / K + 1; sh->Wo = (Wi + 2 * pad - K) / K + 1;
  sh->vin = Di * Hi * Wi; sh->M = sh->Do * sh->Ho * sh->Wo;   // (at most the row's voxels)
  if (B * sh->M > (int64_t)0x7fffffff) { *why = "B Do Ho Wo, the patches, must stay below 2^31"; return false; }
  sh->tpb = (sh->M + PC_MT - 1) / PC_MT;
  sh->nitems = B * sh->tpb;
  sh->rec_bytes = (size_t)Cout * ((size_t)Cin * sh->K3 + 1) * sizeof(float);
  int64_t want = (int64_t)(PC_REC_BYTES / sh->rec_bytes);
  want = want < 2 ? 2 : (want > MAX_REC ? MAX_REC : want);
  const Runs runs = cut_runs(sh->nitems, want);
  sh->nrec = runs.n; sh->per = runs.per;
  sh->wp_bytes = align_up((size_t)Cin * sh->K3 * pc_pad_to(Cout) * sizeof(float));
  return true;
}

static int pc_check(const char* fn, int64_t B, int Cin, int Cout, int K, int pad, int64_t Di, int64_t Hi, int64_t Wi, int zeros, float slope,
                    PcShape* sh) {
  const char* why = "";
  if (!pc_shape(B, Cin, Cout, K, pad, Di, Hi, Wi, sh, &why)) {
    set_error("%s: B = %lld, Cin = %d, Cout = %d, k = %d, pad = %d, Di Hi Wi = %lld x %lld x %lld: %s", fn, (long long)B, Cin, Cout, K, pad,
              (long long)Di, (long long)Hi, (long long)Wi, why);
    return MGS_ERR_INVALID_ARG;
  }
  if (zeros != 0 && zeros != 1) { set_error("%s: zeros_pad = %d (0: replicate, 1: zeros)", fn, zeros); return MGS_ERR_INVALID_ARG; }
  if (slope != slope) { set_error("%s: negative_slope is NaN (below 0: no activation)", fn); return MGS_ERR_INVALID_ARG; }
  return MGS_OK;
}

static PcGeom pc_geom(const PcShape& sh, int Cin, int Cout, int pad, int zeros, int64_t Di, int64_t Hi, int64_t Wi, float slope) {
  PcGeom g;
  g.Cin = Cin; g.Cout = Cout; g.CoutPad = pc_pad_to(Cout);
  g.pad = pad; g.zeros = zeros;
  g.D = (int)Di; g.H = (int)Hi; g.W = (int)Wi; g.Do = (int)sh.Do; g.Ho = (int)sh.Ho; g.Wo = (int)sh.Wo;
  g.M = (int)sh.M; g.vin = sh.vin;
  g.act = slope >= 0.f; g.slope = slope;
  g.want_dw = 0;
  g.tpb = (uint32_t)sh.tpb; g.nitems = (uint32_t)sh.nitems; g.nrec = (uint32_t)sh.nrec; g.per = (uint32_t)sh.per;
  return g;
}

template <typename... A>
static void pc_launch(int K, void (*k2)(A...), void (*k3)(A...), void (*k4)(A...), void (*k5)(A...), dim3 grid, hipStream_t s, A... a) {
  void (*kern)(A...) = K == 2 ? k2 : K == 3 ? k3 : K == 4 ? k4 : k5;
  hipLaunchKernelGGL(kern, grid, dim3(PC_THREADS), 0, s, a...);
}

}  // namespace mgs

using namespace mgs;

extern "C" {

size_t mgs_patch_conv3d_workspace_bytes(int64_t B, int Cin, int Cout, int k, int pad, int64_t Di, int64_t Hi, int64_t Wi) {
  PcShape sh;
  const char* why;
  if (!pc_shape(B, Cin, Cout, k, pad, Di, Hi, Wi, &sh, &why)) return 0;
  // the forward's rearranged weights and the backward's records share the bytes: each call writes what it reads
  const size_t rec = align_up((size_t)sh.nrec * sh.rec_bytes);
  return (sh.wp_bytes > rec ? sh.wp_bytes : rec) + ALIGN;
}

int mgs_patch_conv3d_forward(int64_t B, int Cin, int Cout, int k, int pad, int64_t Di, int64_t Hi, int64_t Wi, int zeros_pad,
                             float negative_slope, const float* x, const float* w, const float* bias, float* y, void* workspace,
                             size_t workspace_bytes, mgs_stream_t stream) {
  const char* fn = "patch_conv3d_forward";
  PcShape sh;
  if (int rc = pc_check(fn, B, Cin, Cout, k, pad, Di, Hi, Wi, zeros_pad, negative_slope, &sh)) return rc;
  if (!x || !w || !y || !workspace) { set_error("%s: NULL x, w, y or workspace", fn); return MGS_ERR_INVALID_ARG; }
  if (misaligned16(x) || misaligned16(w) || misaligned16(y) || misaligned16(bias) || misaligned16(workspace)) {
    set_error("%s: x, w, bias, y and the workspace must be 16-byte aligned", fn);
    return MGS_ERR_INVALID_ARG;
  }
  if (int rc = workspace_short(fn, workspace_bytes, mgs_patch_conv3d_workspace_bytes(B, Cin, Cout, k, pad, Di, Hi, Wi))) return rc;
  hipStream_t s = (hipStream_t)stream;
  float* wp = reinterpret_cast<float*>(workspace);
  const PcGeom g = pc_geom(sh, Cin, Cout, pad, zeros_pad, Di, Hi, Wi, negative_slope);
  const uint32_t total = (uint32_t)Cin * (uint32_t)sh.K3 * (uint32_t)g.CoutPad;
  hipLaunchKernelGGL(pc_prep_kernel, dim3((total + PC_THREADS - 1) / PC_THREADS), dim3(PC_THREADS), 0, s, k, Cin, Cout, g.CoutPad, total, w, wp);
  const dim3 grid((unsigned)sh.tpb, (unsigned)(g.CoutPad / PC_NT), (unsigned)B);
  pc_launch(k, pc_fwd_kernel<2>, pc_fwd_kernel<3>, pc_fwd_kernel<4>, pc_fwd_kernel<5>, grid, s, g, x, (const float*)wp, bias, y);
  return launch_done(fn);
}

int mgs_patch_conv3d_backward(int64_t B, int Cin, int Cout, int k, int pad, int64_t Di, int64_t Hi, int64_t Wi, int zeros_pad,
                              float negative_slope, const float* x, const float* y, const float* g_y, const float* w, float* dx, float* dw,
                              float* db, void* workspace, size_t workspace_bytes, int split, mgs_stream_t stream) {
  const char* fn = "patch_conv3d_backward";
  PcShape sh;
  if (int rc = pc_check(fn, B, Cin, Cout, k, pad, Di, Hi, Wi, zeros_pad, negative_slope, &sh)) return rc;
  if (int rc = split_check(fn, split)) return rc;
  const int act = negative_slope >= 0.f;
  if (!dx && !dw && !db) { set_error("%s: NULL dx, dw and db: no gradient is asked for", fn); return MGS_ERR_INVALID_ARG; }
  if (!g_y || (act && !y) || (dx && !w) || (dw && !x)) {
    set_error("%s: NULL g_y, y (needed with an activation), w (needed for dx) or x (needed for dw)", fn);
    return MGS_ERR_INVALID_ARG;
  }
  if (misaligned16(x) || misaligned16(y) || misaligned16(g_y) || misaligned16(w) || misaligned16(dx) || misaligned16(dw) || misaligned16(db)) {
    set_error("%s: x, y, g_y, w, dx, dw and db must be 16-byte aligned", fn);
    return MGS_ERR_INVALID_ARG;
  }
  if (dw || db) {
    if (int rc = records_workspace(fn, workspace, workspace_bytes, mgs_patch_conv3d_workspace_bytes(B, Cin, Cout, k, pad, Di, Hi, Wi))) return rc;
  }
  hipStream_t s = (hipStream_t)stream;
  PcGeom g = pc_geom(sh, Cin, Cout, pad, zeros_pad, Di, Hi, Wi, negative_slope);
  if (dx) {
    const dim3 grid((unsigned)sh.tpb, (unsigned)((Cin + PC_CG - 1) / PC_CG), (unsigned)B);
    pc_launch(k, pc_bwd_data_kernel<2>, pc_bwd_data_kernel<3>, pc_bwd_data_kernel<4>, pc_bwd_data_kernel<5>, grid, s, g, g_y, y, w, dx);
  }
  if (dw || db) {
    float* records = reinterpret_cast<float*>(workspace);
    g.want_dw = dw != nullptr;
    const int64_t wgs = split_clamp(split, sh.nrec, sh.nrec);
    const int cpb = PC_ROWS / pc_taps_padded(k);
    const dim3 grid((unsigned)(g.want_dw ? Cin / cpb : 1), (unsigned)(g.CoutPad / PC_NT), (unsigned)wgs);
    pc_launch(k, pc_bwd_weight_kernel<2>, pc_bwd_weight_kernel<3>, pc_bwd_weight_kernel<4>, pc_bwd_weight_kernel<5>, grid, s, g, x, y, g_y,
              records);
    launch_records_merge(sh.nrec, Cout, Cin * sh.K3 + 1, Cin * sh.K3, (const float*)records, dw, db, s);
  }
  return launch_done(fn);
}

}  // extern "C"
