// mgs_conv3d.hip -- the voxel encoder stem's 3x3x3 convolutions (helpers/network_utils.py:234-306: nn.Conv3d(k=3, pad=1, stride 1 or
// 2, no bias) and nn.ConvTranspose3d(k=3, pad=1, stride=2, no bias)), direct, fp32, NCDHW, 1..64 channels, VALU only.
//
//   forward          y[b,co,o]   = sum_ci sum_tap w[co,ci,tap] x[b,ci,o s + tap - 1]              O = (I - 1) / s + 1 per dimension
//   backward-data    dx[b,ci,i]  = sum_co sum_{(o,tap): o s + tap - 1 = i} w[co,ci,tap] g[b,co,o]
//   backward-weight  dw[co,ci,tap] = sum_b sum_o g[b,co,o] x[b,ci,o s + tap - 1]
//
// All three are gathers: every output element is written once by one thread from a sum whose terms and order depend on the shape
// alone.  No atomics, no workgroup waits for another, nothing to zero.
//
// Forward (cv_fwd_kernel<S, FLIP>).  A workgroup of 256 threads = 32 lanes along W x 8 rows along H takes an output tile of
// ND x 8 x 32 voxels (ND = 4 at stride 1, 2 at stride 2: the outputs along D a thread keeps in registers) and COG output channels
// (8 at stride 1, 16 at stride 2): ND x COG = 32 accumulators per thread.  The input halo tile of a slab of input channels is staged
// in LDS (out-of-range taps as zeros); at stride 2 a row is stored even columns first, so that the 32 lanes of a row read consecutive
// words for every tap.  Per input channel a thread reads its (ND - 1) S + 3 planes x 9 values once, then runs 27 ND fused
// multiply-adds per output channel against weights whose address is uniform across the wave (scalar loads, SGPR operands).
// Backward-data at stride 1 is the same kernel with the channel roles exchanged and the taps reversed (FLIP).
//
// Backward-data at stride 2 (cv_bwd_data_s2_kernel).  A thread takes one 2x2x2 block of dx (voxels 2m + {0,1} per dimension) and 4
// input channels: per dimension tap 1 feeds the even voxel from g[m], taps 0 and 2 feed the odd one from g[m+1] and g[m], so each of
// the 27 taps is used exactly once per block -- the 1, 2, 4 or 8 terms of the eight parity classes -- from 8 staged values of g.
//
// Backward-weight (cv_bwd_weight_kernel<S>; merge: mgs_records.hip).  The output tiles of the forward, in their linear order, are cut into
// nrec <= 64 runs of tpr tiles; nrec and tpr depend on the shape alone.  A workgroup takes one input channel and 4 output channels
// and, per run, keeps 4 x 27 accumulators per thread over the run's tiles (x from the staged halo tile, g from memory, one voxel
// column per thread), then adds them up over its 256 threads in a fixed order into the run's RECORD [Cout, Cin, 27] in the workspace.
// `split` is the number of workgroups that share a (channel group, input channel)'s runs: it decides who computes a record, not
// what the record is.  The merge launch sums the records in ascending order in double.  dw is the same bits for every split.
//
// Element offsets are 64-bit; indices inside a (batch, channel) row are 32-bit (D H W < 2^31).
#include "mgs_common.h"

namespace mgs {

constexpr int CV_THREADS = 256;
constexpr int CV_TW = 32, CV_TH = 8;       // an output tile's lanes along W and rows along H
constexpr int CV_MAX_C = 64;
constexpr int CV_TARGET_BLOCKS = 2048;
constexpr int CV_BW_COG = 4;               // output channels per workgroup of the weight gradient
constexpr int CV_TAPS = 27;
constexpr int CV_RED_STRIDE = CV_THREADS + 8;   // floats per tap row of the weight gradient's reduction buffer (8 mod 32)

template <int S>
struct CvTile {
  static constexpr int ND = S == 1 ? 4 : 2;           // tile depth = outputs along D per thread
  static constexpr int COG = S == 1 ? 8 : 16;         // forward: output channels per workgroup (ND x COG = 32 accumulators)
  static constexpr int SLAB = S == 1 ? 4 : 2;         // forward: input channels staged at once
  static constexpr int ED = (ND - 1) * S + 3, EH = (CV_TH - 1) * S + 3, EW = (CV_TW - 1) * S + 3;
  static constexpr int PLANE = EH * EW, VOL = ED * PLANE;
  static constexpr int NEVEN = (EW + 1) / 2;
  // where lane tx finds the column of tap kw in a staged row (stride 2 keeps the even columns first: cv_stage_box)
  static __device__ __forceinline__ int tapcol(int tx, int kw) { return S == 1 ? tx + kw : (kw == 1 ? NEVEN + tx : tx + (kw >> 1)); }
};

// One pass's view of the problem: Cl channels are looped over (read), Co are produced; I* are the extents of the staged (read)
// volume for the tile kernels, O* those of the tiled (output-side) volume.
struct CvGeom {
  int B, Cl, Co;
  int ID, IH, IW, OD, OH, OW;
  int tD, tH, tW;          // tiles
  int64_t ivol, ovol;
};

struct CvTilePos { int b, od0, oh0, ow0; };
template <int ND>
__device__ __forceinline__ CvTilePos cv_tile_pos(uint32_t t, const CvGeom& g) {
  CvTilePos p;
  const uint32_t tw = t % (uint32_t)g.tW; t /= (uint32_t)g.tW;
  const uint32_t th = t % (uint32_t)g.tH; t /= (uint32_t)g.tH;
  const uint32_t td = t % (uint32_t)g.tD;
  p.b = (int)(t / (uint32_t)g.tD);
  p.od0 = (int)td * ND; p.oh0 = (int)th * CV_TH; p.ow0 = (int)tw * CV_TW;
  return p;
}

// A box of ED x EH x EW voxels of nch consecutive channels (src = the first one's row, rows chstride apart) whose first voxel is
// (d0, h0, w0) of a volume of nd x nh x nw; voxels outside the volume are zeros.  Eight loads per thread are in flight before the
// first of them is stored (an absent voxel loads the row's first element and drops it: no branch around a load); four in the weight
// gradient, whose accumulators leave no room for more.  S = 2 keeps the even columns of a row first.
template <int ED, int EH, int EW, int S, int CV_STAGE_UNROLL = 8>
__device__ __forceinline__ void cv_stage_box(float* tile, const float* __restrict__ src, int nch, int64_t chstride, int d0, int h0,
                                             int w0, int nd, int nh, int nw) {
  constexpr int PLANE = EH * EW, VOL = ED * PLANE, NEVEN = (EW + 1) / 2;
  const int total = nch * VOL;
  for (int e0 = threadIdx.x; e0 < total; e0 += CV_STAGE_UNROLL * CV_THREADS) {
    float v[CV_STAGE_UNROLL];
    int at[CV_STAGE_UNROLL];
#pragma unroll
    for (int u = 0; u < CV_STAGE_UNROLL; ++u) {
      const int e = e0 + u * CV_THREADS;
      const int k = e / VOL, r0 = e - k * VOL, d = r0 / PLANE, r = r0 - d * PLANE, h = r / EW, c = r - h * EW;
      const int id = d0 + d, ih = h0 + h, iw = w0 + c;
      const bool live = e < total && (unsigned)id < (unsigned)nd && (unsigned)ih < (unsigned)nh && (unsigned)iw < (unsigned)nw;
      const float got = src[live ? (int64_t)k * chstride + ((id * nh + ih) * nw + iw) : (int64_t)0];
      v[u] = live ? got : 0.f;
      const int col = S == 1 ? c : ((c & 1) ? NEVEN + (c >> 1) : (c >> 1));
      at[u] = e < total ? k * VOL + d * PLANE + h * EW + col : -1;
    }
#pragma unroll
    for (int u = 0; u < CV_STAGE_UNROLL; ++u)
      if (at[u] >= 0) tile[at[u]] = v[u];
  }
}

// the halo tiles of nch channels for the output tile at p
template <int S, int UNROLL = 8>
__device__ __forceinline__ void cv_stage(float* tile, const float* __restrict__ src, int nch, const CvTilePos& p, const CvGeom& g) {
  using T = CvTile<S>;
  cv_stage_box<T::ED, T::EH, T::EW, S, UNROLL>(tile, src, nch, g.ivol, p.od0 * S - 1, p.oh0 * S - 1, p.ow0 * S - 1, g.ID, g.IH, g.IW);
}

// ---- forward, and backward-data at stride 1 (FLIP: w is [Cl, Co, 27] read with the taps reversed) ---------------------------------
template <int S, bool FLIP>
__global__ __launch_bounds__(CV_THREADS) void cv_fwd_kernel(CvGeom g, const float* __restrict__ x, const float* __restrict__ w,
                                                            float* __restrict__ y) {
  using T = CvTile<S>;
  constexpr int ND = T::ND, COG = T::COG;
  __shared__ float tile[T::SLAB * T::VOL];
  const CvTilePos p = cv_tile_pos<ND>(blockIdx.x, g);
  const int oc0 = (int)blockIdx.y * COG;
  const int tx = threadIdx.x & (CV_TW - 1), ty = threadIdx.x >> 5;

  float acc[ND][COG];
#pragma unroll
  for (int dz = 0; dz < ND; ++dz)
#pragma unroll
    for (int j = 0; j < COG; ++j) acc[dz][j] = 0.f;

  for (int lc0 = 0; lc0 < g.Cl; lc0 += T::SLAB) {
    const int nslab = min(T::SLAB, g.Cl - lc0);
    __syncthreads();
    cv_stage<S>(tile, x + ((int64_t)p.b * g.Cl + lc0) * g.ivol, nslab, p, g);
    __syncthreads();
    for (int k = 0; k < nslab; ++k) {
      float xv[T::ED][9];
      const float* tp = tile + k * T::VOL + (ty * S) * T::EW;
#pragma unroll
      for (int q = 0; q < T::ED; ++q)
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
          for (int kw = 0; kw < 3; ++kw) xv[q][kh * 3 + kw] = tp[q * T::PLANE + kh * T::EW + T::tapcol(tx, kw)];
      const int lc = lc0 + k;
#pragma unroll
      for (int j = 0; j < COG; ++j) {
        const int oc = min(oc0 + j, g.Co - 1);   // (a channel past the last repeats it and is not stored)
        const float* wp = FLIP ? w + ((int64_t)lc * g.Co + oc) * CV_TAPS : w + ((int64_t)oc * g.Cl + lc) * CV_TAPS;
#pragma unroll
        for (int kd = 0; kd < 3; ++kd)
#pragma unroll
          for (int t9 = 0; t9 < 9; ++t9) {
            const float wv = FLIP ? wp[26 - (kd * 9 + t9)] : wp[kd * 9 + t9];
#pragma unroll
            for (int dz = 0; dz < ND; ++dz) acc[dz][j] = fmaf(wv, xv[dz * S + kd][t9], acc[dz][j]);
          }
      }
    }
  }

  const int oh = p.oh0 + ty, ow = p.ow0 + tx;
  if (oh < g.OH && ow < g.OW) {
#pragma unroll
    for (int j = 0; j < COG; ++j) {
      float* yr = y + ((int64_t)p.b * g.Co + oc0 + j) * g.ovol;
#pragma unroll
      for (int dz = 0; dz < ND; ++dz) {
        const int od = p.od0 + dz;
        if (oc0 + j < g.Co && od < g.OD) yr[(od * g.OH + oh) * g.OW + ow] = acc[dz][j];
      }
    }
  }
}

// ---- backward-data at stride 2: one 2x2x2 block of dx per thread ------------------------------------------------------------------
constexpr int CV_BD_TW = 32, CV_BD_TH = 4, CV_BD_TD = 2;   // blocks per workgroup
constexpr int CV_BD_CIG = 4;                               // input channels (of the convolution) per workgroup
constexpr int CV_BD_SLAB = 8;                              // output channels staged at once
constexpr int CV_BD_GW = CV_BD_TW + 1, CV_BD_GH = CV_BD_TH + 1, CV_BD_GD = CV_BD_TD + 1;
constexpr int CV_BD_PLANE = CV_BD_GH * CV_BD_GW, CV_BD_VOL = CV_BD_GD * CV_BD_PLANE;

// here g.I* are the extents of dx (written), g.O* those of the incoming gradient (staged); Cl = Cout (looped), Co = Cin (produced)
__global__ __launch_bounds__(CV_THREADS) void cv_bwd_data_s2_kernel(CvGeom g, const float* __restrict__ gy, const float* __restrict__ w,
                                                                    float* __restrict__ dx) {
  __shared__ float tile[CV_BD_SLAB * CV_BD_VOL];
  uint32_t t = blockIdx.x;
  const uint32_t tw = t % (uint32_t)g.tW; t /= (uint32_t)g.tW;
  const uint32_t th = t % (uint32_t)g.tH; t /= (uint32_t)g.tH;
  const uint32_t td = t % (uint32_t)g.tD;
  const int b = (int)(t / (uint32_t)g.tD);
  const int md0 = (int)td * CV_BD_TD, mh0 = (int)th * CV_BD_TH, mw0 = (int)tw * CV_BD_TW;
  const int ci0 = (int)blockIdx.y * CV_BD_CIG;
  const int tx = threadIdx.x & 31, ty = (threadIdx.x >> 5) & 3, tz = threadIdx.x >> 7;

  float acc[CV_BD_CIG][8];
#pragma unroll
  for (int j = 0; j < CV_BD_CIG; ++j)
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[j][q] = 0.f;

  for (int co0 = 0; co0 < g.Cl; co0 += CV_BD_SLAB) {
    const int nslab = min(CV_BD_SLAB, g.Cl - co0);
    __syncthreads();
    cv_stage_box<CV_BD_GD, CV_BD_GH, CV_BD_GW, 1>(tile, gy + ((int64_t)b * g.Cl + co0) * g.ovol, nslab, g.ovol, md0, mh0, mw0, g.OD,
                                                  g.OH, g.OW);
    __syncthreads();
    for (int k = 0; k < nslab; ++k) {
      float gv[8];
      const float* tp = tile + k * CV_BD_VOL + tz * CV_BD_PLANE + ty * CV_BD_GW + tx;
#pragma unroll
      for (int q = 0; q < 8; ++q) gv[q] = tp[(q >> 2) * CV_BD_PLANE + ((q >> 1) & 1) * CV_BD_GW + (q & 1)];
      const int co = co0 + k;
#pragma unroll
      for (int j = 0; j < CV_BD_CIG; ++j) {
        const int ci = min(ci0 + j, g.Co - 1);
        const float* wp = w + ((int64_t)co * g.Co + ci) * CV_TAPS;
#pragma unroll
        for (int kd = 0; kd < 3; ++kd)
#pragma unroll
          for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
              // per dimension: tap 1 -> even voxel from g[m]; tap 0 -> odd voxel from g[m+1]; tap 2 -> odd voxel from g[m]
              const int par = (kd != 1) * 4 + (kh != 1) * 2 + (kw != 1);
              const int src = (kd == 0) * 4 + (kh == 0) * 2 + (kw == 0);
              acc[j][par] = fmaf(wp[kd * 9 + kh * 3 + kw], gv[src], acc[j][par]);
            }
      }
    }
  }

#pragma unroll
  for (int j = 0; j < CV_BD_CIG; ++j) {
    float* dr = dx + ((int64_t)b * g.Co + ci0 + j) * g.ivol;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int id = 2 * (md0 + tz) + (q >> 2), ih = 2 * (mh0 + ty) + ((q >> 1) & 1), iw = 2 * (mw0 + tx) + (q & 1);
      if (ci0 + j < g.Co && id < g.ID && ih < g.IH && iw < g.IW) dr[(id * g.IH + ih) * g.IW + iw] = acc[j][q];
    }
  }
}

// ---- backward-weight ------------------------------------------------------------------------------------------------------------
// g.I*: x (staged); g.O*: the incoming gradient (tiled); Cl = Cin, Co = Cout.  grid = (workgroups per channel pair group,
// ceil(Cout / 4), Cin).
template <int S>
__global__ __launch_bounds__(CV_THREADS, 2) void cv_bwd_weight_kernel(CvGeom g, uint32_t nrec, uint32_t tpr, uint32_t ntiles,
                                                                   const float* __restrict__ x, const float* __restrict__ gy,
                                                                   float* __restrict__ records) {
  using T = CvTile<S>;
  constexpr int ND = T::ND, COG = CV_BW_COG;
  __shared__ float tile[T::VOL];
  __shared__ float red[CV_TAPS * CV_RED_STRIDE];
  __shared__ float red8[CV_TAPS * 8];
  const int ci = (int)blockIdx.z, co0 = (int)blockIdx.y * COG;
  const int tid = threadIdx.x, tx = tid & (CV_TW - 1), ty = tid >> 5;

  for (uint32_t rec = blockIdx.x; rec < nrec; rec += gridDim.x) {
    float acc[COG][CV_TAPS];
#pragma unroll
    for (int j = 0; j < COG; ++j)
#pragma unroll
      for (int k = 0; k < CV_TAPS; ++k) acc[j][k] = 0.f;
    const uint32_t t0 = rec * tpr, t1 = min(t0 + tpr, ntiles);
    for (uint32_t t = t0; t < t1; ++t) {
      const CvTilePos p = cv_tile_pos<ND>(t, g);
      __syncthreads();
      cv_stage<S, 4>(tile, x + ((int64_t)p.b * g.Cl + ci) * g.ivol, 1, p, g);
      float gv[ND][COG];
      const int oh = p.oh0 + ty, ow = p.ow0 + tx;
#pragma unroll
      for (int dz = 0; dz < ND; ++dz)
#pragma unroll
        for (int j = 0; j < COG; ++j) {
          const int od = p.od0 + dz;
          const bool live = od < g.OD && oh < g.OH && ow < g.OW && co0 + j < g.Co;
          gv[dz][j] = live ? gy[((int64_t)p.b * g.Co + co0 + j) * g.ovol + (od * g.OH + oh) * g.OW + ow] : 0.f;
        }
      __syncthreads();
      const float* tp = tile + (ty * S) * T::EW;
#pragma unroll
      for (int q = 0; q < T::ED; ++q)
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
          for (int kw = 0; kw < 3; ++kw) {
            const float xv = tp[q * T::PLANE + kh * T::EW + T::tapcol(tx, kw)];
#pragma unroll
            for (int dz = 0; dz < ND; ++dz) {
              const int kd = q - dz * S;
              if (kd < 0 || kd > 2) continue;
#pragma unroll
              for (int j = 0; j < COG; ++j) acc[j][kd * 9 + kh * 3 + kw] = fmaf(gv[dz][j], xv, acc[j][kd * 9 + kh * 3 + kw]);
            }
          }
    }
    // the workgroup's 256 partial sums of each accumulator, one output channel at a time: through LDS ([tap][thread], rows padded so
    // that the eight threads of a tap and the four taps of a 32-lane group read different banks), thread (tap, s) adds elements
    // s, s + 8, .. in ascending order, then thread tap adds the eight in a fixed tree
#pragma unroll
    for (int j = 0; j < COG; ++j) {
      __syncthreads();
#pragma unroll
      for (int k = 0; k < CV_TAPS; ++k) red[k * CV_RED_STRIDE + tid] = acc[j][k];
      __syncthreads();
      if (tid < CV_TAPS * 8) {
        const float* rp = red + (tid >> 3) * CV_RED_STRIDE + (tid & 7);
        float v = 0.f;
#pragma unroll
        for (int i = 0; i < CV_THREADS / 8; ++i) v += rp[8 * i];
        red8[tid] = v;
      }
      __syncthreads();
      if (tid < CV_TAPS && co0 + j < g.Co) {
        const float* r8 = red8 + tid * 8;
        records[(((int64_t)rec * g.Co + co0 + j) * g.Cl + ci) * CV_TAPS + tid] =
            ((r8[0] + r8[1]) + (r8[2] + r8[3])) + ((r8[4] + r8[5]) + (r8[6] + r8[7]));
      }
    }
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
struct CvShape {
  int64_t B;
  int Cin, Cout, S;
  int64_t I[3], O[3];
  int64_t ivol, ovol;
  int64_t tiles[3], ntiles;     // the forward's output tiles (per batch entry: tiles[0] tiles[1] tiles[2]); ntiles includes B
  int64_t nrec, tpr;            // the weight gradient's records
};

// sizes inside the limits -> *sh; else false and the reason in *why
static bool cv_shape(int64_t B, int Cin, int Cout, int64_t D, int64_t H, int64_t W, int stride, CvShape* sh, const char** why) {
  if (Cin < 1 || Cin > CV_MAX_C || Cout < 1 || Cout > CV_MAX_C) { *why = "channel counts must be 1 to 64"; return false; }
  if (stride != 1 && stride != 2) { *why = "stride must be 1 or 2"; return false; }
  if (B < 1 || D < 1 || H < 1 || W < 1) { *why = "B and every extent must be at least 1"; return false; }
  if (row_too_long(D, H, W)) { *why = "a (batch, channel) row must hold fewer than 2^31 elements"; return false; }
  const int64_t lim = 0x7fffffff;
  sh->B = B; sh->Cin = Cin; sh->Cout = Cout; sh->S = stride;
  sh->I[0] = D; sh->I[1] = H; sh->I[2] = W;
  for (int k = 0; k < 3; ++k) sh->O[k] = (sh->I[k] - 1) / stride + 1;
  sh->ivol = D * H * W;
  sh->ovol = sh->O[0] * sh->O[1] * sh->O[2];
  const int nd = stride == 1 ? CvTile<1>::ND : CvTile<2>::ND;
  sh->tiles[0] = (sh->O[0] + nd - 1) / nd;
  sh->tiles[1] = (sh->O[1] + CV_TH - 1) / CV_TH;
  sh->tiles[2] = (sh->O[2] + CV_TW - 1) / CV_TW;
  const int64_t per = sh->tiles[0] * sh->tiles[1] * sh->tiles[2];
  // a launch's grid is B x the tiles of its pass: `finest` bounds the tile count of every pass's tiling from above
  const int64_t finest = ((D + 1) / 2 + 1) * ((H + 3) / 4 + 1) * ((W + 31) / 32 + 1);
  if (B > lim / (per > finest ? per : finest)) { *why = "B times the number of tiles exceeds 2^31 - 1"; return false; }
  sh->ntiles = B * per;
  const Runs runs = cut_runs(sh->ntiles, MAX_REC);
  sh->nrec = runs.n; sh->tpr = runs.per;
  return true;
}

static int cv_check(const char* fn, int64_t B, int Cin, int Cout, int64_t D, int64_t H, int64_t W, int stride, CvShape* sh) {
  const char* why = "";
  if (!cv_shape(B, Cin, Cout, D, H, W, stride, sh, &why)) {
    set_error("%s: B = %lld, Cin = %d, Cout = %d, D H W = %lld x %lld x %lld, stride = %d: %s", fn, (long long)B, Cin, Cout, (long long)D,
              (long long)H, (long long)W, stride, why);
    return MGS_ERR_INVALID_ARG;
  }
  return MGS_OK;
}

static int cv_pointers(const char* fn, const void* a, const void* b, const void* c, const char* names) {
  if (!a || !b || !c) { set_error("%s: NULL %s", fn, names); return MGS_ERR_INVALID_ARG; }
  if (misaligned16(a) || misaligned16(b) || misaligned16(c)) { set_error("%s: %s must be 16-byte aligned", fn, names); return MGS_ERR_INVALID_ARG; }
  return MGS_OK;
}

static CvGeom cv_geom(const CvShape& sh, int Cl, int Co) {
  CvGeom g;
  g.B = (int)sh.B; g.Cl = Cl; g.Co = Co;
  g.ID = (int)sh.I[0]; g.IH = (int)sh.I[1]; g.IW = (int)sh.I[2];
  g.OD = (int)sh.O[0]; g.OH = (int)sh.O[1]; g.OW = (int)sh.O[2];
  g.tD = (int)sh.tiles[0]; g.tH = (int)sh.tiles[1]; g.tW = (int)sh.tiles[2];
  g.ivol = sh.ivol; g.ovol = sh.ovol;
  return g;
}

}  // namespace mgs

using namespace mgs;

extern "C" {

size_t mgs_conv3d_workspace_bytes(int64_t B, int Cin, int Cout, int64_t D, int64_t H, int64_t W, int stride) {
  CvShape sh;
  const char* why;
  if (!cv_shape(B, Cin, Cout, D, H, W, stride, &sh, &why)) return 0;
  return align_up((size_t)sh.nrec * (size_t)Cout * (size_t)Cin * CV_TAPS * sizeof(float)) + ALIGN;
}

int mgs_conv3d_forward(int64_t B, int Cin, int Cout, int64_t D, int64_t H, int64_t W, int stride, const float* x, const float* w,
                       float* y, mgs_stream_t stream) {
  const char* fn = "conv3d_forward";
  CvShape sh;
  if (int rc = cv_check(fn, B, Cin, Cout, D, H, W, stride, &sh)) return rc;
  if (int rc = cv_pointers(fn, x, w, y, "x, w or y")) return rc;
  hipStream_t s = (hipStream_t)stream;
  const CvGeom g = cv_geom(sh, Cin, Cout);
  if (stride == 1) {
    const dim3 grid((unsigned)sh.ntiles, (unsigned)((Cout + CvTile<1>::COG - 1) / CvTile<1>::COG));
    hipLaunchKernelGGL((cv_fwd_kernel<1, false>), grid, dim3(CV_THREADS), 0, s, g, x, w, y);
  } else {
    const dim3 grid((unsigned)sh.ntiles, (unsigned)((Cout + CvTile<2>::COG - 1) / CvTile<2>::COG));
    hipLaunchKernelGGL((cv_fwd_kernel<2, false>), grid, dim3(CV_THREADS), 0, s, g, x, w, y);
  }
  return launch_done(fn);
}

int mgs_conv3d_backward_data(int64_t B, int Cin, int Cout, int64_t D, int64_t H, int64_t W, int stride, const float* g_y,
                             const float* w, float* dx, mgs_stream_t stream) {
  const char* fn = "conv3d_backward_data";
  CvShape sh;
  if (int rc = cv_check(fn, B, Cin, Cout, D, H, W, stride, &sh)) return rc;
  if (int rc = cv_pointers(fn, g_y, w, dx, "g_y, w or dx")) return rc;
  hipStream_t s = (hipStream_t)stream;
  CvGeom g = cv_geom(sh, Cout, Cin);
  if (stride == 1) {   // the forward with the channel roles exchanged and the taps reversed (input and output extents are equal)
    const dim3 grid((unsigned)sh.ntiles, (unsigned)((Cin + CvTile<1>::COG - 1) / CvTile<1>::COG));
    hipLaunchKernelGGL((cv_fwd_kernel<1, true>), grid, dim3(CV_THREADS), 0, s, g, g_y, w, dx);
  } else {
    g.tD = (int)((sh.O[0] + CV_BD_TD - 1) / CV_BD_TD);
    g.tH = (int)((sh.O[1] + CV_BD_TH - 1) / CV_BD_TH);
    g.tW = (int)((sh.O[2] + CV_BD_TW - 1) / CV_BD_TW);
    const dim3 grid((unsigned)(sh.B * g.tD * g.tH * g.tW), (unsigned)((Cin + CV_BD_CIG - 1) / CV_BD_CIG));
    hipLaunchKernelGGL(cv_bwd_data_s2_kernel, grid, dim3(CV_THREADS), 0, s, g, g_y, w, dx);
  }
  return launch_done(fn);
}

int mgs_conv3d_backward_weight(int64_t B, int Cin, int Cout, int64_t D, int64_t H, int64_t W, int stride, const float* x,
                               const float* g_y, float* dw, void* workspace, size_t workspace_bytes, int split, mgs_stream_t stream) {
  const char* fn = "conv3d_backward_weight";
  CvShape sh;
  if (int rc = cv_check(fn, B, Cin, Cout, D, H, W, stride, &sh)) return rc;
  if (int rc = split_check(fn, split)) return rc;
  if (int rc = cv_pointers(fn, x, g_y, dw, "x, g_y or dw")) return rc;
  if (int rc = records_workspace(fn, workspace, workspace_bytes, mgs_conv3d_workspace_bytes(B, Cin, Cout, D, H, W, stride))) return rc;
  hipStream_t s = (hipStream_t)stream;
  const CvGeom g = cv_geom(sh, Cin, Cout);
  const int64_t groups = (int64_t)((Cout + CV_BW_COG - 1) / CV_BW_COG) * Cin;
  const int64_t wgs = split_clamp(split, (CV_TARGET_BLOCKS + groups - 1) / groups, sh.nrec);
  float* records = reinterpret_cast<float*>(workspace);
  const dim3 grid((unsigned)wgs, (unsigned)((Cout + CV_BW_COG - 1) / CV_BW_COG), (unsigned)Cin);
  if (stride == 1)
    hipLaunchKernelGGL((cv_bwd_weight_kernel<1>), grid, dim3(CV_THREADS), 0, s, g, (uint32_t)sh.nrec, (uint32_t)sh.tpr,
                       (uint32_t)sh.ntiles, x, g_y, records);
  else
    hipLaunchKernelGGL((cv_bwd_weight_kernel<2>), grid, dim3(CV_THREADS), 0, s, g, (uint32_t)sh.nrec, (uint32_t)sh.tpr,
                       (uint32_t)sh.ntiles, x, g_y, records);
  launch_records_merge(sh.nrec, Cout, Cin * CV_TAPS, Cin * CV_TAPS, records, dw, nullptr, s);
  return launch_done(fn);
}

}  // extern "C"
