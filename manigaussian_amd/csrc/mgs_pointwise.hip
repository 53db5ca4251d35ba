// mgs_pointwise.hip -- the voxel encoder stem's 1x1x1 convolution with bias (helpers/network_utils.py:248-306: conv_out =
// nn.Conv3d(8, 64, 1, bias=True)), fp32, NCDHW, 1..64 channels on either side, VALU only.  n = D H W voxels per (batch, channel) row.
//
//   forward    y[b,co,v]  = bias[co] + sum_ci w[co,ci] x[b,ci,v]
//   backward   dx[b,ci,v] = sum_co w[co,ci] g[b,co,v]      dw[co,ci] = sum_{b,v} g[b,co,v] x[b,ci,v]      db[co] = sum_{b,v} g[b,co,v]
//
// Every output element is written once by one thread from a sum whose terms and order depend on the shape alone.  No atomics, no
// workgroup waits for another, nothing to zero, no scratch.
//
// Forward.  A workgroup of 256 threads takes PW_TILE = 1024 consecutive voxels of one batch entry, four per thread, and EVERY
// output channel.  Lanes run along v: where n is a multiple of 4 every row starts on a 16-byte boundary and a thread's four voxels
// are one 16-byte access (VEC); for any other n the rows start anywhere, and the thread takes voxels tid, tid + 256, .. of the tile
// as single words (still consecutive across the lanes).  Up to 16 input channels (pw_fwd_narrow_kernel) a thread keeps its x values
// in registers -- x is read once -- and walks the output channels: bias, then the input channels in ascending order, against
// weights whose address is uniform across the wave (scalar loads, SGPR operands).  Above 16 (pw_fwd_wide_kernel) it keeps 8 output
// channels x 4 voxels of accumulators and reads x once per group of 8 output channels.  TRANS reads the weight as its transpose:
// the input gradient alone (dx wanted, dw and db not) is the forward of the transposed weight without a bias, its sum taken in the
// fused backward's order (a chain per 8 output channels, the chains added in ascending order): dx is the same bits either way.
// No load sits behind a branch: a voxel or channel that is not there loads an element that is and drops it, so that all of a
// thread's loads are in flight before the first is used.
//
// Backward, whenever dw or db is wanted (pw_bwd_kernel; merge: mgs_records.hip).  Tiles of TV = 64 VPL voxels (VPL = 4 voxels per lane up
// to 8 input channels, 2 up to 16), in their linear order over (batch, voxel), are cut into nrec <= 64 runs of tpr tiles; nrec and
// tpr depend on the shape alone.  A workgroup of 8 waves takes a run.  Wave k owns output channels 8k .. 8k + 7 for the whole run:
// per tile it reads ITS rows of g -- so every element of g is read from memory once, by one wave -- and the tile's x, and keeps
// 8 x (Cin + 1) accumulators per lane (g x per input channel, and g itself for db); no other wave touches those sums.  For dx the
// wave multiplies its 8 rows of g by its 8 x Cin weights (loaded once, one per lane, and read back lane by lane into SGPR operands)
// into a partial dx of the tile, the partials of the waves meet in LDS, and thread (input channel, lane) adds them in ascending wave
// order and writes dx.  The next tile's g is requested before the current one is used and is not waited for until it becomes the
// current one, the two barriers of a tile included.  At the end of a run a wave adds each accumulator over its 64 lanes in a fixed xor tree
// (32, 16, .. 1) and lane 0 writes the run's RECORD [Cout, Cin + 1] into the workspace.  `split` is the number of workgroups that
// share the runs: it decides who computes a record, not what the record is.  The merge launch sums the records in ascending order
// in double: dw and db are the same bits for every split.  Above 16 input channels the launch is repeated per group of 16 input
// channels, re-reading g (the accumulators of more do not fit a lane).
//
// The wide op (mgs_pointwise_wide_*: Cin 1..16, Cout 65..256; conv_out at final_dim = 128 is 8 -> 128).  Forward and the input
// gradient alone are the kernels above as they are: pw_fwd_narrow_kernel walks any number of output channels, pw_fwd_wide_kernel<TRANS>
// any number of looped ones.  The fused backward is pw_bwd_kernel<.., BLOCKS>: 8 waves of 8 output channels are a BLOCK of 64, and a
// workgroup walks its run of tiles once per block, in ascending order, with the same registers as the narrow op's single pass.  g is
// read once, x once per block; dx is written once per block, and from the second block on a thread first reads back what IT stored
// for the element in the block before and adds the waves' shares to that -- one chain over the groups of 8 output channels in
// ascending order, the TRANS forward's association, so dx is the same bits whether or not dw and db are asked for.  (DERIVED: 168
// rows of n floats at 8 -> 128 against 144 if both blocks' accumulators were live at once, which 256 VGPRs do not hold beside the
// double-buffered g.)  Up to 8 input channels the read-back is the first load of a tile, in flight while the tile is worked on;
// above 8 the registers for that are not there and it is issued behind the tile's barrier.
//
// Element offsets are 64-bit; n < 2^31.
#include "mgs_common.h"

namespace mgs {

constexpr int PW_MAX_C = 64;
constexpr int PW_THREADS = 256;             // forward
constexpr int PW_TILE = 4 * PW_THREADS;     // voxels per workgroup of the forward
constexpr int PW_NARROW = 16;               // most input channels a thread of the forward keeps in registers
constexpr int PW_FWD_COG = 8;               // output channels per accumulator group of the wide forward
constexpr int PW_BWD_WAVES = 8;             // waves per workgroup of the backward
constexpr int PW_BWD_THREADS = 64 * PW_BWD_WAVES;
constexpr int PW_BWD_COG = 8;               // output channels per wave of the backward
constexpr int PW_BWD_CIG = 16;              // most input channels per launch of the backward
constexpr int PW_BWD_BLOCK = PW_BWD_WAVES * PW_BWD_COG;   // output channels per pass of a workgroup over its run
constexpr int PW_WIDE_MAX_CIN = PW_BWD_CIG; // the wide op (mgs_pointwise_wide_*): what the fused backward holds per lane ...
constexpr int PW_WIDE_MIN_COUT = PW_MAX_C + 1, PW_WIDE_MAX_COUT = 256;   // ... and the output channels the narrow op does not take

// NV values of the row `row` (n long) for the tile that starts at voxel v0: VEC: voxels v0 + pos NV .. + NV - 1 in one access (n and
// v0 are multiples of NV, the row starts on a 16-byte boundary); else voxels v0 + pos + k LANES, one word each.  Voxels past n are 0,
// and so is everything when `live` is false (`row` must be a row that exists all the same).  No branch around a load -- a voxel that
// is not there loads the row's first element and drops it -- so that a thread's loads are all in flight before the first is used.
// the two halves of pw_load: the loads alone (what comes back for a voxel that is not there is undefined) ...
template <int NV, int LANES, bool VEC>
__device__ __forceinline__ void pw_fetch(float (&v)[NV], const float* __restrict__ row, int64_t v0, int pos, int64_t n) {
  if (VEC) {
    const int64_t i = v0 + (int64_t)pos * NV;
    if (NV == 4) {
      const float4 q = *reinterpret_cast<const float4*>(row + (i < n ? i : (int64_t)0));
      v[0] = q.x; v[1] = q.y; v[NV - 2] = q.z; v[NV - 1] = q.w;
    } else {
      const float2 q = *reinterpret_cast<const float2*>(row + (i < n ? i : (int64_t)0));
      v[0] = q.x; v[1] = q.y;
    }
  } else {
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int64_t i = v0 + pos + (int64_t)k * LANES;
      v[k] = row[i < n ? i : (int64_t)0];
    }
  }
}
// ... and the zeros, which may be put in long after: nothing waits for a load until its value is used
template <int NV, int LANES, bool VEC>
__device__ __forceinline__ void pw_mask(float (&v)[NV], int64_t v0, int pos, int64_t n, bool live) {
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int64_t i = VEC ? v0 + (int64_t)pos * NV : v0 + pos + (int64_t)k * LANES;
    if (!(live && i < n)) v[k] = 0.f;
  }
}
template <int NV, int LANES, bool VEC>
__device__ __forceinline__ void pw_load(float (&v)[NV], const float* __restrict__ row, int64_t v0, int pos, int64_t n, bool live = true) {
  pw_fetch<NV, LANES, VEC>(v, row, v0, pos, n);
  pw_mask<NV, LANES, VEC>(v, v0, pos, n, live);
}

template <int NV, int LANES, bool VEC>
__device__ __forceinline__ void pw_store(const float (&v)[NV], float* __restrict__ row, int64_t v0, int pos, int64_t n) {
  if (VEC) {
    const int64_t i = v0 + (int64_t)pos * NV;
    if (i < n) {
      if (NV == 4) *reinterpret_cast<float4*>(row + i) = make_float4(v[0], v[1], v[NV - 2], v[NV - 1]);
      else *reinterpret_cast<float2*>(row + i) = make_float2(v[0], v[1]);
    }
  } else {
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int64_t i = v0 + pos + (int64_t)k * LANES;
      if (i < n) row[i] = v[k];
    }
  }
}

// the weight of (looped channel lc, produced channel oc): w is [Co, Cl], or [Cl, Co] read as its transpose
template <bool TRANS>
__device__ __forceinline__ float pw_weight(const float* __restrict__ w, int lc, int oc, int Cl, int Co) {
  return TRANS ? w[lc * Co + oc] : w[oc * Cl + lc];
}

// ---- forward: up to CI looped channels, kept in registers ---------------------------------------------------------------------
template <int CI, bool VEC, bool TRANS>
__global__ __launch_bounds__(PW_THREADS) void pw_fwd_narrow_kernel(int Cl, int Co, int64_t n, uint32_t tiles_per_row,
                                                                   const float* __restrict__ x, const float* __restrict__ w,
                                                                   const float* __restrict__ bias, float* __restrict__ y) {
  const uint32_t b = blockIdx.x / tiles_per_row, t = blockIdx.x - b * tiles_per_row;
  const int64_t v0 = (int64_t)t * PW_TILE;
  const int tid = threadIdx.x;
  const float* xb = x + (int64_t)b * Cl * n;
  float* yb = y + (int64_t)b * Co * n;
  float xv[CI][4];
#pragma unroll
  for (int ci = 0; ci < CI; ++ci) {
    // (a channel past the last: zeros against a zero weight)
    pw_load<4, PW_THREADS, VEC>(xv[ci], xb + (int64_t)min(ci, Cl - 1) * n, v0, tid, n, ci < Cl);
  }
#pragma unroll 2
  for (int oc = 0; oc < Co; ++oc) {
    const float b0 = (!TRANS && bias) ? bias[oc] : 0.f;
    float a[4] = {b0, b0, b0, b0};
#pragma unroll
    for (int c0 = 0; c0 < CI; c0 += PW_BWD_COG) {
      if (TRANS && c0 > 0 && c0 >= Cl) break;
      // forward: one chain from the bias.  TRANS: a chain from zero per group of 8 looped channels, the groups added in ascending
      // order -- the order in which pw_bwd_kernel's waves form dx, so that dx is the same bits whether dw and db are asked for or not
      float p[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ci = c0; ci < c0 + PW_BWD_COG; ++ci) {
        const float wv = ci < Cl ? pw_weight<TRANS>(w, ci, oc, Cl, Co) : 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (TRANS && c0 > 0) p[k] = fmaf(wv, xv[ci][k], p[k]);
          else a[k] = fmaf(wv, xv[ci][k], a[k]);
        }
      }
      if (TRANS && c0 > 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) a[k] += p[k];
      }
    }
    pw_store<4, PW_THREADS, VEC>(a, yb + (int64_t)oc * n, v0, tid, n);
  }
}

// ---- forward: any number of looped channels; x is read once per group of PW_FWD_COG produced channels ---------------------------
template <bool VEC, bool TRANS>
__global__ __launch_bounds__(PW_THREADS) void pw_fwd_wide_kernel(int Cl, int Co, int64_t n, uint32_t tiles_per_row,
                                                                 const float* __restrict__ x, const float* __restrict__ w,
                                                                 const float* __restrict__ bias, float* __restrict__ y) {
  constexpr int COG = PW_FWD_COG;
  const uint32_t b = blockIdx.x / tiles_per_row, t = blockIdx.x - b * tiles_per_row;
  const int64_t v0 = (int64_t)t * PW_TILE;
  const int tid = threadIdx.x;
  const float* xb = x + (int64_t)b * Cl * n;
  float* yb = y + (int64_t)b * Co * n;
  for (int oc0 = 0; oc0 < Co; oc0 += COG) {
    float a[COG][4];
#pragma unroll
    for (int j = 0; j < COG; ++j) {
      const float b0 = (!TRANS && bias) ? bias[min(oc0 + j, Co - 1)] : 0.f;   // (a channel past the last repeats it and is not stored)
#pragma unroll
      for (int k = 0; k < 4; ++k) a[j][k] = b0;
    }
    if (!TRANS) {   // one chain from the bias
#pragma unroll 2
      for (int lc = 0; lc < Cl; ++lc) {
        float xv[4];
        pw_load<4, PW_THREADS, VEC>(xv, xb + (int64_t)lc * n, v0, tid, n);
#pragma unroll
        for (int j = 0; j < COG; ++j) {
          const float wv = pw_weight<TRANS>(w, lc, min(oc0 + j, Co - 1), Cl, Co);
#pragma unroll
          for (int k = 0; k < 4; ++k) a[j][k] = fmaf(wv, xv[k], a[j][k]);
        }
      }
    } else {        // a chain from zero per group of 8 looped channels, the groups added in ascending order (see the narrow kernel)
      for (int lc0 = 0; lc0 < Cl; lc0 += PW_BWD_COG) {
        float p[COG][4];
#pragma unroll
        for (int j = 0; j < COG; ++j)
#pragma unroll
          for (int k = 0; k < 4; ++k) p[j][k] = 0.f;
#pragma unroll
        for (int i = 0; i < PW_BWD_COG; ++i) {
          const int lc = lc0 + i;
          float xv[4];
          pw_load<4, PW_THREADS, VEC>(xv, xb + (int64_t)min(lc, Cl - 1) * n, v0, tid, n, lc < Cl);
#pragma unroll
          for (int j = 0; j < COG; ++j) {
            const float wv = lc < Cl ? pw_weight<TRANS>(w, lc, min(oc0 + j, Co - 1), Cl, Co) : 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) p[j][k] = fmaf(wv, xv[k], p[j][k]);
          }
        }
#pragma unroll
        for (int j = 0; j < COG; ++j)
#pragma unroll
          for (int k = 0; k < 4; ++k) a[j][k] = lc0 == 0 ? p[j][k] : a[j][k] + p[j][k];
      }
    }
#pragma unroll
    for (int j = 0; j < COG; ++j)
      if (oc0 + j < Co) pw_store<4, PW_THREADS, VEC>(a[j], yb + (int64_t)(oc0 + j) * n, v0, tid, n);
  }
}

// ---- backward with dw | db (and dx, when asked for, from the same read of g) ------------------------------------------------------
struct PwBwd {
  int Cin, Cout;
  int ci0, nci;                        // this launch's input channels: ci0 .. ci0 + nci - 1
  int64_t n;
  uint32_t tiles_per_row, ntiles;      // tiles of TV voxels: per (batch entry), and B times that
  uint32_t nrec, tpr;                  // runs, tiles per run
  const float *x, *g, *w;
  float *dx, *records;                 // dx may be nullptr; records [nrec, Cout, Cin + 1]
};

__device__ __forceinline__ float pw_wave_sum(float v) {   // the 64 lanes' values in a fixed tree; every lane gets the sum
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// A wave's COG x CI weights w[co0 + j][ci0 + ci], one per lane of NW = COG CI / 64 registers (element j CI + ci in lane (j CI + ci) % 64
// of register (j CI + ci) / 64; zero where the wave or the launch has no such channel), loaded once per workgroup and read back lane
// by lane into scalar registers: no load inside the tile loop.
template <int COG, int CI>
struct PwWeights {
  static constexpr int NW = COG * CI / 64;
  float r[NW];
  __device__ __forceinline__ void load(const float* __restrict__ w, int co0, int nco, int ci0, int nci, int Cin, int lane) {
#pragma unroll
    for (int h = 0; h < NW; ++h) {
      const int e = h * 64 + lane, j = e / CI, ci = e - j * CI;
      const bool live = j < nco && ci < nci;
      const float got = w[live ? (co0 + j) * Cin + ci0 + ci : 0];
      r[h] = live ? got : 0.f;
    }
  }
  // j is a constant after unrolling; ci may be any value that is uniform across the wave
  __device__ __forceinline__ float at(int j, int ci) const {
    // (CI divides 64 and ci < CI: the register is a function of j alone, a constant index)
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(r[(j * CI) >> 6]), ((j * CI) & 63) + ci));
  }
};

// one input channel of a wave's share of dx: sum_j w[j][ci] cur[j][.] over the wave's output channels, in ascending order, into the
// wave's LDS row `out` (indexed by the voxel's offset in the tile)
template <int COG, int CI, int VPL, bool VEC>
__device__ __forceinline__ void pw_dx_share(const float (&cur)[COG][VPL], const PwWeights<COG, CI>& wt, int ci, float* out, int lane) {
  float p[VPL];
#pragma unroll
  for (int k = 0; k < VPL; ++k) p[k] = 0.f;
#pragma unroll
  for (int j = 0; j < COG; ++j) {
    const float wv = wt.at(j, ci);
#pragma unroll
    for (int k = 0; k < VPL; ++k) p[k] = fmaf(wv, cur[j][k], p[k]);
  }
  if (VEC) {
    if (VPL == 4) *reinterpret_cast<float4*>(out + lane * VPL) = make_float4(p[0], p[1], p[VPL - 2], p[VPL - 1]);
    else *reinterpret_cast<float2*>(out + lane * VPL) = make_float2(p[0], p[1]);
  } else {
#pragma unroll
    for (int k = 0; k < VPL; ++k) out[k * 64 + lane] = p[k];
  }
}

// BLOCKS (the wide op: more than PW_BWD_BLOCK = 64 output channels, one launch, ci0 = 0): a run is walked once per block of 64 output
// channels, in ascending order.  In block c wave k owns channels 64 c + 8 k .. + 7 and writes those rows of the run's record.  In a
// block after the first a dx element's sum starts from what the SAME thread stored for it in the block before, and the waves'
// shares are added to that in ascending wave order: dx is one chain over the groups of 8 output channels in ascending order, the
// association of the TRANS forward.  Without BLOCKS there is the one block, taken before the runs as ever.
template <int CI, int VPL, bool VEC, bool BLOCKS = false>
__global__ __launch_bounds__(PW_BWD_THREADS) void pw_bwd_kernel(PwBwd a) {
  constexpr int COG = PW_BWD_COG, TV = 64 * VPL;
  constexpr int UNITS = CI * 64 / PW_BWD_THREADS;                 // (input channel, lane) units of dx per thread
  __shared__ __attribute__((aligned(16))) float part[PW_BWD_WAVES * CI * TV];   // [wave][input channel][voxel of the tile]
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const bool want_dx = a.dx != nullptr;
  const int64_t n = a.n;
  const int nblk = BLOCKS ? (a.Cout + PW_BWD_BLOCK - 1) / PW_BWD_BLOCK : 1;
  int co0, nco, nwave;
  PwWeights<COG, CI> wt;
  auto take_block = [&](int cb) {
    co0 = cb * PW_BWD_BLOCK + wave * COG;
    nco = min(max(a.Cout - co0, 0), COG);                         // this wave's output channels (0: it only helps to add up dx)
    nwave = (min(a.Cout - cb * PW_BWD_BLOCK, PW_BWD_BLOCK) + COG - 1) / COG;   // waves that own output channels
    if (want_dx) {
      wt.load(a.w, co0, nco, a.ci0, a.nci, a.Cin, lane);
    } else {   // (w may be NULL then)
#pragma unroll
      for (int h = 0; h < PwWeights<COG, CI>::NW; ++h) wt.r[h] = 0.f;
    }
  };
  if (!BLOCKS) take_block(0);

  // the rows of tile t: g of this wave's output channels, x of the launch's input channels (rows that do not exist: zeros)
  auto fetch_g = [&](float (&gv)[COG][VPL], uint32_t t) {   // (the zeros are put in when the tile becomes the current one)
    const uint32_t b = t / a.tiles_per_row, vt = t - b * a.tiles_per_row;
#pragma unroll
    for (int j = 0; j < COG; ++j)
      pw_fetch<VPL, 64, VEC>(gv[j], a.g + ((int64_t)b * a.Cout + min(co0 + j, a.Cout - 1)) * n, (int64_t)vt * TV, lane, n);
  };
  auto load_x = [&](float (&xv)[CI][VPL], uint32_t t) {
    const uint32_t b = t / a.tiles_per_row, vt = t - b * a.tiles_per_row;
#pragma unroll
    for (int ci = 0; ci < CI; ++ci)
      pw_load<VPL, 64, VEC>(xv[ci], a.x + ((int64_t)b * a.Cin + a.ci0 + min(ci, a.nci - 1)) * n, (int64_t)vt * TV, lane, n, ci < a.nci);
  };

  for (uint32_t rec = blockIdx.x; rec < a.nrec; rec += gridDim.x)
  for (int cb = 0; cb < nblk; ++cb) {   // (one block, taken above, without BLOCKS)
    if (BLOCKS) take_block(cb);
    const bool later = BLOCKS && cb > 0 && want_dx;   // dx holds the sum over the blocks before this one
    float acc[COG][CI + 1];
#pragma unroll
    for (int j = 0; j < COG; ++j)
#pragma unroll
      for (int c = 0; c <= CI; ++c) acc[j][c] = 0.f;
    const uint32_t t0 = rec * a.tpr, t1 = min(t0 + a.tpr, a.ntiles);

    float gn[COG][VPL];
    if (nco > 0) fetch_g(gn, t0);
    for (uint32_t t = t0; t < t1; ++t) {
      const uint32_t b = t / a.tiles_per_row, vt = t - b * a.tiles_per_row;
      const int64_t v0 = (int64_t)vt * TV;
      // what this thread stored into its units of dx in the block before (behind a uniform branch).  A voxel or channel that is not
      // there loads one that is and is not stored.  With VPL = 4 it is the first of the tile's loads, in flight while the tile is
      // worked on; with VPL = 2 the registers for that are not there, and it is asked for behind the barrier, the tile's g and x spent.
      float prev[UNITS][VPL];
      auto fetch_prev = [&]() {
#pragma unroll
        for (int i = 0; i < UNITS; ++i) {
          const int u = threadIdx.x + i * PW_BWD_THREADS;
          pw_fetch<VPL, 64, VEC>(prev[i], a.dx + ((int64_t)b * a.Cin + min(u >> 6, a.nci - 1)) * n, v0, u & 63, n);
        }
      };
      if (later && VPL == 4) fetch_prev();
      if (nco > 0) {   // (uniform across the wave)
        float cur[COG][VPL], xv[CI][VPL];
#pragma unroll
        for (int j = 0; j < COG; ++j) {
#pragma unroll
          for (int k = 0; k < VPL; ++k) cur[j][k] = gn[j][k];
          pw_mask<VPL, 64, VEC>(cur[j], v0, lane, n, j < nco);
        }
        load_x(xv, t);                     // (before the next tile's g: loads return in order, and x is needed first)
        fetch_g(gn, min(t + 1, t1 - 1));    // the next tile's g, in flight while this one is used (the run's last tile: itself again)
        if (want_dx) {
          // this wave's share of dx over its own output channels, in ascending order
          float* pp = part + wave * CI * TV;
          if (CI <= 8) {
#pragma unroll
            for (int ci = 0; ci < CI; ++ci)
              if (ci < a.nci) pw_dx_share<COG, CI, VPL, VEC>(cur, wt, ci, pp + ci * TV, lane);
          } else {
#pragma unroll 1
            for (int ci = 0; ci < a.nci; ++ci) pw_dx_share<COG, CI, VPL, VEC>(cur, wt, ci, pp + ci * TV, lane);
          }
        }
        // dw and db: g x per input channel, g itself
#pragma unroll
        for (int j = 0; j < COG; ++j) {
#pragma unroll
          for (int ci = 0; ci < CI; ++ci)
#pragma unroll
            for (int k = 0; k < VPL; ++k) acc[j][ci] = fmaf(cur[j][k], xv[ci][k], acc[j][ci]);
#pragma unroll
          for (int k = 0; k < VPL; ++k) acc[j][CI] += cur[j][k];
        }
      }
      if (want_dx) {
        __syncthreads();
        if (later && VPL != 4) fetch_prev();
        // the waves' shares, added in ascending wave order (in a later block: to `before`, the blocks before this one): one (input
        // channel, lane) unit of VPL voxels per step
        auto add_up = [&](int u, const float (&before)[VPL]) {
          const int ci = u >> 6, l = u & 63;
          if (ci < a.nci) {
            float s[VPL];
#pragma unroll
            for (int k = 0; k < VPL; ++k) {
              s[k] = part[ci * TV + (VEC ? l * VPL + k : k * 64 + l)];
              if (later) s[k] = before[k] + s[k];
            }
            for (int wv = 1; wv < nwave; ++wv)
#pragma unroll
              for (int k = 0; k < VPL; ++k) s[k] += part[(wv * CI + ci) * TV + (VEC ? l * VPL + k : k * 64 + l)];
            pw_store<VPL, 64, VEC>(s, a.dx + ((int64_t)b * a.Cin + a.ci0 + ci) * n, v0, l, n);
          }
        };
        if (BLOCKS) {
#pragma unroll
          for (int i = 0; i < UNITS; ++i) add_up(threadIdx.x + i * PW_BWD_THREADS, prev[i]);
        } else {
          for (int u = threadIdx.x; u < CI * 64; u += PW_BWD_THREADS) add_up(u, prev[0]);
        }
        __syncthreads();
      }
    }
    // the run's record: every accumulator over the wave's 64 lanes, in a fixed tree
    float* rp = a.records + (int64_t)rec * a.Cout * (a.Cin + 1);
#pragma unroll
    for (int j = 0; j < COG; ++j)
#pragma unroll
      for (int c = 0; c <= CI; ++c) {
        const float s = pw_wave_sum(acc[j][c]);
        const bool mine = c < CI ? c < a.nci : a.ci0 == 0;   // (the bias column is written by the first input-channel group)
        if (lane == 0 && j < nco && mine) rp[(co0 + j) * (a.Cin + 1) + (c < CI ? a.ci0 + c : a.Cin)] = s;
      }
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
struct PwShape {
  int64_t B, n;
  int Cin, Cout;
  bool vec;                     // n is a multiple of 4: every row starts on a 16-byte boundary
  int64_t fwd_tiles_per_row;    // tiles of PW_TILE voxels
  int vpl;                      // the backward's voxels per lane (4 up to 8 input channels, else 2); its tile is 64 vpl voxels
  int64_t tiles_per_row, ntiles, nrec, tpr;   // the backward's tiles, runs and tiles per run
};

// wide: the limits of mgs_pointwise_wide_* (everything else is the same)
static bool pw_shape(int64_t B, int Cin, int Cout, int64_t n, PwShape* sh, const char** why, bool wide = false) {
  if (wide) {
    if (Cin < 1 || Cin > PW_WIDE_MAX_CIN) { *why = "Cin must be 1 to 16"; return false; }
    if (Cout < PW_WIDE_MIN_COUT || Cout > PW_WIDE_MAX_COUT) { *why = "Cout must be 65 to 256"; return false; }
  } else if (Cin < 1 || Cin > PW_MAX_C || Cout < 1 || Cout > PW_MAX_C) { *why = "channel counts must be 1 to 64"; return false; }
  if (B < 1 || n < 1) { *why = "B and n must be at least 1"; return false; }
  if (row_too_long(1, 1, n)) { *why = "a (batch, channel) row must hold fewer than 2^31 elements"; return false; }
  const int64_t lim = 0x7fffffff;
  sh->B = B; sh->n = n; sh->Cin = Cin; sh->Cout = Cout;
  sh->vec = n % 4 == 0;
  sh->fwd_tiles_per_row = (n + PW_TILE - 1) / PW_TILE;
  sh->vpl = Cin <= 8 ? 4 : 2;
  const int64_t tv = 64 * sh->vpl;
  sh->tiles_per_row = (n + tv - 1) / tv;
  const int64_t finest = (n + 127) / 128;   // bounds the tile count of every launch from above
  if (B > lim / finest) { *why = "B times the number of tiles exceeds 2^31 - 1"; return false; }
  sh->ntiles = B * sh->tiles_per_row;
  const Runs runs = cut_runs(sh->ntiles, MAX_REC);
  sh->nrec = runs.n; sh->tpr = runs.per;
  return true;
}

static int pw_check(const char* fn, int64_t B, int Cin, int Cout, int64_t n, PwShape* sh, bool wide = false) {
  const char* why = "";
  if (!pw_shape(B, Cin, Cout, n, sh, &why, wide)) {
    set_error("%s: B = %lld, Cin = %d, Cout = %d, n = %lld: %s", fn, (long long)B, Cin, Cout, (long long)n, why);
    return MGS_ERR_INVALID_ARG;
  }
  return MGS_OK;
}

// the forward kernels: Cl looped channels -> Co produced ones; trans: w is [Cl, Co]
static void pw_launch_forward(const PwShape& sh, int Cl, int Co, bool trans, const float* x, const float* w, const float* bias,
                              float* y, hipStream_t s) {
  const dim3 grid((unsigned)(sh.B * sh.fwd_tiles_per_row)), block(PW_THREADS);
  const uint32_t tpr = (uint32_t)sh.fwd_tiles_per_row;
#define PW_FWD(KERNEL) hipLaunchKernelGGL(KERNEL, grid, block, 0, s, Cl, Co, sh.n, tpr, x, w, bias, y)
#define PW_FWD_NARROW(CI)                                            \
  do {                                                               \
    if (sh.vec) {                                                    \
      if (trans) PW_FWD((pw_fwd_narrow_kernel<CI, true, true>));     \
      else PW_FWD((pw_fwd_narrow_kernel<CI, true, false>));          \
    } else {                                                         \
      if (trans) PW_FWD((pw_fwd_narrow_kernel<CI, false, true>));    \
      else PW_FWD((pw_fwd_narrow_kernel<CI, false, false>));         \
    }                                                                \
  } while (0)
  if (Cl <= 8) {
    PW_FWD_NARROW(8);
  } else if (Cl <= PW_NARROW) {
    PW_FWD_NARROW(16);
  } else if (sh.vec) {
    if (trans) PW_FWD((pw_fwd_wide_kernel<true, true>));
    else PW_FWD((pw_fwd_wide_kernel<true, false>));
  } else {
    if (trans) PW_FWD((pw_fwd_wide_kernel<false, true>));
    else PW_FWD((pw_fwd_wide_kernel<false, false>));
  }
#undef PW_FWD_NARROW
#undef PW_FWD
}

// ---- the entry points' bodies: mgs_pointwise_* and, wide, mgs_pointwise_wide_* (its limits, and the backward walks blocks of 64
// output channels) -----------------------------------------------------------------------------------------------------------------
static size_t pw_workspace_bytes(int64_t B, int Cin, int Cout, int64_t n, bool wide) {
  PwShape sh;
  const char* why;
  if (!pw_shape(B, Cin, Cout, n, &sh, &why, wide)) return 0;
  return align_up((size_t)sh.nrec * (size_t)Cout * (size_t)(Cin + 1) * sizeof(float)) + ALIGN;
}

static int pw_forward(const char* fn, bool wide, int64_t B, int Cin, int Cout, int64_t n, const float* x, const float* w,
                      const float* bias, float* y, mgs_stream_t stream) {
  PwShape sh;
  if (int rc = pw_check(fn, B, Cin, Cout, n, &sh, wide)) return rc;
  if (!x || !w || !y) { set_error("%s: NULL x, w or y", fn); return MGS_ERR_INVALID_ARG; }
  if (misaligned16(x) || misaligned16(w) || misaligned16(y) || misaligned16(bias)) {
    set_error("%s: x, w, bias and y must be 16-byte aligned", fn);
    return MGS_ERR_INVALID_ARG;
  }
  pw_launch_forward(sh, Cin, Cout, false, x, w, bias, y, (hipStream_t)stream);
  return launch_done(fn);
}

static int pw_backward(const char* fn, bool wide, int64_t B, int Cin, int Cout, int64_t n, const float* x, const float* g_y,
                       const float* w, float* dx, float* dw, float* db, void* workspace, size_t workspace_bytes, int split,
                       mgs_stream_t stream) {
  PwShape sh;
  if (int rc = pw_check(fn, B, Cin, Cout, n, &sh, wide)) return rc;
  if (int rc = split_check(fn, split)) return rc;
  if (!dx && !dw && !db) { set_error("%s: NULL dx, dw and db: no gradient is asked for", fn); return MGS_ERR_INVALID_ARG; }
  const bool sums = dw || db;
  if (!g_y || (dx && !w) || (sums && !x)) { set_error("%s: NULL g_y, w (needed for dx) or x (needed for dw and db)", fn); return MGS_ERR_INVALID_ARG; }
  if (misaligned16(x) || misaligned16(g_y) || misaligned16(w) || misaligned16(dx) || misaligned16(dw) || misaligned16(db)) {
    set_error("%s: x, g_y, w, dx, dw and db must be 16-byte aligned", fn);
    return MGS_ERR_INVALID_ARG;
  }
  hipStream_t s = (hipStream_t)stream;
  if (!sums) {   // dx alone: the forward of the transposed weight, no bias, no workspace, one launch
    pw_launch_forward(sh, Cout, Cin, true, g_y, w, nullptr, dx, s);
    return launch_done(fn);
  }
  if (int rc = records_workspace(fn, workspace, workspace_bytes, pw_workspace_bytes(B, Cin, Cout, n, wide))) return rc;
  const int64_t wgs = split_clamp(split, MAX_REC, sh.nrec);
  PwBwd a;
  a.Cin = Cin; a.Cout = Cout; a.n = n;
  a.tiles_per_row = (uint32_t)sh.tiles_per_row; a.ntiles = (uint32_t)sh.ntiles;
  a.nrec = (uint32_t)sh.nrec; a.tpr = (uint32_t)sh.tpr;
  a.x = x; a.g = g_y; a.w = w; a.dx = dx;
  a.records = reinterpret_cast<float*>(workspace);
  const dim3 grid((unsigned)wgs), block(PW_BWD_THREADS);
  if (wide) {   // up to 16 input channels: one launch, g read once; the blocks of 64 output channels inside it
    a.ci0 = 0;
    a.nci = Cin;
    if (sh.vpl == 4) {
      if (sh.vec) hipLaunchKernelGGL((pw_bwd_kernel<8, 4, true, true>), grid, block, 0, s, a);
      else hipLaunchKernelGGL((pw_bwd_kernel<8, 4, false, true>), grid, block, 0, s, a);
    } else {
      if (sh.vec) hipLaunchKernelGGL((pw_bwd_kernel<16, 2, true, true>), grid, block, 0, s, a);
      else hipLaunchKernelGGL((pw_bwd_kernel<16, 2, false, true>), grid, block, 0, s, a);
    }
  }
  // more than 16 input channels: one launch per group of 16, each reading g again
  for (int ci0 = 0; !wide && ci0 < Cin; ci0 += PW_BWD_CIG) {
    a.ci0 = ci0;
    a.nci = Cin - ci0 < PW_BWD_CIG ? Cin - ci0 : PW_BWD_CIG;
    if (sh.vpl == 4) {
      if (sh.vec) hipLaunchKernelGGL((pw_bwd_kernel<8, 4, true>), grid, block, 0, s, a);
      else hipLaunchKernelGGL((pw_bwd_kernel<8, 4, false>), grid, block, 0, s, a);
    } else {
      if (sh.vec) hipLaunchKernelGGL((pw_bwd_kernel<16, 2, true>), grid, block, 0, s, a);
      else hipLaunchKernelGGL((pw_bwd_kernel<16, 2, false>), grid, block, 0, s, a);
    }
  }
  launch_records_merge(sh.nrec, Cout, Cin + 1, Cin, a.records, dw, db, s);
  return launch_done(fn);
}

}  // namespace mgs

using namespace mgs;

extern "C" {

size_t mgs_pointwise_workspace_bytes(int64_t B, int Cin, int Cout, int64_t n) { return pw_workspace_bytes(B, Cin, Cout, n, false); }

int mgs_pointwise_forward(int64_t B, int Cin, int Cout, int64_t n, const float* x, const float* w, const float* bias, float* y,
                          mgs_stream_t stream) {
  return pw_forward("pointwise_forward", false, B, Cin, Cout, n, x, w, bias, y, stream);
}

int mgs_pointwise_backward(int64_t B, int Cin, int Cout, int64_t n, const float* x, const float* g_y, const float* w, float* dx,
                           float* dw, float* db, void* workspace, size_t workspace_bytes, int split, mgs_stream_t stream) {
  return pw_backward("pointwise_backward", false, B, Cin, Cout, n, x, g_y, w, dx, dw, db, workspace, workspace_bytes, split, stream);
}

// Cin 1..16, Cout 65..256: the same forward kernels (x in registers, any number of output channels; the input gradient alone is the
// TRANS forward), and the fused backward over blocks of 64 output channels
size_t mgs_pointwise_wide_workspace_bytes(int64_t B, int Cin, int Cout, int64_t n) { return pw_workspace_bytes(B, Cin, Cout, n, true); }

int mgs_pointwise_wide_forward(int64_t B, int Cin, int Cout, int64_t n, const float* x, const float* w, const float* bias, float* y,
                               mgs_stream_t stream) {
  return pw_forward("pointwise_wide_forward", true, B, Cin, Cout, n, x, w, bias, y, stream);
}

int mgs_pointwise_wide_backward(int64_t B, int Cin, int Cout, int64_t n, const float* x, const float* g_y, const float* w, float* dx,
                                float* dw, float* db, void* workspace, size_t workspace_bytes, int split, mgs_stream_t stream) {
  return pw_backward("pointwise_wide_backward", true, B, Cin, Cout, n, x, g_y, w, dx, dw, db, workspace, workspace_bytes, split,
                     stream);
}

}  // extern "C"
