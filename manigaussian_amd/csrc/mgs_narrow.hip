// mgs_narrow.hip -- the Perceiver decoder's narrow-output 3x3x3 convolution with its pad folded into the addressing
// (agents/manigaussian_bc/perceiver_lang_io.py:322: trans_decoder = Conv3DBlock(128, 1, 3) = nn.Conv3d(128, 1, 3, padding=1,
// padding_mode='replicate') with bias on [B,128,100^3]), direct, fp32, NCDHW, Cin 1..256, Cout 1..4, VALU only.
//
// With c(i) = clamp(i, 0, n - 1) per dimension in replicate mode (in zeros mode a tap outside the volume contributes nothing):
//   forward          y[b,co,o]     = bias[co] + sum_ci sum_tap w[co,ci,tap] x[b,ci,c(o + tap - 1)]
//   backward-data    dx[b,ci,i]    = sum_co sum_{(o,tap): c(o + tap - 1) = i} w[co,ci,tap] g[b,co,o]
//   backward-weight  dw[co,ci,tap] = sum_b sum_o g[b,co,o] x[b,ci,c(o + tap - 1)]          db[co] = sum_b sum_o g[b,co,o]
// The padded volume never exists.  All three are gathers: every output element is written once by one thread from a sum whose terms
// and order depend on the shape alone.  No atomics, no workgroup waits for another, nothing to zero.
//
// The tile.  A group of 128 threads = 8 blocks along W x 8 rows along H x 2 blocks along D takes 32 x 8 x 8 voxels (W x H x D); a
// thread keeps a register block of 4 (D) x 4 (W) voxels of one row.  The halo box of one channel, 34 x 10 x 10 values, is staged in
// LDS, 27 values per thread, from offsets worked out once per tile (clamped to the volume in replicate mode; -1, a zero, for a
// voxel outside it in zeros mode).  Per channel and plane of the box a thread reads its 3 rows x 6 values as 8-byte LDS reads and
// feeds each to up to 3 (D) x 3 (W) of its 16 sums: 108 LDS words for 432 fused multiply-adds, against weights whose address is
// uniform across the wave (scalar loads, SGPR operands).
//
// Forward (nc_fwd_kernel).  One output channel gives 16 sums per thread and one million voxels 977 waves: too few to hide a load.
// So a workgroup is FOUR groups on the same tile; group k takes input channels k, k + 4, .. into a box of its own, the next channel's
// values in flight (in registers) while the current one is used, and the four partial sums meet in LDS and are added in ascending
// group order (group 0 starts from the bias).
//
// Backward-data (nc_bwd_data_kernel).  A workgroup of one group stages the tile's halo of g (zeros outside the volume) for all Cout
// once and then walks 16 input channels (blockIdx.y), all from LDS: dx needs no x.  In replicate mode a border voxel also collects
// what its replicated copies received.  Per dimension the sources of tap k' (which reads g at offset k' - 1 with weight w[2 - k'])
// are  k' = 0: {i - 1} and, at i = n - 1, {i};  k' = 1: {i};  k' = 2: {i + 1} and, at i = 0, {i}  (zeros outside), and the sources of
// a 3-D tap are the product of the three sets.  So along H the centre row is added to the row above (below) it at the last (first)
// row, along W the centre value to its neighbour in the same way -- a select per value, only in tiles that touch such a border --
// and along D, where the border is uniform across the wave, the centre plane is run through the third set of weights as well.
//
// Backward-weight and -bias (nc_bwd_weight_kernel; merge: mgs_records.hip).  The tiles, in their linear order, are cut into nrec <= 64 runs
// of tpr tiles; nrec and tpr depend on the shape alone.  A workgroup of one group takes two input channels at Cout = 1, else one (their
// sums have to fit the registers) and, per run, keeps 27 Cout sums per channel and Cout for db per thread over the run's tiles: per
// tile the box offsets and g of the thread's own 16 voxels are worked out and read once, then the channels' halo boxes of x go
// through LDS one after the other, the next one's values in flight while the current one is used.  At the end of a run the sums are
// added over the 128 threads in a fixed tree into the run's RECORD [Cout, 27 Cin + 1] in the workspace (the last column, db, by the
// workgroups of the first channel group).  `split` is the number of workgroups that share a channel group's runs: it decides who
// computes a record, not what the record is.  The merge launch sums the records in ascending order in double.
//
// Element offsets are 64-bit; indices inside a (batch, channel) row are 32-bit (D H W < 2^31).
#include "mgs_common.h"

namespace mgs {

constexpr int NC_MAX_CIN = 256, NC_MAX_COUT = 4;
constexpr int NC_TW = 32, NC_TH = 8, NC_TD = 8;     // a tile
constexpr int NC_GROUP = 128;                       // threads on a tile: 8 (W) x 8 (H) x 2 (D) register blocks of 4 (D) x 4 (W)
constexpr int NC_EW = NC_TW + 2, NC_EH = NC_TH + 2, NC_ED = NC_TD + 2;
constexpr int NC_PLANE = NC_EH * NC_EW, NC_VOL = NC_ED * NC_PLANE;
constexpr int NC_PER = (NC_VOL + NC_GROUP - 1) / NC_GROUP;   // staged values per thread
constexpr int NC_BOX = NC_PER * NC_GROUP;           // floats of a box in LDS (the last few are never read)
constexpr int NC_KG = 4;                            // the forward's groups per workgroup
constexpr int NC_DX_CIG = 16;                       // input channels per workgroup of backward-data
constexpr int NC_TAPS = 27;

struct NcGeom {
  int Cin, Cout;
  int D, H, W;
  int tD, tH, tW;      // tiles
  int zeros;           // the pad: 0 replicate, 1 zeros
  int vec;             // W is a multiple of 4: a thread's 4 voxels are one 16-byte access
  int64_t vol;
};

struct NcPos { int b, d0, h0, w0; };
__device__ __forceinline__ NcPos nc_tile_pos(uint32_t t, const NcGeom& g) {
  NcPos p;
  const uint32_t tw = t % (uint32_t)g.tW; t /= (uint32_t)g.tW;
  const uint32_t th = t % (uint32_t)g.tH; t /= (uint32_t)g.tH;
  const uint32_t td = t % (uint32_t)g.tD;
  p.b = (int)(t / (uint32_t)g.tD);
  p.d0 = (int)td * NC_TD; p.h0 = (int)th * NC_TH; p.w0 = (int)tw * NC_TW;
  return p;
}

// where thread t of a group finds its NC_PER values of the halo box of the tile at p, inside a (batch, channel) row: the voxel
// clamped to the volume, or -1 (a zero) for a box element that does not exist and, with `zeros`, for a voxel outside the volume
__device__ __forceinline__ void nc_offsets(int (&off)[NC_PER], int t, const NcPos& p, const NcGeom& g, bool zeros) {
#pragma unroll
  for (int u = 0; u < NC_PER; ++u) {
    const int e = t + u * NC_GROUP;
    const int d = e / NC_PLANE, r = e - d * NC_PLANE, h = r / NC_EW, c = r - h * NC_EW;
    const int id = p.d0 - 1 + d, ih = p.h0 - 1 + h, iw = p.w0 - 1 + c;
    const bool inside = (unsigned)id < (unsigned)g.D && (unsigned)ih < (unsigned)g.H && (unsigned)iw < (unsigned)g.W;
    const int cd = min(max(id, 0), g.D - 1), ch = min(max(ih, 0), g.H - 1), cw = min(max(iw, 0), g.W - 1);
    off[u] = (e < NC_VOL && (inside || !zeros)) ? (cd * g.H + ch) * g.W + cw : -1;
  }
}
// the same offsets kept in LDS (tab [NC_PER][NC_GROUP], never negative) for the kernels that stage channel after channel -- in
// registers they and the addresses made of them cost the waves that hide the loads; returns the mask of the -1s, bit u for value u
__device__ __forceinline__ uint32_t nc_offsets_to(int* tab, bool write, int t, const NcPos& p, const NcGeom& g, bool zeros) {
  int off[NC_PER];
  nc_offsets(off, t, p, g, zeros);
  uint32_t none = 0;
#pragma unroll
  for (int u = 0; u < NC_PER; ++u) {
    if (write) tab[u * NC_GROUP + t] = max(off[u], 0);
    none |= off[u] < 0 ? 1u << u : 0u;
  }
  return none;
}
// the loads alone (no branch around a load: an element that is not there loads the row's first one and drops it) ...
__device__ __forceinline__ void nc_fetch(float (&v)[NC_PER], const float* __restrict__ row, const int (&off)[NC_PER]) {
#pragma unroll
  for (int u = 0; u < NC_PER; ++u) v[u] = row[max(off[u], 0)];
}
__device__ __forceinline__ void nc_fetch(float (&v)[NC_PER], const float* __restrict__ row, const int* tab, int t) {
#pragma unroll
  for (int u = 0; u < NC_PER; ++u) v[u] = row[tab[u * NC_GROUP + t]];
}
// ... and their way into the box, which may come long after
__device__ __forceinline__ void nc_put(float* box, const float (&v)[NC_PER], const int (&off)[NC_PER], int t) {
#pragma unroll
  for (int u = 0; u < NC_PER; ++u) box[t + u * NC_GROUP] = off[u] < 0 ? 0.f : v[u];
}
__device__ __forceinline__ void nc_put(float* box, const float (&v)[NC_PER], uint32_t none, int t) {
#pragma unroll
  for (int u = 0; u < NC_PER; ++u) box[t + u * NC_GROUP] = (none >> u & 1u) ? 0.f : v[u];
}
// a thread's 3 rows x 6 values of one plane of the box (tp: its first value there, 8-byte aligned)
__device__ __forceinline__ void nc_rows(float (&xv)[3][6], const float* tp) {
#pragma unroll
  for (int kh = 0; kh < 3; ++kh)
#pragma unroll
    for (int c = 0; c < 6; c += 2) {
      const float2 q = *reinterpret_cast<const float2*>(tp + kh * NC_EW + c);
      xv[kh][c] = q.x; xv[kh][c + 1] = q.y;
    }
}
// Between the planes of a box: without it the compiler issues all six planes' reads first and holds 108 values where 18 do, which
// costs the waves that would hide those reads
__device__ __forceinline__ void nc_plane_fence() { __builtin_amdgcn_sched_barrier(0); }
__device__ __forceinline__ void nc_load4(float (&v)[4], const float* __restrict__ p, int n, bool vec) {   // n: how many exist (0..4)
  if (vec) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = k < n ? p[k] : 0.f;
  }
}
__device__ __forceinline__ void nc_store4(const float (&v)[4], float* __restrict__ p, int n, bool vec) {
  if (vec) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < n) p[k] = v[k];
  }
}

// ---- forward --------------------------------------------------------------------------------------------------------------------
template <int CO>
__global__ __launch_bounds__(NC_GROUP* NC_KG, CO == 1 ? 4 : (CO == 2 ? 3 : 2)) void nc_fwd_kernel(NcGeom g, const float* __restrict__ x, const float* __restrict__ w,
                                                                  const float* __restrict__ bias, float* __restrict__ y) {
  __shared__ __attribute__((aligned(16))) float boxes[NC_KG * NC_BOX];
  __shared__ int tab[NC_BOX];
  const int kg = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / NC_GROUP));
  const int t = threadIdx.x & (NC_GROUP - 1), tx = t & 7, ty = (t >> 3) & 7, tz = t >> 6;
  const NcPos p = nc_tile_pos(blockIdx.x, g);
  const uint32_t none = nc_offsets_to(tab, kg == 0, t, p, g, g.zeros != 0);
  float* box = boxes + kg * NC_BOX;
  const float* tp = box + (4 * tz) * NC_PLANE + ty * NC_EW + 4 * tx;
  const float* xb = x + (int64_t)p.b * g.Cin * g.vol;

  float acc[CO][4][4];
#pragma unroll
  for (int co = 0; co < CO; ++co) {
    const float b0 = (kg == 0 && bias) ? bias[co] : 0.f;
#pragma unroll
    for (int dz = 0; dz < 4; ++dz)
#pragma unroll
      for (int wx = 0; wx < 4; ++wx) acc[co][dz][wx] = b0;
  }

  float v[NC_PER];
  __syncthreads();
  if (kg < g.Cin) nc_fetch(v, xb + (int64_t)kg * g.vol, tab, t);
  for (int c0 = 0; c0 < g.Cin; c0 += NC_KG) {
    const int ci = c0 + kg;   // (uniform across the wave)
    __syncthreads();
    if (ci < g.Cin) nc_put(box, v, none, t);
    __syncthreads();
    if (ci + NC_KG < g.Cin) nc_fetch(v, xb + (int64_t)(ci + NC_KG) * g.vol, tab, t);   // in flight while this channel is used
    if (ci < g.Cin) {
      const float* wp = w + (int64_t)ci * NC_TAPS;
#pragma unroll
      for (int q = 0; q < 6; ++q) {
        float xv[3][6];
        nc_plane_fence();
        nc_rows(xv, tp + q * NC_PLANE);
#pragma unroll
        for (int kd = 0; kd < 3; ++kd) {
          const int dz = q - kd;
          if (dz < 0 || dz > 3) continue;
#pragma unroll
          for (int co = 0; co < CO; ++co)
#pragma unroll
            for (int kh = 0; kh < 3; ++kh)
#pragma unroll
              for (int kw = 0; kw < 3; ++kw) {
                const float wv = wp[(int64_t)co * g.Cin * NC_TAPS + kd * 9 + kh * 3 + kw];
#pragma unroll
                for (int wx = 0; wx < 4; ++wx) acc[co][dz][wx] = fmaf(wv, xv[kh][wx + kw], acc[co][dz][wx]);
              }
        }
      }
    }
  }

  // the four groups' sums, added in ascending group order by group 0, one output channel at a time
  const int oh = p.h0 + ty, ow = p.w0 + 4 * tx;
#pragma unroll
  for (int co = 0; co < CO; ++co) {
    __syncthreads();
    if (kg > 0) {
#pragma unroll
      for (int k = 0; k < 16; ++k) boxes[((kg - 1) * 16 + k) * NC_GROUP + t] = acc[co][k >> 2][k & 3];
    }
    __syncthreads();
    if (kg == 0) {
#pragma unroll
      for (int k = 0; k < 16; ++k)
#pragma unroll
        for (int o = 0; o < NC_KG - 1; ++o) acc[co][k >> 2][k & 3] += boxes[(o * 16 + k) * NC_GROUP + t];
      if (oh < g.H && ow < g.W) {
        float* yr = y + ((int64_t)p.b * CO + co) * g.vol;
#pragma unroll
        for (int dz = 0; dz < 4; ++dz) {
          const int od = p.d0 + 4 * tz + dz;
          if (od < g.D) nc_store4(acc[co][dz], yr + ((od * g.H + oh) * g.W + ow), g.W - ow, g.vec != 0);
        }
      }
    }
  }
}

// ---- backward-data ----------------------------------------------------------------------------------------------------------------
template <int CO>
__global__ __launch_bounds__(NC_GROUP, 4) void nc_bwd_data_kernel(NcGeom g, const float* __restrict__ gy, const float* __restrict__ w,
                                                               float* __restrict__ dx) {
  __shared__ __attribute__((aligned(16))) float boxes[CO * NC_BOX];
  const int t = threadIdx.x, tx = t & 7, ty = (t >> 3) & 7;
  const int tz = __builtin_amdgcn_readfirstlane(t >> 6);
  const NcPos p = nc_tile_pos(blockIdx.x, g);
  {
    int off[NC_PER];
    nc_offsets(off, t, p, g, true);
#pragma unroll 1
    for (int co = 0; co < CO; ++co) {
      float v[NC_PER];
      nc_fetch(v, gy + ((int64_t)p.b * CO + co) * g.vol, off);
      nc_put(boxes + co * NC_BOX, v, off, t);
    }
  }
  __syncthreads();

  const bool repl = g.zeros == 0;
  const int oh = p.h0 + ty, ow = p.w0 + 4 * tx, od0 = p.d0 + 4 * tz;
  // does the tile hold a first or last row or column?  (uniform across the workgroup)
  const bool edge_hw = repl && (p.h0 == 0 || p.h0 + NC_TH >= g.H || p.w0 == 0 || p.w0 + NC_TW >= g.W);
  const bool lo_h = repl && oh == 0, hi_h = repl && oh == g.H - 1;
  bool lo_w[4], hi_w[4];
#pragma unroll
  for (int wx = 0; wx < 4; ++wx) { lo_w[wx] = repl && ow + wx == 0; hi_w[wx] = repl && ow + wx == g.W - 1; }
  const float* tp = boxes + (4 * tz) * NC_PLANE + ty * NC_EW + 4 * tx;

  const int ci0 = (int)blockIdx.y * NC_DX_CIG, ci1 = min(ci0 + NC_DX_CIG, g.Cin);
  for (int ci = ci0; ci < ci1; ++ci) {
    float acc[4][4];
#pragma unroll
    for (int dz = 0; dz < 4; ++dz)
#pragma unroll
      for (int wx = 0; wx < 4; ++wx) acc[dz][wx] = 0.f;
#pragma unroll 1
    for (int co = 0; co < CO; ++co) {
      const float* wp = w + ((int64_t)co * g.Cin + ci) * NC_TAPS;
#pragma unroll
      for (int q = 0; q < 6; ++q) {
        float xv[3][6];
        nc_plane_fence();
        nc_rows(xv, tp + co * NC_BOX + q * NC_PLANE);
        // val[kh][kw][wx]: what tap (kh, kw) of voxel wx reads in this plane
        float val[3][3][4];
        if (edge_hw) {
#pragma unroll
          for (int c = 0; c < 6; ++c) {
            const float mid = xv[1][c];
            xv[0][c] += hi_h ? mid : 0.f;
            xv[2][c] += lo_h ? mid : 0.f;
          }
        }
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
          for (int wx = 0; wx < 4; ++wx) {
            const float mid = xv[kh][wx + 1];
            val[kh][0][wx] = xv[kh][wx];
            val[kh][1][wx] = mid;
            val[kh][2][wx] = xv[kh][wx + 2];
            if (edge_hw) {
              val[kh][0][wx] += hi_w[wx] ? mid : 0.f;
              val[kh][2][wx] += lo_w[wx] ? mid : 0.f;
            }
          }
        // plane q is what tap kd of voxel dz = q - kd reads; the weight of the flipped tap (kd, kh, kw) is w[26 - its index]
        auto apply = [&](int dz, int kd) {
#pragma unroll
          for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
              const float wv = wp[26 - (kd * 9 + kh * 3 + kw)];
#pragma unroll
              for (int wx = 0; wx < 4; ++wx) acc[dz][wx] = fmaf(wv, val[kh][kw][wx], acc[dz][wx]);
            }
        };
#pragma unroll
        for (int kd = 0; kd < 3; ++kd) {
          const int dz = q - kd;
          if (dz < 0 || dz > 3) continue;
          apply(dz, kd);
        }
        // ... and at the first (last) plane of the volume the centre plane stands for the replicated one in front of (behind) it too
        const int dc = q - 1;
        if (dc >= 0 && dc <= 3 && repl) {   // (uniform across the wave)
          if (od0 + dc == 0) apply(dc, 2);
          if (od0 + dc == g.D - 1) apply(dc, 0);
        }
      }
    }
    if (oh < g.H && ow < g.W) {
      float* dr = dx + ((int64_t)p.b * g.Cin + ci) * g.vol;
#pragma unroll
      for (int dz = 0; dz < 4; ++dz) {
        const int od = od0 + dz;
        if (od < g.D) nc_store4(acc[dz], dr + ((od * g.H + oh) * g.W + ow), g.W - ow, g.vec != 0);
      }
    }
  }
}

// ---- backward-weight and -bias -----------------------------------------------------------------------------------------------------
__device__ __forceinline__ float nc_wave_sum(float v) {   // the 64 lanes' values in a fixed tree; every lane gets the sum
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// the input channels a workgroup of the weight gradient takes: their 27 Cout sums each have to fit a thread's registers
template <int CO>
struct NcBw { static constexpr int CIG = CO == 1 ? 2 : 1; };

// One channel's halo box against the thread's 4 (D) x 4 (W) voxels: acc[co][tap] += g[co][voxel] x[voxel + tap].  A voxel outside the
// volume takes no part: its g is a zero, but its taps are clamped copies of border voxels, and 0 x NaN or 0 x inf would put a NaN
// into sums the voxel has nothing to do with.  Along D the voxels that exist are the first ndz (uniform across the wave: a skipped
// plane), along W the first nw; EDGE: nw < 4, the thread straddles the volume's end (W no multiple of 4 only) and the taps of its
// missing voxels are selected zeros.  A thread with no voxel at all does not come here.
template <int CO, bool EDGE>
__device__ __forceinline__ void nc_dw_planes(float (&acc)[CO][NC_TAPS], const float (&gv)[CO][4][4], const float* tp, int ndz, int nw) {
#pragma unroll
  for (int q = 0; q < 6; ++q) {
    float xv[3][6];
    nc_plane_fence();
    nc_rows(xv, tp + q * NC_PLANE);
#pragma unroll
    for (int kd = 0; kd < 3; ++kd) {
      const int dz = q - kd;
      if (dz < 0 || dz > 3) continue;
      if (dz >= ndz) continue;
#pragma unroll
      for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw)
#pragma unroll
          for (int wx = 0; wx < 4; ++wx) {
            const float xx = (EDGE && wx >= nw) ? 0.f : xv[kh][wx + kw];
#pragma unroll
            for (int co = 0; co < CO; ++co)
              acc[co][kd * 9 + kh * 3 + kw] = fmaf(gv[co][dz][wx], xx, acc[co][kd * 9 + kh * 3 + kw]);
          }
    }
  }
}

// grid = (workgroups per group of input channels, ceil(Cin / CIG) -- or 1 when dw is not wanted: then x is not read)
template <int CO>
__global__ __launch_bounds__(NC_GROUP, 2) void nc_bwd_weight_kernel(NcGeom g, uint32_t nrec, uint32_t tpr, uint32_t ntiles, int want_dw,
                                                                 const float* __restrict__ x, const float* __restrict__ gy,
                                                                 float* __restrict__ records) {
  constexpr int CIG = NcBw<CO>::CIG;
  constexpr int NW = CIG * CO * NC_TAPS, NS = NW + CO;   // a workgroup's sums: [channel of the group][co][tap], then [co] of db
  static_assert(NS <= NC_GROUP, "one thread per sum writes the record");
  __shared__ __attribute__((aligned(16))) float box[NC_BOX];
  __shared__ int tab[NC_BOX];
  __shared__ float red[2 * NS];
  const int ci0 = (int)blockIdx.y * CIG, nci = min(CIG, g.Cin - ci0);
  const int t = threadIdx.x, tx = t & 7, ty = (t >> 3) & 7, tz = t >> 6, lane = t & 63;
  const int cols = g.Cin * NC_TAPS + 1;
  const float* tp = box + (4 * tz) * NC_PLANE + ty * NC_EW + 4 * tx;

  for (uint32_t rec = blockIdx.x; rec < nrec; rec += gridDim.x) {
    float acc[CIG][CO][NC_TAPS], accb[CO];
#pragma unroll
    for (int co = 0; co < CO; ++co) {
      accb[co] = 0.f;
#pragma unroll
      for (int j = 0; j < CIG; ++j)
#pragma unroll
        for (int k = 0; k < NC_TAPS; ++k) acc[j][co][k] = 0.f;
    }
    const uint32_t t0 = rec * tpr, t1 = min(t0 + tpr, ntiles);
    for (uint32_t tile = t0; tile < t1; ++tile) {
      const NcPos p = nc_tile_pos(tile, g);
      // g of the thread's own voxels (zeros where there is none)
      float gv[CO][4][4];
      const int oh = p.h0 + ty, ow = p.w0 + 4 * tx;
#pragma unroll
      for (int co = 0; co < CO; ++co)
#pragma unroll
        for (int dz = 0; dz < 4; ++dz) {
          const int od = p.d0 + 4 * tz + dz;
          const bool live = od < g.D && oh < g.H && ow < g.W;
          const float* gr = gy + ((int64_t)p.b * CO + co) * g.vol;
          nc_load4(gv[co][dz], gr + (live ? (od * g.H + oh) * g.W + ow : 0), live ? g.W - ow : 0, g.vec != 0);
#pragma unroll
          for (int wx = 0; wx < 4; ++wx) {
            if (!live) gv[co][dz][wx] = 0.f;
            accb[co] += gv[co][dz][wx];
          }
        }
      if (!want_dw) continue;   // (uniform across the launch)
      const int nw = oh < g.H ? g.W - ow : 0;                                          // the thread's voxels along W that exist (<= 0: none)
      const int ndz = __builtin_amdgcn_readfirstlane(g.D - (p.d0 + 4 * tz));          // ... along D: tz is the wave
      float v[NC_PER];
      __syncthreads();   // (the last tile's offsets are no longer read)
      int ts = t;   // (opaque: or the 27 elements' box coordinates are kept across the tiles, 81 registers)
      asm volatile("" : "+v"(ts));
      const uint32_t none = nc_offsets_to(tab, true, ts, p, g, g.zeros != 0);   // (a thread reads back only what it wrote itself)
      const float* xb = x + ((int64_t)p.b * g.Cin + ci0) * g.vol;
      nc_fetch(v, xb, tab, t);
#pragma unroll
      for (int j = 0; j < CIG; ++j) {
        __syncthreads();
        if (j < nci) nc_put(box, v, none, t);
        __syncthreads();
        if (j + 1 < nci) nc_fetch(v, xb + (int64_t)(j + 1) * g.vol, tab, t);   // in flight while this channel is used
        if (j < nci && nw > 0) {
          if (nw >= 4) nc_dw_planes<CO, false>(acc[j], gv, tp, ndz, 4);
          else nc_dw_planes<CO, true>(acc[j], gv, tp, ndz, nw);
        }
      }
    }
    // the run's record: every sum over a wave's 64 lanes in a fixed tree, then wave 0's plus wave 1's
    __syncthreads();
#pragma unroll
    for (int j = 0; j < CIG; ++j)
#pragma unroll
      for (int co = 0; co < CO; ++co)
#pragma unroll
        for (int k = 0; k < NC_TAPS; ++k) {
          if (k % 9 == 0) nc_plane_fence();   // (nine sums' trees at a time: all of them at once would double the registers)
          const float s = nc_wave_sum(acc[j][co][k]);
          if (lane == 0) red[tz * NS + (j * CO + co) * NC_TAPS + k] = s;
        }
#pragma unroll
    for (int co = 0; co < CO; ++co) {
      const float sb = nc_wave_sum(accb[co]);
      if (lane == 0) red[tz * NS + NW + co] = sb;
    }
    __syncthreads();
    if (t < NS) {
      const float s = red[t] + red[NS + t];
      float* rp = records + (int64_t)rec * CO * cols;
      if (t < NW) {
        const int j = t / (CO * NC_TAPS), r = t - j * (CO * NC_TAPS), co = r / NC_TAPS, k = r - co * NC_TAPS;
        if (want_dw && j < nci) rp[(int64_t)co * cols + (ci0 + j) * NC_TAPS + k] = s;
      } else if (blockIdx.y == 0) {
        rp[(int64_t)(t - NW) * cols + cols - 1] = s;
      }
    }
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
struct NcShape {
  int64_t B, D, H, W, vol;
  int Cin, Cout;
  int64_t tiles[3], ntiles;     // per batch entry tiles[0] tiles[1] tiles[2]; ntiles includes B
  int64_t nrec, tpr;            // the records of dw | db
};

static bool nc_shape(int64_t B, int Cin, int Cout, int64_t D, int64_t H, int64_t W, NcShape* sh, const char** why) {
  if (Cin < 1 || Cin > NC_MAX_CIN) { *why = "Cin must be 1 to 256"; return false; }
  if (Cout < 1 || Cout > NC_MAX_COUT) { *why = "Cout must be 1 to 4"; return false; }
  if (B < 1 || D < 1 || H < 1 || W < 1) { *why = "B and every extent must be at least 1"; return false; }
  if (row_too_long(D, H, W)) { *why = "a (batch, channel) row must hold fewer than 2^31 elements"; return false; }
  const int64_t lim = 0x7fffffff;
  sh->B = B; sh->D = D; sh->H = H; sh->W = W; sh->vol = D * H * W; sh->Cin = Cin; sh->Cout = Cout;
  sh->tiles[0] = (D + NC_TD - 1) / NC_TD;
  sh->tiles[1] = (H + NC_TH - 1) / NC_TH;
  sh->tiles[2] = (W + NC_TW - 1) / NC_TW;
  const int64_t per = sh->tiles[0] * sh->tiles[1] * sh->tiles[2];
  if (B > lim / per) { *why = "B times the number of tiles exceeds 2^31 - 1"; return false; }
  sh->ntiles = B * per;
  const Runs runs = cut_runs(sh->ntiles, MAX_REC);
  sh->nrec = runs.n; sh->tpr = runs.per;
  return true;
}

static int nc_check(const char* fn, int64_t B, int Cin, int Cout, int64_t D, int64_t H, int64_t W, int zeros_pad, NcShape* sh) {
  const char* why = "";
  if (!nc_shape(B, Cin, Cout, D, H, W, sh, &why)) {
    set_error("%s: B = %lld, Cin = %d, Cout = %d, D H W = %lld x %lld x %lld: %s", fn, (long long)B, Cin, Cout, (long long)D,
              (long long)H, (long long)W, why);
    return MGS_ERR_INVALID_ARG;
  }
  if (zeros_pad != 0 && zeros_pad != 1) {
    set_error("%s: zeros_pad = %d (0: replicate, 1: zeros)", fn, zeros_pad);
    return MGS_ERR_INVALID_ARG;
  }
  return MGS_OK;
}

static NcGeom nc_geom(const NcShape& sh, int zeros_pad) {
  NcGeom g;
  g.Cin = sh.Cin; g.Cout = sh.Cout;
  g.D = (int)sh.D; g.H = (int)sh.H; g.W = (int)sh.W;
  g.tD = (int)sh.tiles[0]; g.tH = (int)sh.tiles[1]; g.tW = (int)sh.tiles[2];
  g.zeros = zeros_pad;
  g.vec = sh.W % 4 == 0;
  g.vol = sh.vol;
  return g;
}

// KERNEL<Cout> with the launch's Cout as a template argument
#define NC_LAUNCH(KERNEL, COUT, GRID, BLOCK, STREAM, ...)                                         \
  do {                                                                                            \
    switch (COUT) {                                                                               \
      case 1: hipLaunchKernelGGL((KERNEL<1>), GRID, BLOCK, 0, STREAM, __VA_ARGS__); break;        \
      case 2: hipLaunchKernelGGL((KERNEL<2>), GRID, BLOCK, 0, STREAM, __VA_ARGS__); break;        \
      case 3: hipLaunchKernelGGL((KERNEL<3>), GRID, BLOCK, 0, STREAM, __VA_ARGS__); break;        \
      default: hipLaunchKernelGGL((KERNEL<4>), GRID, BLOCK, 0, STREAM, __VA_ARGS__); break;       \
    }                                                                                             \
  } while (0)

}  // namespace mgs

using namespace mgs;

extern "C" {

size_t mgs_narrow_conv3d_workspace_bytes(int64_t B, int Cin, int Cout, int64_t D, int64_t H, int64_t W) {
  NcShape sh;
  const char* why;
  if (!nc_shape(B, Cin, Cout, D, H, W, &sh, &why)) return 0;
  return align_up((size_t)sh.nrec * (size_t)Cout * ((size_t)Cin * NC_TAPS + 1) * sizeof(float)) + ALIGN;
}

int mgs_narrow_conv3d_forward(int64_t B, int Cin, int Cout, int64_t D, int64_t H, int64_t W, int zeros_pad, const float* x,
                              const float* w, const float* bias, float* y, mgs_stream_t stream) {
  const char* fn = "narrow_conv3d_forward";
  NcShape sh;
  if (int rc = nc_check(fn, B, Cin, Cout, D, H, W, zeros_pad, &sh)) return rc;
  if (!x || !w || !y) { set_error("%s: NULL x, w or y", fn); return MGS_ERR_INVALID_ARG; }
  if (misaligned16(x) || misaligned16(w) || misaligned16(y) || misaligned16(bias)) {
    set_error("%s: x, w, bias and y must be 16-byte aligned", fn);
    return MGS_ERR_INVALID_ARG;
  }
  const NcGeom g = nc_geom(sh, zeros_pad);
  NC_LAUNCH(nc_fwd_kernel, Cout, dim3((unsigned)sh.ntiles), dim3(NC_GROUP * NC_KG), (hipStream_t)stream, g, x, w, bias, y);
  return launch_done(fn);
}

int mgs_narrow_conv3d_backward(int64_t B, int Cin, int Cout, int64_t D, int64_t H, int64_t W, int zeros_pad, const float* x,
                               const float* g_y, const float* w, float* dx, float* dw, float* db, void* workspace,
                               size_t workspace_bytes, int split, mgs_stream_t stream) {
  const char* fn = "narrow_conv3d_backward";
  NcShape sh;
  if (int rc = nc_check(fn, B, Cin, Cout, D, H, W, zeros_pad, &sh)) return rc;
  if (int rc = split_check(fn, split)) return rc;
  if (!dx && !dw && !db) { set_error("%s: NULL dx, dw and db: no gradient is asked for", fn); return MGS_ERR_INVALID_ARG; }
  if (!g_y || (dx && !w) || (dw && !x)) { set_error("%s: NULL g_y, w (needed for dx) or x (needed for dw)", fn); return MGS_ERR_INVALID_ARG; }
  if (misaligned16(x) || misaligned16(g_y) || misaligned16(w) || misaligned16(dx) || misaligned16(dw) || misaligned16(db)) {
    set_error("%s: x, g_y, w, dx, dw and db must be 16-byte aligned", fn);
    return MGS_ERR_INVALID_ARG;
  }
  const bool sums = dw || db;
  if (sums)
    if (int rc = records_workspace(fn, workspace, workspace_bytes, mgs_narrow_conv3d_workspace_bytes(B, Cin, Cout, D, H, W))) return rc;
  hipStream_t s = (hipStream_t)stream;
  const NcGeom g = nc_geom(sh, zeros_pad);
  if (dx) {
    const dim3 grid((unsigned)sh.ntiles, (unsigned)((Cin + NC_DX_CIG - 1) / NC_DX_CIG));
    NC_LAUNCH(nc_bwd_data_kernel, Cout, grid, dim3(NC_GROUP), s, g, g_y, w, dx);
  }
  if (sums) {
    const int64_t wgs = split_clamp(split, MAX_REC, sh.nrec);
    float* records = reinterpret_cast<float*>(workspace);
    const int want_dw = dw != nullptr;
    const int cig = Cout == 1 ? NcBw<1>::CIG : 1;
    const dim3 grid((unsigned)wgs, (unsigned)(want_dw ? (Cin + cig - 1) / cig : 1));
    NC_LAUNCH(nc_bwd_weight_kernel, Cout, grid, dim3(NC_GROUP), s, g, (uint32_t)sh.nrec, (uint32_t)sh.tpr, (uint32_t)sh.ntiles,
              want_dw, x, g_y, records);
    launch_records_merge(sh.nrec, Cout, Cin * NC_TAPS + 1, Cin * NC_TAPS, records, dw, db, s);
  }
  return launch_done(fn);
}

}  // extern "C"
