// mgs_volume.hip -- what the Perceiver decoder does to its 100^3 volumes between the convolutions
// (agents/manigaussian_bc/perceiver_lang_io.py:488-499, helpers/network_utils.py:129-171, 374-391), fused, fp32:
//
//   out = replicate_pad(trilinear_upsample(cat(sources, 1), scale, align_corners = False), pad)
//
// Per axis (source length n, scale s, pad p), for the padded output index op:
//   o = clamp(op - p, 0, s n - 1);  src = max((o + 0.5) / s - 0.5, 0);  i0 = floor(src);  lambda = src - i0;  i1 = min(i0 + 1, n - 1)
// with weight 1 - lambda on i0 and lambda on i1; the 3-D weight is the product of the three axes' weights.  1 / s and lambda are
// fp32, as in torch.  Interpolation and padding act per channel, so the concatenation is only a choice of base pointer.
//
// Forward, ONE launch: a lane owns one aligned 16-byte vector of the flat padded output and writes it once.  The flat index is
// split into (batch x channel, z, y, x) by multiply-and-shift (VolDiv); the z and y taps and the source row pointers are found
// once per vector when its four elements lie in one output row (else per element).  COPY (scale == 1) reads one value per
// element -- one 16-byte load at any float address where the four lie inside the source row -- and is a bit-exact copy.
//
// Backward is a gather: per axis, source index i receives the padded outputs op whose clamped src lies within 1 of i, weight
// max(0, 1 - |min(src, n - 1) - i|) -- the same two weights seen from the source's side (src > n - 1 is where i1 was clamped onto
// i0).  The candidates are a fixed index range around s i, widened to the replicated border at the two ends, walked in
// ascending order: every gradient element is written once, by one lane, from a sum in a fixed order.  Nothing is zero-filled
// and no lane adds into memory another lane writes: the same bits from run to run.
//   scale > 1: vol_bwd_xy_kernel reduces x and y for every padded z-plane into the workspace [B C, s D + 2 p, H, W];
//              vol_bwd_z_kernel reduces z and writes each source's gradient (grid.y = source).
//   COPY:      one launch (grid.y = source), a lane per aligned 16-byte vector of a source's gradient; interior elements are
//              one value each (a 16-byte load where the four are interior), border elements sum their (p + 1)-wide ranges.
//
// Indices inside the padded output, a source's gradient and the workspace are 32-bit (each at most 2^31 - 1 elements, checked);
// a source's element offset b stride_b + c stride_c is 64-bit.
#include <math.h>

#include "mgs_common.h"

namespace mgs {

constexpr int VOL_THREADS = 256;
constexpr int VOL_SRC = MGS_VOLUME_MAX_SOURCES;
constexpr int64_t VOL_MAX_ELEMS = 0x7fffffff;

typedef float volf4 __attribute__((ext_vector_type(4)));
typedef volf4 volf4_any __attribute__((aligned(4)));  // a 16-byte access at any float address

// n / d for n < 2^31 and 1 <= d < 2^31: (n mul) >> shift with mul = floor(2^shift / d) + 1, shift = 31 + ceil(log2 d)
struct VolDiv { uint32_t mul, shift; };
static VolDiv vol_div(uint32_t d) {
  uint32_t s = 0;
  while (((uint64_t)1 << s) < d) ++s;
  VolDiv r;
  r.shift = 31 + s;
  r.mul = (uint32_t)((((uint64_t)1 << r.shift) / d) + 1);
  return r;
}
__device__ __forceinline__ uint32_t vol_quot(uint32_t n, const VolDiv& d) { return (uint32_t)(((uint64_t)n * d.mul) >> d.shift); }

struct VolGeom {
  uint32_t D, H, W;       // the sources' spatial shape
  uint32_t Do, Ho, Wo;    // the padded output's
  uint32_t Ct;            // channels of the concatenation
  uint32_t nsrc, scale, pad;
  uint32_t total;         // elements the launch covers (forward: the padded output; xy pass: the workspace)
  float inv_s;            // (float)(1.0 / scale)
  VolDiv dW, dH, dD, dWo, dHo, dDo, dCt;
  VolDiv dC[VOL_SRC];
  uint32_t C[VOL_SRC], cbeg[VOL_SRC];  // a source's channels and its first channel in the concatenation
  const float* src[VOL_SRC];
  int64_t sb[VOL_SRC], sc[VOL_SRC];
  float* gsrc[VOL_SRC];   // backward: each source's gradient [B, C_k, D, H, W]
};

// ---- the per-axis formula -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t vol_unpad(uint32_t op, uint32_t n_up, uint32_t pad) {
  const int o = (int)op - (int)pad;
  return (uint32_t)min(max(o, 0), (int)n_up - 1);
}
__device__ __forceinline__ float vol_src(uint32_t op, uint32_t n, const VolGeom& g) {
  const uint32_t o = vol_unpad(op, g.scale * n, g.pad);
  return fmaxf(g.inv_s * ((float)o + 0.5f) - 0.5f, 0.f);
}
struct VolTap { uint32_t i0, i1; float lam; };
__device__ __forceinline__ VolTap vol_tap(uint32_t op, uint32_t n, const VolGeom& g) {
  const float src = vol_src(op, n, g);
  VolTap t;
  t.i0 = min((uint32_t)src, n - 1);
  t.i1 = min(t.i0 + 1, n - 1);
  t.lam = src - (float)t.i0;
  return t;
}
// the weight of padded output op on source index i
__device__ __forceinline__ float vol_weight(uint32_t op, uint32_t i, uint32_t n, const VolGeom& g) {
  const float src = fminf(vol_src(op, n, g), (float)(n - 1));
  return fmaxf(0.f, 1.f - fabsf(src - (float)i));
}
// [lo, hi]: padded outputs that can reach source index i.  The unpadded o with |src(o) - i| < 1 are s i - s / 2 ... s i + 3 s / 2 - 1
// (integer halves); the range below holds one more index on either side, 1 / s in src where fp32 moves src by a few 1e-6 at most,
// and runs out to the replicated border where it touches an end.
__device__ __forceinline__ void vol_range(uint32_t i, uint32_t n, const VolGeom& g, uint32_t& lo, uint32_t& hi) {
  const int s = (int)g.scale, p = (int)g.pad, last = s * (int)n - 1;
  const int olo = s * (int)i - s / 2 - 1, ohi = s * (int)i + (3 * s) / 2;
  lo = olo <= 0 ? 0u : (uint32_t)(olo + p);
  hi = ohi >= last ? (uint32_t)(last + 2 * p) : (uint32_t)(ohi + p);
}
// ... and for COPY, where op reaches i = clamp(op - p, 0, n - 1) alone
__device__ __forceinline__ void vol_copy_range(uint32_t i, uint32_t n, uint32_t p, uint32_t& lo, uint32_t& hi) {
  lo = i == 0 ? 0u : i + p;
  hi = i == n - 1 ? i + 2 * p : i + p;
}

// the source that holds channel c of the concatenation: that channel's first element for batch b
__device__ __forceinline__ const float* vol_channel(const VolGeom& g, uint32_t b, uint32_t c) {
  const float* p = g.src[0];
  int64_t sb = g.sb[0], sc = g.sc[0];
  uint32_t c0 = 0;
  if (g.nsrc > 1 && c >= g.cbeg[1]) { p = g.src[1]; sb = g.sb[1]; sc = g.sc[1]; c0 = g.cbeg[1]; }
  if (g.nsrc > 2 && c >= g.cbeg[2]) { p = g.src[2]; sb = g.sb[2]; sc = g.sc[2]; c0 = g.cbeg[2]; }
  if (g.nsrc > 3 && c >= g.cbeg[3]) { p = g.src[3]; sb = g.sb[3]; sc = g.sc[3]; c0 = g.cbeg[3]; }
  return p + (int64_t)b * sb + (int64_t)(c - c0) * sc;
}

// ---- forward --------------------------------------------------------------------------------------------------------------------
// the source rows under one output row (z0 y0, z0 y1, z1 y0, z1 y1) and the z and y lambdas (COPY: one row)
struct VolRow { const float* r[4]; float lz, ly; };
template <bool COPY>
__device__ __forceinline__ VolRow vol_row(const VolGeom& g, uint32_t bc, uint32_t oz, uint32_t oy) {
  const uint32_t b = vol_quot(bc, g.dCt), c = bc - b * g.Ct;
  const float* base = vol_channel(g, b, c);
  VolRow R;
  if (COPY) {
    const uint32_t iz = vol_unpad(oz, g.D, g.pad), iy = vol_unpad(oy, g.H, g.pad);
    R.r[0] = R.r[1] = R.r[2] = R.r[3] = base + (iz * g.H + iy) * g.W;
    R.lz = R.ly = 0.f;
  } else {
    const VolTap z = vol_tap(oz, g.D, g), y = vol_tap(oy, g.H, g);
    R.r[0] = base + (z.i0 * g.H + y.i0) * g.W;
    R.r[1] = base + (z.i0 * g.H + y.i1) * g.W;
    R.r[2] = base + (z.i1 * g.H + y.i0) * g.W;
    R.r[3] = base + (z.i1 * g.H + y.i1) * g.W;
    R.lz = z.lam; R.ly = y.lam;
  }
  return R;
}
// (1 - t) a + t b as a + t (b - a): where a tap was clamped onto its neighbour (a == b) the value passes through exactly
__device__ __forceinline__ float vol_lerp(float a, float b, float t) { return fmaf(t, b - a, a); }
__device__ __forceinline__ float vol_column(const VolRow& R, uint32_t i) {
  return vol_lerp(vol_lerp(R.r[0][i], R.r[1][i], R.ly), vol_lerp(R.r[2][i], R.r[3][i], R.ly), R.lz);
}
// The same sample as a sum of weighted taps, the form F.interpolate computes: with an infinite tap a, a + t (b - a) is inf - inf =
// NaN where (1 - t) a + t b is the infinity.  Taken only where the lerp form gave a NaN, so finite volumes keep their bits.
__device__ __forceinline__ float vol_mix(float a, float b, float t) { return (1.f - t) * a + t * b; }
__device__ __forceinline__ float vol_column_mix(const VolRow& R, uint32_t i) {
  return vol_mix(vol_mix(R.r[0][i], R.r[1][i], R.ly), vol_mix(R.r[2][i], R.r[3][i], R.ly), R.lz);
}
template <bool COPY>
__device__ __forceinline__ float vol_sample(const VolGeom& g, const VolRow& R, uint32_t ox) {
  if (COPY) return R.r[0][vol_unpad(ox, g.W, g.pad)];
  const VolTap x = vol_tap(ox, g.W, g);
  return vol_lerp(vol_column(R, x.i0), vol_column(R, x.i1), x.lam);
}
// (ox goes through an opaque move: the compiler must not keep the first form's taps in registers for this one)
__device__ __forceinline__ float vol_sample_mix(const VolGeom& g, const VolRow& R, uint32_t ox) {
  asm volatile("" : "+v"(ox));
  const VolTap x = vol_tap(ox, g.W, g);
  return vol_mix(vol_column_mix(R, x.i0), vol_column_mix(R, x.i1), x.lam);
}

template <bool COPY>
__global__ __launch_bounds__(VOL_THREADS) void vol_fwd_kernel(VolGeom g, float* __restrict__ out) {
  const uint32_t e = 4u * (blockIdx.x * VOL_THREADS + threadIdx.x);
  if (e >= g.total) return;
  const uint32_t count = min(4u, g.total - e);
  const uint32_t q1 = vol_quot(e, g.dWo), q2 = vol_quot(q1, g.dHo);
  uint32_t ox = e - q1 * g.Wo, oy = q1 - q2 * g.Ho;
  uint32_t bc = vol_quot(q2, g.dDo), oz = q2 - bc * g.Do;
  VolRow R = vol_row<COPY>(g, bc, oz, oy);
  volf4 v;
  if (count == 4 && ox + 3 < g.Wo) {  // one output row
    if (COPY && ox >= g.pad && ox + 3 - g.pad < g.W) {
      v = *reinterpret_cast<const volf4_any*>(R.r[0] + (ox - g.pad));
    } else {
      v.x = vol_sample<COPY>(g, R, ox);
      v.y = vol_sample<COPY>(g, R, ox + 1);
      v.z = vol_sample<COPY>(g, R, ox + 2);
      v.w = vol_sample<COPY>(g, R, ox + 3);
      if (!COPY && ((v.x != v.x) | (v.y != v.y) | (v.z != v.z) | (v.w != v.w))) {   // a NaN or an infinity among the taps
        v.x = vol_sample_mix(g, R, ox);
        v.y = vol_sample_mix(g, R, ox + 1);
        v.z = vol_sample_mix(g, R, ox + 2);
        v.w = vol_sample_mix(g, R, ox + 3);
      }
    }
    *reinterpret_cast<volf4*>(out + e) = v;
    return;
  }
  // the vector runs over the end of an output row (or of the output): element by element, a new row where one begins
  float t[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) {
    if (j < count) {
      t[j] = vol_sample<COPY>(g, R, ox);
      if (!COPY && t[j] != t[j]) t[j] = vol_sample_mix(g, R, ox);
      if (++ox == g.Wo && j + 1 < count) {
        ox = 0;
        if (++oy == g.Ho) {
          oy = 0;
          if (++oz == g.Do) { oz = 0; ++bc; }
        }
        R = vol_row<COPY>(g, bc, oz, oy);
      }
    }
  }
  if (count == 4) {
    v.x = t[0]; v.y = t[1]; v.z = t[2]; v.w = t[3];
    *reinterpret_cast<volf4*>(out + e) = v;
  } else {
#pragma unroll
    for (uint32_t j = 0; j < 3; ++j)
      if (j < count) out[e + j] = t[j];
  }
}

// ---- backward, scale > 1 --------------------------------------------------------------------------------------------------------
// workspace[row, iy, ix] = sum_opy sum_opx w_y w_x g_out[row, opy, opx], row = (b Ct + c) Do + opz: one lane per element
__global__ __launch_bounds__(VOL_THREADS) void vol_bwd_xy_kernel(VolGeom g, const float* __restrict__ g_out, float* __restrict__ ws) {
  const uint32_t t = blockIdx.x * VOL_THREADS + threadIdx.x;
  if (t >= g.total) return;
  const uint32_t q1 = vol_quot(t, g.dW), ix = t - q1 * g.W;
  const uint32_t row = vol_quot(q1, g.dH), iy = q1 - row * g.H;
  const float* plane = g_out + row * (g.Ho * g.Wo);
  uint32_t ylo, yhi, xlo, xhi;
  vol_range(iy, g.H, g, ylo, yhi);
  vol_range(ix, g.W, g, xlo, xhi);
  float acc = -0.f;
  for (uint32_t opy = ylo; opy <= yhi; ++opy) {
    const float wy = vol_weight(opy, iy, g.H, g);
    if (wy == 0.f) continue;  // (the spare rows of the range, mostly)
    const float* line = plane + opy * g.Wo;
    float a = -0.f;
    for (uint32_t opx = xlo; opx <= xhi; ++opx) a = fmaf(vol_weight(opx, ix, g.W, g), line[opx], a);
    acc = fmaf(wy, a, acc);
  }
  ws[t] = acc;
}

// g_src[k][b, cc, iz, iy, ix] = sum_opz w_z workspace[(b Ct + cbeg_k + cc) Do + opz, iy, ix]: one lane per element, grid.y = k
__global__ __launch_bounds__(VOL_THREADS) void vol_bwd_z_kernel(VolGeom g, const float* __restrict__ ws) {
  const uint32_t k = blockIdx.y;
  uint32_t Ck = g.C[0], c0 = 0;
  VolDiv dCk = g.dC[0];
  float* dst = g.gsrc[0];
#pragma unroll
  for (int j = 1; j < VOL_SRC; ++j)
    if (k == (uint32_t)j) { Ck = g.C[j]; c0 = g.cbeg[j]; dCk = g.dC[j]; dst = g.gsrc[j]; }
  const uint32_t HW = g.H * g.W;
  const uint32_t u = blockIdx.x * VOL_THREADS + threadIdx.x;
  if (u >= (g.total / g.Ct) * Ck) return;  // total = B Ct D H W here
  const uint32_t q1 = vol_quot(u, g.dW), q2 = vol_quot(q1, g.dH);
  const uint32_t xy = u - q2 * HW;
  const uint32_t r = vol_quot(q2, g.dD), iz = q2 - r * g.D;
  const uint32_t b = vol_quot(r, dCk), cc = r - b * Ck;
  const float* col = ws + ((b * g.Ct + c0 + cc) * g.Do) * HW + xy;
  uint32_t zlo, zhi;
  vol_range(iz, g.D, g, zlo, zhi);
  float acc = -0.f;
  for (uint32_t opz = zlo; opz <= zhi; ++opz) acc = fmaf(vol_weight(opz, iz, g.D, g), col[opz * HW], acc);
  dst[u] = acc;
}

// ---- backward, COPY -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float vol_copy_grad(const VolGeom& g, const float* __restrict__ vol, uint32_t iz, uint32_t iy, uint32_t ix) {
  uint32_t zlo, zhi, ylo, yhi, xlo, xhi;
  vol_copy_range(iz, g.D, g.pad, zlo, zhi);
  vol_copy_range(iy, g.H, g.pad, ylo, yhi);
  vol_copy_range(ix, g.W, g.pad, xlo, xhi);
  float acc = -0.f;  // (-0 + x = x for every x: a single term passes through bit for bit)
  for (uint32_t z = zlo; z <= zhi; ++z)
    for (uint32_t y = ylo; y <= yhi; ++y) {
      const float* line = vol + (z * g.Ho + y) * g.Wo;
      for (uint32_t x = xlo; x <= xhi; ++x) acc += line[x];
    }
  return acc;
}

// one lane per aligned 16-byte vector of source k's gradient (grid.y = k); total = B Ct D H W
__global__ __launch_bounds__(VOL_THREADS) void vol_bwd_copy_kernel(VolGeom g, const float* __restrict__ g_out) {
  const uint32_t k = blockIdx.y;
  uint32_t Ck = g.C[0], c0 = 0;
  VolDiv dCk = g.dC[0];
  float* dst = g.gsrc[0];
#pragma unroll
  for (int j = 1; j < VOL_SRC; ++j)
    if (k == (uint32_t)j) { Ck = g.C[j]; c0 = g.cbeg[j]; dCk = g.dC[j]; dst = g.gsrc[j]; }
  const uint32_t elems = (g.total / g.Ct) * Ck;
  const uint32_t u = 4u * (blockIdx.x * VOL_THREADS + threadIdx.x);
  if (u >= elems) return;
  const uint32_t count = min(4u, elems - u);
  const uint32_t q1 = vol_quot(u, g.dW), q2 = vol_quot(q1, g.dH);
  uint32_t ix = u - q1 * g.W, iy = q1 - q2 * g.H;
  uint32_t r = vol_quot(q2, g.dD), iz = q2 - r * g.D;
  const uint32_t per = g.Do * g.Ho * g.Wo;  // the padded volume of one (batch, channel)
  const uint32_t p = g.pad;
  {
    const uint32_t b = vol_quot(r, dCk), cc = r - b * Ck;
    const bool inside = p == 0 || (iz > 0 && iz + 1 < g.D && iy > 0 && iy + 1 < g.H && ix > 0 && ix + 4 < g.W);
    if (count == 4 && ix + 3 < g.W && inside) {
      const float* at = g_out + (b * g.Ct + c0 + cc) * per + ((iz + p) * g.Ho + (iy + p)) * g.Wo + (ix + p);
      *reinterpret_cast<volf4*>(dst + u) = *reinterpret_cast<const volf4_any*>(at);
      return;
    }
  }
  float t[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) {
    if (j < count) {
      const uint32_t b = vol_quot(r, dCk), cc = r - b * Ck;
      t[j] = vol_copy_grad(g, g_out + (b * g.Ct + c0 + cc) * per, iz, iy, ix);
      if (++ix == g.W) {
        ix = 0;
        if (++iy == g.H) {
          iy = 0;
          if (++iz == g.D) { iz = 0; ++r; }
        }
      }
    }
  }
  if (count == 4) {
    volf4 v;
    v.x = t[0]; v.y = t[1]; v.z = t[2]; v.w = t[3];
    *reinterpret_cast<volf4*>(dst + u) = v;
  } else {
#pragma unroll
    for (uint32_t j = 0; j < 3; ++j)
      if (j < count) dst[u + j] = t[j];
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
static bool vol_misaligned(const void* p, uintptr_t to) { return (reinterpret_cast<uintptr_t>(p) & (to - 1)) != 0; }

// the shape part of the checks, shared by the three entry points; *out_elems = elements of the padded output
static int vol_check_shape(const char* fn, const MgsVolumeArgs* a, int64_t* out_elems, int64_t* channels) {
  if (!a) { set_error("%s: NULL arguments", fn); return MGS_ERR_INVALID_ARG; }
  if (a->scale < 1 || a->scale > MGS_VOLUME_MAX_SCALE || a->pad < 0 || a->pad > MGS_VOLUME_MAX_PAD) {
    set_error("%s: scale = %d (1..%d), pad = %d (0..%d)", fn, a->scale, MGS_VOLUME_MAX_SCALE, a->pad, MGS_VOLUME_MAX_PAD);
    return MGS_ERR_INVALID_ARG;
  }
  if (a->nsrc < 1 || a->nsrc > MGS_VOLUME_MAX_SOURCES) {
    set_error("%s: nsrc = %d (1..%d sources)", fn, a->nsrc, MGS_VOLUME_MAX_SOURCES);
    return MGS_ERR_INVALID_ARG;
  }
  if (a->B < 0 || a->D < 1 || a->H < 1 || a->W < 1) {
    set_error("%s: B = %d (>= 0), D = %d, H = %d, W = %d (each >= 1)", fn, a->B, a->D, a->H, a->W);
    return MGS_ERR_INVALID_ARG;
  }
  int64_t Ct = 0;
  for (int k = 0; k < a->nsrc; ++k) {
    if (a->C[k] < 1) { set_error("%s: C[%d] = %d (>= 1)", fn, k, a->C[k]); return MGS_ERR_INVALID_ARG; }
    Ct += a->C[k];
  }
  const int64_t B = a->B > 0 ? a->B : 1;  // (the limits of an empty batch are those of a batch of one)
  const int64_t Do = (int64_t)a->scale * a->D + 2 * a->pad, Ho = (int64_t)a->scale * a->H + 2 * a->pad;
  const int64_t Wo = (int64_t)a->scale * a->W + 2 * a->pad;
  // (every factor is below 2^35: the products are taken one factor at a time against the limit)
  int64_t n = B * Ct;
  const int64_t dims[3] = {Do, Ho, Wo};
  for (int j = 0; j < 3 && n <= VOL_MAX_ELEMS; ++j) n = dims[j] > VOL_MAX_ELEMS / n ? VOL_MAX_ELEMS + 1 : n * dims[j];
  if (n > VOL_MAX_ELEMS) {
    set_error("%s: the padded output [%d, %lld, %lld, %lld, %lld] exceeds 2^31 - 1 elements", fn, a->B, (long long)Ct, (long long)Do,
              (long long)Ho, (long long)Wo);
    return MGS_ERR_INVALID_ARG;
  }
  *out_elems = n;  // (a source has no more elements than the output: scale >= 1, pad >= 0)
  *channels = Ct;
  return MGS_OK;
}

static void vol_geom(const MgsVolumeArgs* a, int64_t Ct, VolGeom* g) {
  g->D = (uint32_t)a->D; g->H = (uint32_t)a->H; g->W = (uint32_t)a->W;
  g->scale = (uint32_t)a->scale; g->pad = (uint32_t)a->pad; g->nsrc = (uint32_t)a->nsrc;
  g->Do = g->scale * g->D + 2 * g->pad; g->Ho = g->scale * g->H + 2 * g->pad; g->Wo = g->scale * g->W + 2 * g->pad;
  g->Ct = (uint32_t)Ct;
  g->total = 0;
  g->inv_s = (float)(1.0 / (double)a->scale);
  g->dW = vol_div(g->W); g->dH = vol_div(g->H); g->dD = vol_div(g->D);
  g->dWo = vol_div(g->Wo); g->dHo = vol_div(g->Ho); g->dDo = vol_div(g->Do); g->dCt = vol_div(g->Ct);
  uint32_t c = 0;
  for (int k = 0; k < VOL_SRC; ++k) {
    const bool used = k < a->nsrc;
    g->C[k] = used ? (uint32_t)a->C[k] : 1u;
    g->dC[k] = vol_div(g->C[k]);
    g->cbeg[k] = c;
    c += used ? g->C[k] : 0u;
    g->src[k] = used ? a->src[k] : nullptr;
    g->sb[k] = used ? a->stride_b[k] : 0;
    g->sc[k] = used ? a->stride_c[k] : 0;
    g->gsrc[k] = nullptr;
  }
}

static size_t vol_workspace(const MgsVolumeArgs* a, int64_t Ct) {
  if (a->scale == 1) return ALIGN;  // the copy's backward is one launch
  const int64_t B = a->B > 0 ? a->B : 1;
  const size_t n = (size_t)(B * Ct) * (size_t)(a->scale * a->D + 2 * a->pad) * (size_t)a->H * (size_t)a->W;
  return align_up(n * sizeof(float)) + ALIGN;
}

static unsigned vol_blocks(int64_t lanes) { return (unsigned)((lanes + VOL_THREADS - 1) / VOL_THREADS); }

}  // namespace mgs

using namespace mgs;

extern "C" {

size_t mgs_volume_workspace_bytes(const MgsVolumeArgs* a) {
  int64_t out_elems, Ct;
  if (vol_check_shape("volume_workspace_bytes", a, &out_elems, &Ct) != MGS_OK) return 0;
  return vol_workspace(a, Ct);
}

int mgs_volume_resample_pad_forward(const MgsVolumeArgs* a, float* out, mgs_stream_t stream) {
  const char* fn = "volume_resample_pad_forward";
  int64_t out_elems, Ct;
  int rc = vol_check_shape(fn, a, &out_elems, &Ct);
  if (rc != MGS_OK) return rc;
  if (!out || vol_misaligned(out, 16)) { set_error("%s: out is NULL or not 16-byte aligned", fn); return MGS_ERR_INVALID_ARG; }
  for (int k = 0; k < a->nsrc; ++k)
    if (!a->src[k] || vol_misaligned(a->src[k], 4)) {
      set_error("%s: src[%d] is NULL or not 4-byte aligned", fn, k);
      return MGS_ERR_INVALID_ARG;
    }
  if (a->B == 0) return MGS_OK;
  VolGeom g;
  vol_geom(a, Ct, &g);
  g.total = (uint32_t)out_elems;
  const dim3 grid(vol_blocks((out_elems + 3) / 4)), block(VOL_THREADS);
  hipStream_t s = (hipStream_t)stream;
  if (a->scale == 1) hipLaunchKernelGGL((vol_fwd_kernel<true>), grid, block, 0, s, g, out);
  else hipLaunchKernelGGL((vol_fwd_kernel<false>), grid, block, 0, s, g, out);
  return launch_done(fn);
}

int mgs_volume_resample_pad_backward(const MgsVolumeArgs* a, const float* g_out, float* const* g_src, void* workspace,
                                     size_t workspace_bytes, mgs_stream_t stream) {
  const char* fn = "volume_resample_pad_backward";
  int64_t out_elems, Ct;
  int rc = vol_check_shape(fn, a, &out_elems, &Ct);
  if (rc != MGS_OK) return rc;
  if (!g_out || vol_misaligned(g_out, 4)) { set_error("%s: g_out is NULL or not 4-byte aligned", fn); return MGS_ERR_INVALID_ARG; }
  if (!g_src) { set_error("%s: NULL g_src", fn); return MGS_ERR_INVALID_ARG; }
  for (int k = 0; k < a->nsrc; ++k)
    if (!g_src[k] || vol_misaligned(g_src[k], 16)) {
      set_error("%s: g_src[%d] is NULL or not 16-byte aligned", fn, k);
      return MGS_ERR_INVALID_ARG;
    }
  if (!workspace || vol_misaligned(workspace, 16)) {
    set_error("%s: the workspace is NULL or not 16-byte aligned", fn);
    return MGS_ERR_INVALID_ARG;
  }
  const size_t need = vol_workspace(a, Ct);
  if (workspace_short(fn, workspace_bytes, need)) return MGS_ERR_INVALID_ARG;  // (this entry point's code for it)
  if (a->B == 0) return MGS_OK;
  VolGeom g;
  vol_geom(a, Ct, &g);
  int64_t most = 0;  // elements of the largest source gradient
  for (int k = 0; k < a->nsrc; ++k) {
    g.gsrc[k] = g_src[k];
    g.src[k] = nullptr;
    const int64_t n = (int64_t)a->B * a->C[k] * a->D * a->H * a->W;
    most = n > most ? n : most;
  }
  const int64_t in_elems = (int64_t)a->B * Ct * a->D * a->H * a->W;
  const dim3 block(VOL_THREADS);
  hipStream_t s = (hipStream_t)stream;
  if (a->scale == 1) {
    g.total = (uint32_t)in_elems;
    hipLaunchKernelGGL(vol_bwd_copy_kernel, dim3(vol_blocks((most + 3) / 4), (unsigned)a->nsrc), block, 0, s, g, g_out);
  } else {
    float* ws = reinterpret_cast<float*>(workspace);
    const int64_t ws_elems = (int64_t)a->B * Ct * g.Do * a->H * a->W;
    g.total = (uint32_t)ws_elems;
    hipLaunchKernelGGL(vol_bwd_xy_kernel, dim3(vol_blocks(ws_elems)), block, 0, s, g, g_out, ws);
    g.total = (uint32_t)in_elems;
    hipLaunchKernelGGL(vol_bwd_z_kernel, dim3(vol_blocks(most), (unsigned)a->nsrc), block, 0, s, g, (const float*)ws);
  }
  return launch_done(fn);
}

}  // extern "C"
