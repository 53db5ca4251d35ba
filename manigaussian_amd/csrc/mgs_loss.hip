// mgs_loss.hip -- ManiGaussian's rendering losses for V views in one pass, forward and backward.
// Reference: agents/manigaussian_bc/neural_rendering.py:299-329 (the loss block), :90-106 (_embed_loss_fn), :22-27
// (PSNR_torch) and loss.py:12-23 (l2_loss, cosine_loss).  The reference runs a few dozen small torch kernels there, between
// the rasterizer's forward and its backward, and PSNR_torch's `if mse == 0` reads the device in every step.  Here:
//   render_loss_minmax_kernel    ("l2_norm" only) per-view min / max of the target embedding, as workgroup partials
//   render_loss_fwd_kernel       one streaming pass over the images: writes the WEIGHTED UNIT GRADIENTS d loss / d image and
//                                one row of partial sums per workgroup
//   render_loss_finalize_kernel  one workgroup: the partials of every view in a fixed order -> mse, embed, psnr, loss
//   render_loss_bwd_kernel       out = g_up * unit over both gradient buffers, g_up read on the device
// Stream order is the only synchronisation between them: no float atomics, no hand-off between workgroups, no host read.
// Everything is bit-identical from run to run, and the launches can be captured into a HIP graph as they are.
#include "mgs_common.h"
#include "mgs_device.h"

namespace mgs {

constexpr int LOSS_WG = 256;                 // 4 x wave64
constexpr int LOSS_PX = 4;                   // consecutive pixels per thread (one 16-byte access per plane)
constexpr int LOSS_SPAN = LOSS_WG * LOSS_PX; // pixels per workgroup
constexpr int LOSS_MM = 64;                  // min/max partials per view (one per lane of the wave that folds them)
constexpr float COS_EPS = 1e-8f;             // F.cosine_similarity's eps
constexpr float NORM_DENOM = 1e-12f;         // MIN_DENOMINATOR of the "l2_norm" label normalisation

// How a thread reads its 4 pixels of a target: one element at a time; one float4 of 4 pixels of a channel plane (channel-first,
// needs the images' 16-byte path); 12 consecutive floats of 4 channel-last RGB pixels (ditto); one float4 of 4 CHANNELS per pixel
// (channel-last with C % 4 == 0: a lane's 16 bytes instead of four 4-byte gathers a cache line apart).
enum { TGT_STRIDED = 0, TGT_PLANAR4 = 1, TGT_RGB_PACKED = 2, TGT_PIXEL4 = 3 };

// A target image [V, C, H, W] addressed by element strides (channel-last and channel-first tensors without a copy).
struct LossTarget {
  const float* p;
  int sv, sc, sh, sw;
  int mode;  // TGT_*
};

struct LossArgs {
  int V, F, W, H, N, B;  // N = H * W pixels, B = workgroups per view
  int embed_fn;          // MGS_EMBED_*; -1: no embed term
  int vec;               // 1: W % 4 == 0 and every image base is 16-byte aligned: float4 accesses
  const float *color, *feature;
  LossTarget rgb, emb;
  const float* w_dev;    // [V,2] weights in device memory, or nullptr: w[] below
  float w[2 * MAX_VIEWS];
  float *g_color, *g_feature;  // weighted unit gradients (either may be nullptr: not wanted)
  float* partials;             // [V][B][2]: sum (x - t)^2, embed sum
  const float* mm;             // [V][LOSS_MM][2] min / max partials of the target embedding (l2_norm)
};

__device__ __forceinline__ void ld_img(const float* __restrict__ plane, int p, int N, bool vec, float (&o)[LOSS_PX]) {
  if (vec) {
    const float4 q = *reinterpret_cast<const float4*>(plane + p);
    o[0] = q.x; o[1] = q.y; o[2] = q.z; o[3] = q.w;
  } else {
#pragma unroll
    for (int j = 0; j < LOSS_PX; j++) o[j] = (p + j < N) ? plane[p + j] : 0.f;
  }
}

__device__ __forceinline__ void st_img(float* __restrict__ plane, int p, int N, bool vec, const float (&o)[LOSS_PX]) {
  if (vec) {
    *reinterpret_cast<float4*>(plane + p) = make_float4(o[0], o[1], o[2], o[3]);
  } else {
#pragma unroll
    for (int j = 0; j < LOSS_PX; j++)
      if (p + j < N) plane[p + j] = o[j];
  }
}

// Element offsets of a thread's 4 pixels inside one channel plane of a target (-1: the pixel is past the image).
__device__ __forceinline__ void tgt_offsets(const LossTarget& t, int p, int W, int N, int (&off)[LOSS_PX]) {
#pragma unroll
  for (int j = 0; j < LOSS_PX; j++) {
    const int pj = p + j, y = pj / W, x = pj - y * W;
    off[j] = pj < N ? y * t.sh + x * t.sw : -1;
  }
}

__device__ __forceinline__ void ld_tgt(const LossTarget& t, const float* __restrict__ base, const int (&off)[LOSS_PX],
                                       bool vec, float (&o)[LOSS_PX]) {
  if (vec && t.mode == TGT_PLANAR4) {
    const float4 q = *reinterpret_cast<const float4*>(base + off[0]);
    o[0] = q.x; o[1] = q.y; o[2] = q.z; o[3] = q.w;
  } else {
#pragma unroll
    for (int j = 0; j < LOSS_PX; j++) o[j] = off[j] >= 0 ? base[off[j]] : 0.f;
  }
}

// K consecutive channels (starting at `base`'s) of the thread's 4 pixels: o[k][j] = channel k of pixel j.
template <int K>
__device__ __forceinline__ void ld_tgt_k(const LossTarget& t, const float* __restrict__ base, const int (&off)[LOSS_PX],
                                         bool vec, float (&o)[K][LOSS_PX]) {
  if (K == 4 && t.mode == TGT_PIXEL4) {
#pragma unroll
    for (int j = 0; j < LOSS_PX; j++) {
      const float4 q = off[j] >= 0 ? *reinterpret_cast<const float4*>(base + off[j]) : make_float4(0.f, 0.f, 0.f, 0.f);
      o[0][j] = q.x; o[1 % K][j] = q.y; o[2 % K][j] = q.z; o[3 % K][j] = q.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < K; k++) ld_tgt(t, base + k * t.sc, off, vec, o[k]);
  }
}

// The three channel passes of the embed term, K channels at a time (K = 4, then the K = 1 tail).
template <int K>
__device__ __forceinline__ void cos_accum(const LossTarget& t, const float* __restrict__ e_c, const float* __restrict__ t_c, int p,
                                          int N, const int (&off)[LOSS_PX], bool vec, float (&dot)[LOSS_PX],
                                          float (&nn)[LOSS_PX], float (&mm)[LOSS_PX]) {
  float e[K][LOSS_PX], g[K][LOSS_PX];
#pragma unroll
  for (int k = 0; k < K; k++) ld_img(e_c + (size_t)k * N, p, N, vec, e[k]);
  ld_tgt_k<K>(t, t_c, off, vec, g);
#pragma unroll
  for (int k = 0; k < K; k++) {
#pragma unroll
    for (int j = 0; j < LOSS_PX; j++) {
      dot[j] += e[k][j] * g[k][j];
      nn[j] += e[k][j] * e[k][j];
      mm[j] += g[k][j] * g[k][j];
    }
  }
}

template <int K>
__device__ __forceinline__ void cos_grad(const LossTarget& t, const float* __restrict__ e_c, const float* __restrict__ t_c,
                                         float* __restrict__ g_c, int p, int N, const int (&off)[LOSS_PX], bool vec,
                                         const float (&ka)[LOSS_PX], const float (&kb)[LOSS_PX]) {
  float e[K][LOSS_PX], g[K][LOSS_PX];
#pragma unroll
  for (int k = 0; k < K; k++) ld_img(e_c + (size_t)k * N, p, N, vec, e[k]);
  ld_tgt_k<K>(t, t_c, off, vec, g);
#pragma unroll
  for (int k = 0; k < K; k++) {
    float o[LOSS_PX];
#pragma unroll
    for (int j = 0; j < LOSS_PX; j++) o[j] = ka[j] * g[k][j] + kb[j] * e[k][j];
    st_img(g_c + (size_t)k * N, p, N, vec, o);
  }
}

template <int K>
__device__ __forceinline__ float l2_pass(const LossTarget& t, const float* __restrict__ e_c, const float* __restrict__ t_c,
                                         float* __restrict__ g_c, int p, int N, const int (&off)[LOSS_PX], bool vec, bool norm,
                                         float lo, float den, float scale) {
  float e[K][LOSS_PX], g[K][LOSS_PX];
#pragma unroll
  for (int k = 0; k < K; k++) ld_img(e_c + (size_t)k * N, p, N, vec, e[k]);
  ld_tgt_k<K>(t, t_c, off, vec, g);
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < K; k++) {
    float o[LOSS_PX];
#pragma unroll
    for (int j = 0; j < LOSS_PX; j++) {
      const float tt = norm ? (g[k][j] - lo) / den : g[k][j];
      const float d = off[j] >= 0 ? e[k][j] - tt : 0.f;
      s += d * d;
      o[j] = scale * d;
    }
    if (g_c) st_img(g_c + (size_t)k * N, p, N, vec, o);
  }
  return s;
}

// torch's min() and max() are NaN for a tensor that holds one; fminf and fmaxf drop it
__device__ __forceinline__ float loss_min(float a, float b) { return __builtin_isunordered(a, b) ? __builtin_nanf("") : fminf(a, b); }
__device__ __forceinline__ float loss_max(float a, float b) { return __builtin_isunordered(a, b) ? __builtin_nanf("") : fmaxf(a, b); }

__global__ void __launch_bounds__(LOSS_WG) render_loss_minmax_kernel(LossTarget t, int F, int W, int N, float* mm) {
  const int v = blockIdx.y;
  const float* base = t.p + (size_t)v * t.sv;
  float lo = INFINITY, hi = -INFINITY;
  for (int p = blockIdx.x * LOSS_WG + threadIdx.x; p < N; p += LOSS_MM * LOSS_WG) {
    const int y = p / W, x = p - y * W;
    const float* px = base + y * t.sh + x * t.sw;
    for (int c = 0; c < F; c++) {
      const float g = px[c * t.sc];
      lo = loss_min(lo, g);
      hi = loss_max(hi, g);
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    lo = loss_min(lo, __shfl_xor(lo, d, 64));
    hi = loss_max(hi, __shfl_xor(hi, d, 64));
  }
  __shared__ float s[LOSS_WG / WAVE][2];
  const int wave = threadIdx.x / WAVE;
  if ((threadIdx.x & (WAVE - 1)) == 0) { s[wave][0] = lo; s[wave][1] = hi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float* o = mm + 2 * ((size_t)v * LOSS_MM + blockIdx.x);
    o[0] = loss_min(loss_min(s[0][0], s[1][0]), loss_min(s[2][0], s[3][0]));
    o[1] = loss_max(loss_max(s[0][1], s[1][1]), loss_max(s[2][1], s[3][1]));
  }
}

__global__ void __launch_bounds__(LOSS_WG) render_loss_fwd_kernel(LossArgs a) {
  const int v = blockIdx.y;
  const int p = (blockIdx.x * LOSS_WG + threadIdx.x) * LOSS_PX;
  const int N = a.N;
  const bool vec = a.vec != 0;
  const bool live = p < N;  // (a thread past the image still takes part in the reductions)
  const float w_rgb = a.w_dev ? a.w_dev[2 * v] : a.w[2 * v];
  const float w_emb = a.w_dev ? a.w_dev[2 * v + 1] : a.w[2 * v + 1];
  float s_rgb = 0.f, s_emb = 0.f;

  __shared__ float s_mm[2];
  if (a.embed_fn == MGS_EMBED_L2_NORM) {  // fold the view's min / max partials (one per lane of wave 0)
    if (threadIdx.x < WAVE) {
      float lo = a.mm[2 * ((size_t)v * LOSS_MM + threadIdx.x)], hi = a.mm[2 * ((size_t)v * LOSS_MM + threadIdx.x) + 1];
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) {
        lo = loss_min(lo, __shfl_xor(lo, d, 64));
        hi = loss_max(hi, __shfl_xor(hi, d, 64));
      }
      if (threadIdx.x == 0) { s_mm[0] = lo; s_mm[1] = hi; }
    }
    __syncthreads();
  }

  if (live) {
    // ---- l2(rgb): sum (x - t)^2, gradient 2 (x - t) / (3 N) ----
    {
      const float k = w_rgb * (2.0f / (3.0f * (float)N));
      const float* tb = a.rgb.p + (size_t)v * a.rgb.sv;
      int off[LOSS_PX];
      tgt_offsets(a.rgb, p, a.W, N, off);
      const bool packed = vec && a.rgb.mode == TGT_RGB_PACKED;
      float4 q0, q1, q2;
      if (packed) {  // 4 channel-last pixels = 12 consecutive floats
        const float4* q = reinterpret_cast<const float4*>(tb + off[0]);
        q0 = q[0]; q1 = q[1]; q2 = q[2];
      }
#pragma unroll
      for (int c = 0; c < 3; c++) {
        float x[LOSS_PX], t[LOSS_PX], g[LOSS_PX];
        ld_img(a.color + ((size_t)v * 3 + c) * N, p, N, vec, x);
        if (packed) {
          const float f[12] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};
#pragma unroll
          for (int j = 0; j < LOSS_PX; j++) t[j] = f[3 * j + c];
        } else {
          ld_tgt(a.rgb, tb + c * a.rgb.sc, off, vec, t);
        }
#pragma unroll
        for (int j = 0; j < LOSS_PX; j++) {
          const float d = x[j] - t[j];
          s_rgb += d * d;
          g[j] = k * d;
        }
        if (a.g_color) st_img(a.g_color + ((size_t)v * 3 + c) * N, p, N, vec, g);
      }
    }
    // ---- the embed term ----
    if (a.embed_fn >= 0) {
      const int F = a.F;
      const float* eb = a.feature + (size_t)v * F * N;
      float* gb = a.g_feature ? a.g_feature + (size_t)v * F * N : nullptr;
      const float* tb = a.emb.p + (size_t)v * a.emb.sv;
      int off[LOSS_PX];
      tgt_offsets(a.emb, p, a.W, N, off);
      if (a.embed_fn == MGS_EMBED_COSINE) {
        float dot[LOSS_PX] = {0.f, 0.f, 0.f, 0.f}, nn[LOSS_PX] = {0.f, 0.f, 0.f, 0.f}, mm[LOSS_PX] = {0.f, 0.f, 0.f, 0.f};
        int c = 0;
        for (; c + 4 <= F; c += 4) cos_accum<4>(a.emb, eb + (size_t)c * N, tb + c * a.emb.sc, p, N, off, vec, dot, nn, mm);
        for (; c < F; c++) cos_accum<1>(a.emb, eb + (size_t)c * N, tb + c * a.emb.sc, p, N, off, vec, dot, nn, mm);
        // c = e.g / (n_c m_c) with n_c = max(|e|, eps), m_c = max(|g|, eps) (ATen clamps the norms outside the graph);
        // d c / d e = g / (n_c m_c) - c e / (n_c n) for n > 0, g / (n_c m_c) for n = 0.  loss term = 1 - mean c.
        const float kn = -w_emb / (float)N;
        float ka[LOSS_PX], kb[LOSS_PX];
#pragma unroll
        for (int j = 0; j < LOSS_PX; j++) {
          const float n = sqrtf(nn[j]), m = sqrtf(mm[j]);
          // clamp_min as comparisons: a NaN norm stays NaN, as in ATen (fmaxf would make it eps)
          const float n_c = n < COS_EPS ? COS_EPS : n, m_c = m < COS_EPS ? COS_EPS : m;
          const float cs = dot[j] / (n_c * m_c);
          s_emb += cs;  // (a pixel past the image: e = g = 0, cs = 0)
          ka[j] = kn / (n_c * m_c);
          kb[j] = !(n <= 0.f) ? -kn * cs / (n_c * n) : 0.f;   // (a NaN norm takes the general branch)
        }
        if (gb) {  // second pass over the channels (L2 hits) instead of 2 x 4 x F values in registers
          for (c = 0; c + 4 <= F; c += 4)
            cos_grad<4>(a.emb, eb + (size_t)c * N, tb + c * a.emb.sc, gb + (size_t)c * N, p, N, off, vec, ka, kb);
          for (; c < F; c++) cos_grad<1>(a.emb, eb + (size_t)c * N, tb + c * a.emb.sc, gb + (size_t)c * N, p, N, off, vec, ka, kb);
        }
      } else {
        // l2 / l2_norm: sum (e - g')^2 / (F N), g' = (g - min g) / (max g - min g + 1e-12) for l2_norm
        const bool norm = a.embed_fn == MGS_EMBED_L2_NORM;
        const float lo = norm ? s_mm[0] : 0.f;
        const float den = norm ? (s_mm[1] - s_mm[0]) + NORM_DENOM : 1.f;
        const float k = w_emb * (2.0f / ((float)F * (float)N));
        int c = 0;
        for (; c + 4 <= F; c += 4)
          s_emb += l2_pass<4>(a.emb, eb + (size_t)c * N, tb + c * a.emb.sc, gb ? gb + (size_t)c * N : nullptr, p, N, off, vec,
                              norm, lo, den, k);
        for (; c < F; c++)
          s_emb += l2_pass<1>(a.emb, eb + (size_t)c * N, tb + c * a.emb.sc, gb ? gb + (size_t)c * N : nullptr, p, N, off, vec,
                              norm, lo, den, k);
      }
    }
  }
  // ---- workgroup reduction: wave butterflies, four waves through LDS, one plain store ----
  s_rgb = wave_sum_shfl(s_rgb);
  s_emb = wave_sum_shfl(s_emb);
  __shared__ float s_part[LOSS_WG / WAVE][2];
  const int wave = threadIdx.x / WAVE;
  if ((threadIdx.x & (WAVE - 1)) == 0) { s_part[wave][0] = s_rgb; s_part[wave][1] = s_emb; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float* o = a.partials + 2 * ((size_t)v * a.B + blockIdx.x);
    o[0] = (s_part[0][0] + s_part[1][0]) + (s_part[2][0] + s_part[3][0]);
    o[1] = (s_part[0][1] + s_part[1][1]) + (s_part[2][1] + s_part[3][1]);
  }
}

struct LossFinalArgs {
  int V, F, N, B, embed_fn;
  const float* partials;
  const float* w_dev;
  float w[2 * MAX_VIEWS];
  float* terms;  // [V][3]: mse, embed, psnr
  float* loss;
};

// One workgroup.  Wave w folds views w, w + 4, ...: lane l adds partials l, l + 64, ... in index order, then the butterfly.
__global__ void __launch_bounds__(LOSS_WG) render_loss_finalize_kernel(LossFinalArgs a) {
  const int wave = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
  __shared__ float s_term[MAX_VIEWS][2];
  for (int v = wave; v < a.V; v += LOSS_WG / WAVE) {
    float r = 0.f, e = 0.f;
    for (int b = lane; b < a.B; b += WAVE) {
      const float* q = a.partials + 2 * ((size_t)v * a.B + b);
      r += q[0];
      e += q[1];
    }
    r = wave_sum_shfl(r);
    e = wave_sum_shfl(e);
    if (lane == 0) {
      const float N = (float)a.N;
      const float mse = r / (3.0f * N);
      float emb = 0.f;
      if (a.embed_fn == MGS_EMBED_COSINE) emb = 1.0f - e / N;
      else if (a.embed_fn >= 0) emb = e / ((float)a.F * N);
      const float psnr = mse == 0.f ? 100.0f : 20.0f * log10f(1.0f / sqrtf(mse));  // PSNR_torch, without the host read
      a.terms[3 * v] = mse;
      a.terms[3 * v + 1] = emb;
      a.terms[3 * v + 2] = psnr;
      s_term[v][0] = mse;
      s_term[v][1] = emb;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float loss = 0.f;  // loss = 0. ; loss += w_rgb * l_rgb ; loss += w_embed * l_embed -- view by view
    for (int v = 0; v < a.V; v++) {
      const float w_rgb = a.w_dev ? a.w_dev[2 * v] : a.w[2 * v];
      const float w_emb = a.w_dev ? a.w_dev[2 * v + 1] : a.w[2 * v + 1];
      loss += w_rgb * s_term[v][0];
      if (a.embed_fn >= 0) loss += w_emb * s_term[v][1];
    }
    *a.loss = loss;
  }
}

// out = g_up * unit over both buffers.  n4: float4 units of each buffer; the scalar tails follow.
__global__ void __launch_bounds__(LOSS_WG) render_loss_bwd_kernel(const float* __restrict__ g_up,
                                                                  const float* __restrict__ unit_c, float* __restrict__ out_c,
                                                                  size_t n_c, const float* __restrict__ unit_f,
                                                                  float* __restrict__ out_f, size_t n_f, int vec) {
  const float g = *g_up;
  const size_t i = (size_t)blockIdx.x * LOSS_WG + threadIdx.x;
  const size_t qc = (n_c + 3) / 4, qf = (n_f + 3) / 4;
  const float* u;
  float* o;
  size_t n, q;
  if (i < qc) { u = unit_c; o = out_c; n = n_c; q = i; }
  else if (i < qc + qf) { u = unit_f; o = out_f; n = n_f; q = i - qc; }
  else return;
  const size_t e = 4 * q;
  if (vec && e + 4 <= n) {
    const float4 x = *reinterpret_cast<const float4*>(u + e);
    *reinterpret_cast<float4*>(o + e) = make_float4(g * x.x, g * x.y, g * x.z, g * x.w);
  } else {
    for (size_t j = e; j < n && j < e + 4; j++) o[j] = g * u[j];
  }
}

// Validates a target's strides ([V,C,H,W] in elements) and picks how the 16-byte path reads it.
static int fill_target(LossTarget& t, const float* p, const int64_t* st, int V, int C, int W, int H, bool vec, const char* what) {
  if (!p || !st) { set_error("render_loss_fwd: %s is NULL", what); return MGS_ERR_INVALID_ARG; }
  int64_t last = 0;
  const int64_t dims[4] = {V, C, H, W};
  for (int i = 0; i < 4; i++) {
    if (st[i] < 0) { set_error("render_loss_fwd: %s has a negative stride", what); return MGS_ERR_INVALID_ARG; }
    last += (dims[i] - 1) * st[i];
  }
  if (last >= ((int64_t)1 << 31)) { set_error("render_loss_fwd: %s spans 2^31 elements or more", what); return MGS_ERR_INVALID_ARG; }
  t.p = p;
  t.sv = (int)st[0]; t.sc = (int)st[1]; t.sh = (int)st[2]; t.sw = (int)st[3];
  t.mode = TGT_STRIDED;
  const bool rows16 = !misaligned16(p) && (V == 1 || st[0] % 4 == 0) && (H == 1 || st[2] % 4 == 0);
  if (vec && rows16) {
    if (st[3] == 1 && (C == 1 || st[1] % 4 == 0)) t.mode = TGT_PLANAR4;
    else if (C == 3 && st[3] == 3 && st[1] == 1) t.mode = TGT_RGB_PACKED;
  }
  if (t.mode == TGT_STRIDED && rows16 && C % 4 == 0 && st[1] == 1 && (W == 1 || st[3] % 4 == 0)) t.mode = TGT_PIXEL4;
  return MGS_OK;
}

static int loss_shape_ok(const char* fn, int V, int F, int W, int H) {
  if (V < 1 || V > MAX_VIEWS) { set_error("%s: V = %d views (1 .. %d)", fn, V, MAX_VIEWS); return MGS_ERR_INVALID_ARG; }
  if (F < 0 || F > MGS_MAX_FEATURE_CHANNELS) {
    set_error("%s: F = %d feature channels (at most %d)", fn, F, MGS_MAX_FEATURE_CHANNELS);
    return MGS_ERR_INVALID_ARG;
  }
  if (W < 1 || H < 1 || (int64_t)W * H * (int64_t)(F > 3 ? F : 3) * V >= ((int64_t)1 << 31)) {
    set_error("%s: image %d x %d (V = %d, F = %d) is empty or too large", fn, W, H, V, F);
    return MGS_ERR_INVALID_ARG;
  }
  return MGS_OK;
}

static size_t loss_partials_floats(int V, int W, int H) {
  const size_t B = ((size_t)W * H + LOSS_SPAN - 1) / LOSS_SPAN;
  return 2 * (size_t)V * B;
}

}  // namespace mgs

using namespace mgs;

extern "C" {

size_t mgs_render_loss_workspace_bytes(int V, int W, int H) {
  if (V < 1 || W < 1 || H < 1) return 0;
  return align_up(loss_partials_floats(V, W, H) * sizeof(float)) + align_up(2 * (size_t)V * LOSS_MM * sizeof(float));
}

int mgs_render_loss_forward(int V, int F, int W, int H, const float* color, const float* gt_rgb, const int64_t* rgb_strides,
                            const float* feature, const float* gt_embed, const int64_t* embed_strides, int embed_fn,
                            const float* weights_host, const float* weights_dev, float* g_color, float* g_feature,
                            float* terms, float* loss, void* workspace, size_t workspace_bytes, mgs_stream_t stream) {
  const char* fn = "render_loss_fwd";
  if (int rc = loss_shape_ok(fn, V, F, W, H)) return rc;
  if (!color || !terms || !loss || !workspace) { set_error("%s: NULL pointer", fn); return MGS_ERR_INVALID_ARG; }
  if (weights_host && weights_dev) { set_error("%s: weights given by value and as a device pointer", fn); return MGS_ERR_INVALID_ARG; }
  const bool has_embed = feature != nullptr && gt_embed != nullptr && F > 0;
  if ((feature != nullptr) != (gt_embed != nullptr) && F > 0) {
    set_error("%s: feature and gt_embed must be given together", fn);
    return MGS_ERR_INVALID_ARG;
  }
  if (has_embed && (embed_fn < MGS_EMBED_COSINE || embed_fn > MGS_EMBED_L2_NORM)) {
    set_error("%s: unknown embed_fn %d", fn, embed_fn);
    return MGS_ERR_INVALID_ARG;
  }
  if (int rc = workspace_short(fn, workspace_bytes, mgs_render_loss_workspace_bytes(V, W, H))) return rc;
  LossArgs a = {};
  a.V = V; a.F = has_embed ? F : 0; a.W = W; a.H = H; a.N = W * H;
  a.B = (a.N + LOSS_SPAN - 1) / LOSS_SPAN;
  a.embed_fn = has_embed ? embed_fn : -1;
  a.vec = (W % 4 == 0) && !misaligned16(color) && (!g_color || !misaligned16(g_color)) &&
          (!has_embed || (!misaligned16(feature) && (!g_feature || !misaligned16(g_feature))));
  a.color = color; a.feature = has_embed ? feature : nullptr;
  if (int rc = fill_target(a.rgb, gt_rgb, rgb_strides, V, 3, W, H, a.vec, "gt_rgb")) return rc;
  if (has_embed) {
    if (int rc = fill_target(a.emb, gt_embed, embed_strides, V, F, W, H, a.vec, "gt_embed")) return rc;
  }
  a.w_dev = weights_dev;
  for (int i = 0; i < 2 * V; i++) a.w[i] = weights_host ? weights_host[i] : 1.0f;
  a.g_color = g_color; a.g_feature = has_embed ? g_feature : nullptr;
  a.partials = reinterpret_cast<float*>(workspace);
  float* mm = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + align_up(loss_partials_floats(V, W, H) * sizeof(float)));
  a.mm = mm;
  hipStream_t s = (hipStream_t)stream;
  if (a.embed_fn == MGS_EMBED_L2_NORM)
    hipLaunchKernelGGL(render_loss_minmax_kernel, dim3(LOSS_MM, V), dim3(LOSS_WG), 0, s, a.emb, F, W, a.N, mm);
  hipLaunchKernelGGL(render_loss_fwd_kernel, dim3(a.B, V), dim3(LOSS_WG), 0, s, a);
  LossFinalArgs f = {};
  f.V = V; f.F = a.F; f.N = a.N; f.B = a.B; f.embed_fn = a.embed_fn;
  f.partials = a.partials; f.w_dev = weights_dev;
  for (int i = 0; i < 2 * V; i++) f.w[i] = a.w[i];
  f.terms = terms; f.loss = loss;
  hipLaunchKernelGGL(render_loss_finalize_kernel, dim3(1), dim3(LOSS_WG), 0, s, f);
  return launch_done(fn);
}

int mgs_render_loss_backward(int V, int F, int W, int H, const float* g_up, const float* unit_color, const float* unit_feature,
                             float* out_color, float* out_feature, mgs_stream_t stream) {
  const char* fn = "render_loss_bwd";
  if (int rc = loss_shape_ok(fn, V, F, W, H)) return rc;
  if (!g_up) { set_error("%s: g_up is NULL", fn); return MGS_ERR_INVALID_ARG; }
  if ((out_color && !unit_color) || (out_feature && !unit_feature)) {
    set_error("%s: an output without its unit gradient", fn);
    return MGS_ERR_INVALID_ARG;
  }
  const size_t N = (size_t)W * H;
  const size_t n_c = out_color ? (size_t)V * 3 * N : 0, n_f = (out_feature && F > 0) ? (size_t)V * F * N : 0;
  const size_t quads = (n_c + 3) / 4 + (n_f + 3) / 4;
  if (quads == 0) return MGS_OK;
  const int vec = (!n_c || (!misaligned16(unit_color) && !misaligned16(out_color))) && (!n_f || (!misaligned16(unit_feature) && !misaligned16(out_feature)));
  hipLaunchKernelGGL(render_loss_bwd_kernel, dim3((unsigned)((quads + LOSS_WG - 1) / LOSS_WG)), dim3(LOSS_WG), 0,
                     (hipStream_t)stream, g_up, unit_color, out_color, n_c, unit_feature, out_feature, n_f, vec);
  return launch_done(fn);
}

}  // extern "C"
