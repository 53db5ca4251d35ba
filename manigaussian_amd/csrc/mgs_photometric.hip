// mgs_photometric.hip -- the photometric loss of Gaussian splatting for V views in one pass: L1 + L2 + D-SSIM, forward and backward.
// Reference: agents/manigaussian_bc/loss.py:9-13 (l1_loss, l2_loss), :25-68 (gaussian, create_window, ssim, _ssim: an 11 x 11
// Gaussian window of sigma 1.5, zero padding of 5), conf/method/ManiGaussian_BC.yaml:97-98 (lambda_l1, lambda_ssim).  In torch
// that is five grouped conv2d calls forward and their backward plus a dozen elementwise kernels.  Here:
//   photometric_fwd_kernel       one workgroup per 32 x 32 tile of one (view, channel) plane: stages the tile and a halo of x and
//                                y in LDS once, row-filters x, y, x^2, y^2, xy into LDS, column-filters them from there, evaluates
//                                the SSIM map and writes one row of partial sums (|x - y|, (x - y)^2, map) per workgroup and --
//                                when a gradient is wanted -- the three maps d m / d mu_x, d m / d sigma_x^2, d m / d sigma_xy
//   photometric_grad_kernel      the same separable LDS convolution over those three maps:
//                                d ssim / d x(p) = (G*a)(p) + 2 x(p) (G*b)(p) + y(p) (G*c)(p); writes the WEIGHTED UNIT GRADIENT
//                                d loss / d color of the l1 + l2 + ssim terms
//   photometric_finalize_kernel  one workgroup: the partials of every view in a fixed order -> l1, l2, ssim, psnr, loss
//   photometric_bwd_kernel       out[v] = g_up[v * stride] * unit[v], g_up read on the device
// Stream order is the only synchronisation between them: no float atomics, no hand-off between workgroups, no host read.
// Everything is bit-identical from run to run, and the launches can be captured into a HIP graph as they are.
//
// LDS layout.  A staged plane holds PH_ROWS = 42 rows (the tile's 32 + 5 above + 5 below) of PH_SW = 48 columns:
// the tile's 32 + 8 to the left + 8 to the right, so that its first column is 16-byte aligned in the image and a row is twelve
// float4 loads; the window needs columns 3 .. 44 of them.  The row pass gives a thread 4 consecutive outputs of one row (14
// staged values -> 4 x 11 taps), so the lanes of a 32-lane group touch 4 rows x 8 column groups: with a row stride of 49
// (odd) and 4-float groups, (row * 49 + 4 * group) mod 32 is distinct for all of them -- no bank conflict; the same holds for
// the row-filtered planes' stride of 33 on the write side.  The column pass gives a thread 4 consecutive rows of one column (14
// row-filtered values -> 4 x 11 taps) with the lanes on consecutive columns: conflict-free at any stride.
#include "mgs_common.h"
#include "mgs_device.h"

namespace mgs {

constexpr int PH_WG = 256;                      // 4 x wave64
constexpr int PH_T = 32;                        // outputs per tile, both directions
constexpr int PH_K = MGS_SSIM_WINDOW_SIZE;      // taps
constexpr int PH_R = PH_K / 2;                  // halo
constexpr int PH_ROWS = PH_T + 2 * PH_R;        // 42 staged rows
constexpr int PH_LEAD = 8;                      // staged columns left of the tile (>= PH_R, a multiple of 4)
constexpr int PH_SW = PH_T + 2 * PH_LEAD;       // 48 staged columns
constexpr int PH_SS = PH_SW + 1;                // 49: staged row stride (odd)
constexpr int PH_RS = PH_T + 1;                 // 33: row stride of the row-filtered planes and of the output tile (odd)
constexpr int PH_SPAN = 4 + PH_K - 1;           // 14 inputs of 4 consecutive outputs
constexpr float SSIM_C1 = 0.01f * 0.01f;
constexpr float SSIM_C2 = 0.03f * 0.03f;
static_assert(PH_K == 11 && PH_LEAD >= PH_R && PH_LEAD % 4 == 0 && PH_WG == 8 * PH_T, "tile geometry");

__constant__ float PH_G[PH_K] = MGS_SSIM_WINDOW;

// One [H][W] plane addressed by element strides; vec: rows can be read as float4 (column stride 1, everything 16-byte aligned)
struct PhPlane {
  const float* p;
  long long sh, sw;
  int vec;
};

struct PhTarget {
  const float* p;
  long long sv, sc, sh, sw;
  int vec;
};

struct PhArgs {
  int V, C, W, H, tiles_x, tiles_y;
  int vec;                    // W % 4 == 0 and color, unit_grad and the maps are 16-byte aligned
  const float* color;
  PhTarget tgt;
  const float* w_dev;         // [V,3] weights in device memory, or nullptr: w[] below
  float w[3 * MAX_VIEWS];
  float* maps;                // [3][V*C][H][W]: a, b, c (nullptr: not wanted)
  float* partials;            // [V*C*tiles][3]
  float* unit;                // [V,C,H,W]
};

// Stages rows y0 - 5 .. y0 + 36, columns x0 - 8 .. x0 + 39 of a plane into s[PH_ROWS][PH_SS]; zero outside the image.
__device__ __forceinline__ void ph_stage(float* __restrict__ s, const PhPlane& pl, int x0, int y0, int W, int H) {
  if (pl.vec) {
    for (int i = threadIdx.x; i < PH_ROWS * (PH_SW / 4); i += PH_WG) {
      const int r = i / (PH_SW / 4), q = i - r * (PH_SW / 4);
      const int y = y0 - PH_R + r, x = x0 - PH_LEAD + 4 * q;  // (W % 4 == 0: a quad is inside the row or outside)
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (y >= 0 && y < H && x >= 0 && x < W) v = *reinterpret_cast<const float4*>(pl.p + (long long)y * pl.sh + x);
      float* d = s + r * PH_SS + 4 * q;
      d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
  } else {
    for (int i = threadIdx.x; i < PH_ROWS * PH_SW; i += PH_WG) {
      const int r = i / PH_SW, j = i - r * PH_SW;
      const int y = y0 - PH_R + r, x = x0 - PH_LEAD + j;
      float v = 0.f;
      if (y >= 0 && y < H && x >= 0 && x < W) v = pl.p[(long long)y * pl.sh + (long long)x * pl.sw];
      s[r * PH_SS + j] = v;
    }
  }
}

// 4 consecutive outputs of the 11-tap filter from 14 consecutive inputs, taps in index order.
__device__ __forceinline__ void ph_taps(const float (&in)[PH_SPAN], const float (&g)[PH_K], float (&out)[4]) {
#pragma unroll
  for (int j = 0; j < 4; j++) {
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < PH_K; k++) acc = fmaf(g[k], in[j + k], acc);
    out[j] = acc;
  }
}

// The SSIM map at one pixel and its three partial derivatives.  Written so that identical images give m == 1 and a == 0,
// c == -2 b EXACTLY: no contraction, products rounded as the reference rounds them (mu1_sq, mu2_sq, mu1_mu2 are tensors there).
__device__ __forceinline__ float ph_map(float mx, float my, float exx, float eyy, float exy, float& a, float& b, float& c) {
#pragma clang fp contract(off)
  const float mxx = mx * mx, myy = my * my, mxy = mx * my;
  const float sx = exx - mxx, sy = eyy - myy, sxy = exy - mxy;
  const float A1 = 2.f * mxy + SSIM_C1, A2 = 2.f * sxy + SSIM_C2;
  const float B1 = (mxx + myy) + SSIM_C1, B2 = (sx + sy) + SSIM_C2;
  const float m = (A1 * A2) / (B1 * B2);
  const float t1 = A1 / B1, t2 = A2 / B2;
  // d m / d mu_x (sigmas held) = (2 / B1) (mu_y A2 / B2 - mu_x m); d m / d sigma_x^2 = -m / B2; d m / d sigma_xy = 2 A1 / (B1 B2)
  const float dmx = (2.f / B1) * (my * t2 - mx * m);
  b = -(m / B2);
  c = 2.f * (t1 / B2);
  // sigma_x^2 = G*x^2 - mu_x^2 and sigma_xy = G*xy - mu_x mu_y: their dependence on mu_x folded into a
  a = (dmx - (2.f * mx) * b) - my * c;
  return m;
}

__device__ __forceinline__ PhPlane ph_target_plane(const PhTarget& t, int v, int c) {
  PhPlane pl;
  pl.p = t.p + (long long)v * t.sv + (long long)c * t.sc;
  pl.sh = t.sh; pl.sw = t.sw; pl.vec = t.vec;
  return pl;
}

__global__ void __launch_bounds__(PH_WG) photometric_fwd_kernel(PhArgs a) {
  __shared__ float s_x[PH_ROWS * PH_SS], s_y[PH_ROWS * PH_SS];
  __shared__ float s_rf[5][PH_ROWS * PH_RS];  // row-filtered x, y, x^2, y^2, xy; afterwards the output tile of the three maps
  __shared__ float s_part[PH_WG / WAVE][3];
  const int tid = threadIdx.x;
  const int plane = blockIdx.z, v = plane / a.C, ch = plane - v * a.C;
  const int x0 = blockIdx.x * PH_T, y0 = blockIdx.y * PH_T;
  const int W = a.W, H = a.H;
  const size_t N = (size_t)W * H;
  float g[PH_K];
#pragma unroll
  for (int k = 0; k < PH_K; k++) g[k] = PH_G[k];

  PhPlane px;
  px.p = a.color + (size_t)plane * N; px.sh = W; px.sw = 1; px.vec = a.vec;
  ph_stage(s_x, px, x0, y0, W, H);
  ph_stage(s_y, ph_target_plane(a.tgt, v, ch), x0, y0, W, H);
  __syncthreads();

  // ---- rows: 42 rows x 8 groups of 4 outputs ----
  for (int i = tid; i < PH_ROWS * (PH_T / 4); i += PH_WG) {
    const int r = i >> 3, cg = i & 7;
    const float* qx = s_x + r * PH_SS + (PH_LEAD - PH_R) + 4 * cg;
    const float* qy = s_y + r * PH_SS + (PH_LEAD - PH_R) + 4 * cg;
    float in[5][PH_SPAN];
#pragma unroll
    for (int j = 0; j < PH_SPAN; j++) {
      const float X = qx[j], Y = qy[j];
      in[0][j] = X; in[1][j] = Y; in[2][j] = X * X; in[3][j] = Y * Y; in[4][j] = X * Y;
    }
#pragma unroll
    for (int q = 0; q < 5; q++) {
      float o[4];
      ph_taps(in[q], g, o);
      float* d = s_rf[q] + r * PH_RS + 4 * cg;
      d[0] = o[0]; d[1] = o[1]; d[2] = o[2]; d[3] = o[3];
    }
  }
  __syncthreads();

  // ---- columns: thread = column c, rows r0 .. r0 + 3 of the tile ----
  const int c = tid & (PH_T - 1), r0 = (tid >> 5) * 4;
  float f[5][4];
#pragma unroll
  for (int q = 0; q < 5; q++) {
    float in[PH_SPAN];
#pragma unroll
    for (int j = 0; j < PH_SPAN; j++) in[j] = s_rf[q][(r0 + j) * PH_RS + c];
    ph_taps(in, g, f[q]);
  }
  float s_l1 = 0.f, s_l2 = 0.f, s_m = 0.f;
  float ma[4], mb[4], mc[4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const bool in_img = x0 + c < W && y0 + r0 + j < H;
    const float X = s_x[(r0 + j + PH_R) * PH_SS + PH_LEAD + c], Y = s_y[(r0 + j + PH_R) * PH_SS + PH_LEAD + c];
    const float d = X - Y;
    const float m = ph_map(f[0][j], f[1][j], f[2][j], f[3][j], f[4][j], ma[j], mb[j], mc[j]);
    if (in_img) {
      s_l1 += fabsf(d);
      s_l2 = fmaf(d, d, s_l2);
      s_m += m;
    }
  }
  // ---- the three maps: through LDS (the row-filtered planes are dead) to 16-byte stores ----
  if (a.maps) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; j++) {
      s_rf[0][(r0 + j) * PH_RS + c] = ma[j];
      s_rf[1][(r0 + j) * PH_RS + c] = mb[j];
      s_rf[2][(r0 + j) * PH_RS + c] = mc[j];
    }
    __syncthreads();
    const int r = tid >> 3, cq = (tid & 7) * 4;
    const int y = y0 + r, x = x0 + cq;
    if (y < H && x < W) {
      const size_t VCN = (size_t)a.V * a.C * N;
#pragma unroll
      for (int q = 0; q < 3; q++) {
        const float* s = s_rf[q] + r * PH_RS + cq;
        float* o = a.maps + (size_t)q * VCN + (size_t)plane * N + (size_t)y * W + x;
        if (a.vec) {
          *reinterpret_cast<float4*>(o) = make_float4(s[0], s[1], s[2], s[3]);
        } else {
#pragma unroll
          for (int j = 0; j < 4; j++)
            if (x + j < W) o[j] = s[j];
        }
      }
    }
  }
  // ---- workgroup reduction: wave butterflies, four waves through LDS, one plain store ----
  s_l1 = wave_sum_shfl(s_l1);
  s_l2 = wave_sum_shfl(s_l2);
  s_m = wave_sum_shfl(s_m);
  const int wave = tid / WAVE;
  if ((tid & (WAVE - 1)) == 0) { s_part[wave][0] = s_l1; s_part[wave][1] = s_l2; s_part[wave][2] = s_m; }
  __syncthreads();
  if (tid < 3) {
    const size_t wg = ((size_t)plane * a.tiles_y + blockIdx.y) * a.tiles_x + blockIdx.x;
    a.partials[3 * wg + tid] = (s_part[0][tid] + s_part[1][tid]) + (s_part[2][tid] + s_part[3][tid]);
  }
}

__global__ void __launch_bounds__(PH_WG) photometric_grad_kernel(PhArgs a) {
  __shared__ float s_in[3][PH_ROWS * PH_SS];  // the staged maps; after the row pass the column-filtered output tile
  __shared__ float s_rf[3][PH_ROWS * PH_RS];
  const int tid = threadIdx.x;
  const int plane = blockIdx.z, v = plane / a.C, ch = plane - v * a.C;
  const int x0 = blockIdx.x * PH_T, y0 = blockIdx.y * PH_T;
  const int W = a.W, H = a.H;
  const size_t N = (size_t)W * H, VCN = (size_t)a.V * a.C * N;
  float g[PH_K];
#pragma unroll
  for (int k = 0; k < PH_K; k++) g[k] = PH_G[k];

#pragma unroll
  for (int q = 0; q < 3; q++) {
    PhPlane pm;
    pm.p = a.maps + (size_t)q * VCN + (size_t)plane * N; pm.sh = W; pm.sw = 1; pm.vec = a.vec;
    ph_stage(s_in[q], pm, x0, y0, W, H);
  }
  __syncthreads();
  for (int i = tid; i < PH_ROWS * (PH_T / 4); i += PH_WG) {
    const int r = i >> 3, cg = i & 7;
#pragma unroll
    for (int q = 0; q < 3; q++) {
      const float* s = s_in[q] + r * PH_SS + (PH_LEAD - PH_R) + 4 * cg;
      float in[PH_SPAN], o[4];
#pragma unroll
      for (int j = 0; j < PH_SPAN; j++) in[j] = s[j];
      ph_taps(in, g, o);
      float* d = s_rf[q] + r * PH_RS + 4 * cg;
      d[0] = o[0]; d[1] = o[1]; d[2] = o[2]; d[3] = o[3];
    }
  }
  __syncthreads();
  {
    const int c = tid & (PH_T - 1), r0 = (tid >> 5) * 4;
#pragma unroll
    for (int q = 0; q < 3; q++) {
      float in[PH_SPAN], o[4];
#pragma unroll
      for (int j = 0; j < PH_SPAN; j++) in[j] = s_rf[q][(r0 + j) * PH_RS + c];
      ph_taps(in, g, o);
#pragma unroll
      for (int j = 0; j < 4; j++) s_in[q][(r0 + j) * PH_RS + c] = o[j];
    }
  }
  __syncthreads();
  // ---- thread = 4 consecutive pixels of one row: x and y from memory, the weighted unit gradient to memory ----
  const int r = tid >> 3, cq = (tid & 7) * 4;
  const int y = y0 + r, x = x0 + cq;
  if (y >= H || x >= W) return;
  const float w_l1 = a.w_dev ? a.w_dev[3 * v] : a.w[3 * v];
  const float w_l2 = a.w_dev ? a.w_dev[3 * v + 1] : a.w[3 * v + 1];
  const float w_ss = a.w_dev ? a.w_dev[3 * v + 2] : a.w[3 * v + 2];
  const float inv_n = 1.0f / ((float)a.C * (float)N);
  const float k_l1 = w_l1 * inv_n, k_l2 = w_l2 * (2.0f * inv_n), k_ss = -(w_ss * inv_n);  // the term is 1 - ssim
  const size_t at = (size_t)plane * N + (size_t)y * W + x;
  const float* ty = a.tgt.p + (long long)v * a.tgt.sv + (long long)ch * a.tgt.sc + (long long)y * a.tgt.sh;
  float X[4], Y[4], o[4];
  if (a.vec) {
    const float4 q = *reinterpret_cast<const float4*>(a.color + at);
    X[0] = q.x; X[1] = q.y; X[2] = q.z; X[3] = q.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++) X[j] = x + j < W ? a.color[at + j] : 0.f;
  }
  if (a.tgt.vec) {
    const float4 q = *reinterpret_cast<const float4*>(ty + x);
    Y[0] = q.x; Y[1] = q.y; Y[2] = q.z; Y[3] = q.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++) Y[j] = x + j < W ? ty[(long long)(x + j) * a.tgt.sw] : 0.f;
  }
#pragma unroll
  for (int j = 0; j < 4; j++) {
#pragma clang fp contract(off)
    const float ga = s_in[0][r * PH_RS + cq + j], gb = s_in[1][r * PH_RS + cq + j], gc = s_in[2][r * PH_RS + cq + j];
    const float d = X[j] - Y[j];
    const float sgn = (float)(d > 0.f) - (float)(d < 0.f);
    const float dssim = (ga + (2.f * X[j]) * gb) + Y[j] * gc;
    o[j] = (k_l1 * sgn + k_l2 * d) + k_ss * dssim;
  }
  if (a.vec) {
    *reinterpret_cast<float4*>(a.unit + at) = make_float4(o[0], o[1], o[2], o[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (x + j < W) a.unit[at + j] = o[j];
  }
}

struct PhFinalArgs {
  int V, B;      // B: partial rows per view (channels x tiles)
  float n;       // C H W
  const float* partials;
  const float* w_dev;
  float w[3 * MAX_VIEWS];
  float* terms;  // [V][4]: l1, l2, ssim, psnr
  float* loss;
};

// One workgroup.  Wave w folds views w, w + 4, ...: lane l adds partials l, l + 64, ... in index order, then the butterfly.
__global__ void __launch_bounds__(PH_WG) photometric_finalize_kernel(PhFinalArgs a) {
  const int wave = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
  __shared__ float s_term[MAX_VIEWS][3];
  for (int v = wave; v < a.V; v += PH_WG / WAVE) {
    float s1 = 0.f, s2 = 0.f, sm = 0.f;
    for (int b = lane; b < a.B; b += WAVE) {
      const float* q = a.partials + 3 * ((size_t)v * a.B + b);
      s1 += q[0];
      s2 += q[1];
      sm += q[2];
    }
    s1 = wave_sum_shfl(s1);
    s2 = wave_sum_shfl(s2);
    sm = wave_sum_shfl(sm);
    if (lane == 0) {
      const float l1 = s1 / a.n, l2 = s2 / a.n, ssim = sm / a.n;
      a.terms[4 * v] = l1;
      a.terms[4 * v + 1] = l2;
      a.terms[4 * v + 2] = ssim;
      a.terms[4 * v + 3] = l2 == 0.f ? 100.0f : 20.0f * log10f(1.0f / sqrtf(l2));
      s_term[v][0] = l1;
      s_term[v][1] = l2;
      s_term[v][2] = 1.0f - ssim;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float loss = 0.f;  // loss = 0. ; loss += w_l1 * l1 ; loss += w_l2 * l2 ; loss += w_ssim * (1 - ssim) -- view by view
    for (int v = 0; v < a.V; v++) {
      const float* w = a.w_dev ? a.w_dev + 3 * v : a.w + 3 * v;
      loss += w[0] * s_term[v][0];
      loss += w[1] * s_term[v][1];
      loss += w[2] * s_term[v][2];
    }
    *a.loss = loss;
  }
}

// out[v] = g_up[v * stride] * unit[v]; per_view: elements of one view (a multiple of 4 on the 16-byte path)
__global__ void __launch_bounds__(PH_WG) photometric_bwd_kernel(const float* __restrict__ g_up, int stride,
                                                                const float* __restrict__ unit, float* __restrict__ out,
                                                                size_t per_view, int vec) {
  const int v = blockIdx.y;
  const float g = g_up[(size_t)v * stride];
  const size_t e = 4 * ((size_t)blockIdx.x * PH_WG + threadIdx.x);
  if (e >= per_view) return;
  const float* u = unit + (size_t)v * per_view + e;
  float* o = out + (size_t)v * per_view + e;
  if (vec && e + 4 <= per_view) {
    const float4 x = *reinterpret_cast<const float4*>(u);
    *reinterpret_cast<float4*>(o) = make_float4(g * x.x, g * x.y, g * x.z, g * x.w);
  } else {
    for (size_t j = 0; j < 4 && e + j < per_view; j++) o[j] = g * u[j];
  }
}

static int ph_shape_ok(const char* fn, int V, int C, int W, int H) {
  if (V < 1 || V > MAX_VIEWS) { set_error("%s: V = %d views (1 .. %d)", fn, V, MAX_VIEWS); return MGS_ERR_INVALID_ARG; }
  if (C < 1 || C > MGS_PHOTOMETRIC_MAX_CHANNELS) {
    set_error("%s: C = %d channels (1 .. %d)", fn, C, MGS_PHOTOMETRIC_MAX_CHANNELS);
    return MGS_ERR_INVALID_ARG;
  }
  if (W < 1 || H < 1 || (int64_t)W * H * C * V >= ((int64_t)1 << 31) || (H + PH_T - 1) / PH_T > 65535) {
    set_error("%s: image %d x %d (V = %d, C = %d) is empty or too large", fn, W, H, V, C);
    return MGS_ERR_INVALID_ARG;
  }
  return MGS_OK;
}

static size_t ph_tiles(int W, int H) { return (size_t)((W + PH_T - 1) / PH_T) * ((H + PH_T - 1) / PH_T); }
static size_t ph_maps_bytes(int V, int C, int W, int H) { return align_up(3 * (size_t)V * C * W * H * sizeof(float)); }
static size_t ph_partials_bytes(int V, int C, int W, int H) { return align_up(3 * (size_t)V * C * ph_tiles(W, H) * sizeof(float)); }

}  // namespace mgs

using namespace mgs;

extern "C" {

size_t mgs_photometric_workspace_bytes(int V, int C, int W, int H) {
  if (V < 1 || C < 1 || W < 1 || H < 1) return 0;
  return ph_maps_bytes(V, C, W, H) + ph_partials_bytes(V, C, W, H);
}

int mgs_photometric_forward(int V, int C, int W, int H, const float* color, const float* target, const int64_t* target_strides,
                            const float* weights_host, const float* weights_dev, float* unit_grad, float* terms, float* loss,
                            void* workspace, size_t workspace_bytes, mgs_stream_t stream) {
  const char* fn = "photometric_fwd";
  if (int rc = ph_shape_ok(fn, V, C, W, H)) return rc;
  if (!color || !target || !target_strides || !terms || !loss || !workspace) { set_error("%s: NULL pointer", fn); return MGS_ERR_INVALID_ARG; }
  if (weights_host && weights_dev) { set_error("%s: weights given by value and as a device pointer", fn); return MGS_ERR_INVALID_ARG; }
  if (misaligned16(workspace)) { set_error("%s: the workspace is not 16-byte aligned", fn); return MGS_ERR_INVALID_ARG; }
  if (int rc = workspace_short(fn, workspace_bytes, mgs_photometric_workspace_bytes(V, C, W, H))) return rc;
  const int64_t* st = target_strides;
  const int64_t dims[4] = {V, C, H, W};
  int64_t last = 0;
  for (int i = 0; i < 4; i++) {
    if (st[i] < 0) { set_error("%s: target has a negative stride", fn); return MGS_ERR_INVALID_ARG; }
    last += (dims[i] - 1) * st[i];
  }
  if (last >= ((int64_t)1 << 31)) { set_error("%s: target spans 2^31 elements or more", fn); return MGS_ERR_INVALID_ARG; }
  PhArgs a = {};
  a.V = V; a.C = C; a.W = W; a.H = H;
  a.tiles_x = (W + PH_T - 1) / PH_T; a.tiles_y = (H + PH_T - 1) / PH_T;
  a.vec = (W % 4 == 0) && !misaligned16(color) && (!unit_grad || !misaligned16(unit_grad));
  a.color = color;
  a.tgt.p = target; a.tgt.sv = st[0]; a.tgt.sc = st[1]; a.tgt.sh = st[2]; a.tgt.sw = st[3];
  a.tgt.vec = (W % 4 == 0) && !misaligned16(target) && st[3] == 1 && (V == 1 || st[0] % 4 == 0) && (C == 1 || st[1] % 4 == 0) &&
              (H == 1 || st[2] % 4 == 0);
  a.w_dev = weights_dev;
  for (int i = 0; i < 3 * V; i++) a.w[i] = weights_host ? weights_host[i] : 1.0f;
  a.maps = unit_grad ? reinterpret_cast<float*>(workspace) : nullptr;
  a.partials = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + ph_maps_bytes(V, C, W, H));
  a.unit = unit_grad;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(a.tiles_x, a.tiles_y, V * C);
  hipLaunchKernelGGL(photometric_fwd_kernel, grid, dim3(PH_WG), 0, s, a);
  if (unit_grad) hipLaunchKernelGGL(photometric_grad_kernel, grid, dim3(PH_WG), 0, s, a);
  PhFinalArgs f = {};
  f.V = V; f.B = C * a.tiles_x * a.tiles_y; f.n = (float)C * (float)W * (float)H;
  f.partials = a.partials; f.w_dev = weights_dev;
  for (int i = 0; i < 3 * V; i++) f.w[i] = a.w[i];
  f.terms = terms; f.loss = loss;
  hipLaunchKernelGGL(photometric_finalize_kernel, dim3(1), dim3(PH_WG), 0, s, f);
  return launch_done(fn);
}

int mgs_photometric_backward(int V, int C, int W, int H, const float* g_up, int g_up_stride, const float* unit_grad, float* out,
                             mgs_stream_t stream) {
  const char* fn = "photometric_bwd";
  if (int rc = ph_shape_ok(fn, V, C, W, H)) return rc;
  if (!g_up) { set_error("%s: g_up is NULL", fn); return MGS_ERR_INVALID_ARG; }
  if (g_up_stride != 0 && g_up_stride != 1) { set_error("%s: g_up_stride = %d (0: one scalar, 1: one value per view)", fn, g_up_stride); return MGS_ERR_INVALID_ARG; }
  if (!unit_grad || !out) { set_error("%s: NULL pointer", fn); return MGS_ERR_INVALID_ARG; }
  const size_t per_view = (size_t)C * W * H;
  const int vec = per_view % 4 == 0 && !misaligned16(unit_grad) && !misaligned16(out);
  const size_t quads = (per_view + 3) / 4;
  hipLaunchKernelGGL(photometric_bwd_kernel, dim3((unsigned)((quads + PH_WG - 1) / PH_WG), V), dim3(PH_WG), 0, (hipStream_t)stream,
                     g_up, g_up_stride, unit_grad, out, per_view, vec);
  return launch_done(fn);
}

}  // extern "C"
