// mgs_selftest.hip -- device self-test of the wave64 cross-lane primitives the kernels rely on (mgs_selftest) and a
// kernel with a KNOWN instruction mix for validating rocprofv3 counter passes (mgs_calibration_kernel).
#include "mgs_common.h"
#include "mgs_device.h"
#include "mgs_render_common.h"

namespace mgs {

// Checks the cross-lane primitives against their definitions with small integers (exact in fp32).
__global__ void selftest_kernel(int* result) {
  const int lane = threadIdx.x;
  int bad = 0;
  {  // swap32: lanes 32..63 of x <-> lanes 0..31 of y
    float x = (float)lane, y = (float)(100 + lane);
    swap32(x, y);
    const float ex = lane < 32 ? (float)lane : (float)(100 + lane - 32);
    const float ey = lane < 32 ? (float)(lane + 32) : (float)(100 + lane);
    if (x != ex || y != ey) bad |= 1;
  }
  if (bcast_lane((float)lane, 37) != 37.f) bad |= 2048;
  if (bcast_lane_u32((uint32_t)lane * 5u, 63) != 315u) bad |= 4096;
  if (wave_umax((uint32_t)lane * 3u) != 189u) bad |= 8192;
  if (wave_umax((uint32_t)((lane * 37) % 64)) != 63u) bad |= 8192;
  {  // 64-lane inclusive prefix sum
    const uint32_t x = (uint32_t)((lane * 7) % 5 + 1);
    uint32_t e = 0;
    for (int i = 0; i <= lane; i++) e += (uint32_t)((i * 7) % 5 + 1);
    if (wave_incl_scan_add_u32(x) != e) bad |= 1 << 24;
  }
  {
    const uint32_t v = (uint32_t)lane * 2654435761u;
    if (lane_xor<1>(v, lane) != (uint32_t)(lane ^ 1) * 2654435761u) bad |= 1 << 14;
    if (lane_xor<2>(v, lane) != (uint32_t)(lane ^ 2) * 2654435761u) bad |= 1 << 15;
    if (lane_xor<4>(v, lane) != (uint32_t)(lane ^ 4) * 2654435761u) bad |= 1 << 16;
    if (lane_xor<8>(v, lane) != (uint32_t)(lane ^ 8) * 2654435761u) bad |= 1 << 17;
    if (lane_xor<16>(v, lane) != (uint32_t)(lane ^ 16) * 2654435761u) bad |= 1 << 18;
    if (lane_xor<32>(v, lane) != (uint32_t)(lane ^ 32) * 2654435761u) bad |= 1 << 19;
  }
  {  // half-wave scans (small integers: exact in float)
    const int n = lane & 31;
    const float a = (float)((lane * 5) % 7 + 1);
    float ea = 0.f;
    for (int i = 0; i <= n; i++) ea += (float)((((lane & 32) + i) * 5) % 7 + 1);
    if (half_incl_scan_add(a) != ea) bad |= 1 << 20;
    const float m = (lane % 3 == 0) ? 2.f : 1.f;
    float em = 1.f;
    for (int i = 0; i < n; i++) em *= (((lane & 32) + i) % 3 == 0) ? 2.f : 1.f;
    if (half_excl_scan_mul(m, lane) != em) bad |= 1 << 21;
    if (half_last((float)lane, lane) != ((lane & 32) ? 63.f : 31.f)) bad |= 1 << 22;
    // the two-at-a-time forms of the render backward's double pixel step: each chain equals its single scan
    const float a2 = (float)((lane * 3) % 5 + 1), m2 = (lane % 4 == 1) ? 2.f : 1.f;
    float ea2 = 0.f, em2 = 1.f;
    for (int i = 0; i <= n; i++) ea2 += (float)((((lane & 32) + i) * 3) % 5 + 1);
    for (int i = 0; i < n; i++) em2 *= (((lane & 32) + i) % 4 == 1) ? 2.f : 1.f;
    float sa = a, sb = a2;
    half_incl_scan_add2(sa, sb);
    if (sa != ea || sb != ea2) bad |= 1 << 26;
    float pa = m, pb = m2;
    half_excl_scan_mul2(pa, pb, lane);
    if (pa != em || pb != em2) bad |= 1 << 27;
    // exclusive suffix sums (the render backward's "what lies behind me"), one and two at a time
    float xa = 0.f, xa2 = 0.f;
    for (int i = n + 1; i < 32; i++) {
      xa += (float)((((lane & 32) + i) * 5) % 7 + 1);
      xa2 += (float)((((lane & 32) + i) * 3) % 5 + 1);
    }
    const float y1 = (float)(100 + lane), y2 = (float)(300 - lane);  // the per-lane addends
    if (half_excl_suffix_add(a, y1) != xa + y1) bad |= (int)0x80000000u;
    float ua = a, ub = a2;
    half_excl_suffix_add2(ua, ub, y1, y2);
    if (ua != xa + y1 || ub != xa2 + y2) bad |= (int)0x80000000u;
  }
  {  // the fp32 MFMA the render kernels use is exact fp32: C = A (32x2) * B (2x32) with small integers
    using f32x16 = __attribute__((ext_vector_type(16))) float;
    f32x16 c;
    for (int i = 0; i < 16; i++) c[i] = 0.f;
    const float a = (float)((lane & 31) + 1 + 100 * (lane >> 5));  // A[i = lane & 31][k = lane >> 5]
    const float b = (float)(2 * (lane & 31) + 1 + (lane >> 5));    // B[k = lane >> 5][j = lane & 31]
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
    for (int i = 0; i < 16; i++) {
      const int row = (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5), col = lane & 31;
      const float want = (float)(row + 1) * (float)(2 * col + 1) + (float)(row + 101) * (float)(2 * col + 2);
      if (c[i] != want) bad |= 1 << 23;
    }
  }
  {  // the render kernels' exact exp (ocml's expf without its range clamps) is expf, bit for bit, over the range that matters:
     // 64 lanes x 4096 steps sweep x in (-100, 0] on a grid no float pattern favours, plus a few positive values
    for (int i = 0; i < 4096; i++) {
      const float x = -((float)(lane * 4096 + i) * 3.8146973e-4f + (float)i * 1.1920929e-7f);
      if (__float_as_uint(exp_ocml_unclamped(x)) != __float_as_uint(expf(x))) bad |= 1 << 25;
    }
    const float xp = (float)lane * 1.37f;
    if (__float_as_uint(exp_ocml_unclamped(xp)) != __float_as_uint(expf(xp))) bad |= 1 << 25;
    // ... and its two-wide form (packed multiply-adds: the same roundings)
    for (int i = 0; i < 1024; i++) {
      const float x0 = -((float)(lane * 1024 + i) * 1.5258789e-3f + (float)i * 2.3841858e-7f), x1 = x0 * 0.37f - 0.011f;
      const f32x2 e2 = exp_ocml_unclamped2(f32x2{x0, x1});
      if (__float_as_uint(e2.x) != __float_as_uint(expf(x0)) || __float_as_uint(e2.y) != __float_as_uint(expf(x1))) bad |= 1 << 28;
    }
    // the pair exponent: its packed form rounds like its scalar form (conic and offsets of the sizes the renderer sees)
    for (int i = 0; i < 1024; i++) {
      const float cx = 0.01f + (float)((lane * 37 + i * 11) % 997) * 3.1e-3f, cz = 0.02f + (float)((lane * 53 + i * 7) % 991) * 2.7e-3f;
      const float cy = ((float)((lane * 29 + i * 13) % 983) - 491.f) * 1.9e-3f;
      const float dx0 = ((float)((lane * 17 + i * 5) % 1021) - 510.f) * 0.0313f, dy = ((float)((lane * 3 + i * 19) % 1019) - 509.f) * 0.0291f;
      const f32x2 p2 = gauss_power2(cx, cy, cz, f32x2{dx0, dx0 - 1.0f}, dy);
      if (__float_as_uint(p2.x) != __float_as_uint(gauss_power(cx, cy, cz, dx0, dy)) ||
          __float_as_uint(p2.y) != __float_as_uint(gauss_power(cx, cy, cz, dx0 - 1.0f, dy))) bad |= 1 << 29;
      const f32x2 p3 = gauss_power2v(f32x2{cx, cz}, f32x2{cy, -cy}, f32x2{cz, cx}, f32x2{dx0, dy}, f32x2{dy, dx0});
      if (__float_as_uint(p3.x) != __float_as_uint(gauss_power(cx, cy, cz, dx0, dy)) ||
          __float_as_uint(p3.y) != __float_as_uint(gauss_power(cz, -cy, cx, dy, dx0))) bad |= 1 << 29;
    }
    {  // known answer: the pair whose alpha sits 1 ulp under 1/255 in the reference's kernels (fuzz_parity seed 101 case 234,
       // pixel (77, 5), Gaussian 56): the reference's roundings give power 0xbf9e36a4 and alpha 0x3b808080 < 1/255 = 0x3b808081
      const float x = __uint_as_float(0x42836bbau), y = __uint_as_float(0xbfaa7610u), cx = __uint_as_float(0x3d3ade4fu);
      const float cy = __uint_as_float(0xbd8604a9u), cz = __uint_as_float(0x3e1993fdu), o = __uint_as_float(0x3c5d264cu);
      const float p = gauss_power(cx, cy, cz, x - 77.0f, y - 5.0f);
      if (__float_as_uint(p) != 0xbf9e36a4u || __float_as_uint(o * exp_ocml_unclamped(p)) != 0x3b808080u) bad |= 1 << 29;
    }
  }
  {  // the pair's pixel offsets: the two-pixel backward forms them as ONE packed subtraction from the exact pixel coordinates,
     // which must equal the forward's and the one-pixel form's scalar `ex - px` bit for bit -- also where |dx| crosses a power
     // of two inside the pair and ex - px is inexact (ex in (0, 1), columns 64 / 65, 128 / 129, ...: advisor r5)
    for (int i = 0; i < 2048; i++) {
      const float ex = ((float)((lane * 131 + i * 7) % 4093) + 0.5f) * 2.4414062e-4f + (float)(i & 3) * 5.9604645e-8f;  // (0, 1)
      const float px0 = (float)(((i >> 2) & 1) ? (32 << ((i >> 3) % 3)) : ((lane * 5 + i) % 126));  // 32, 64, 128 or any column
      const f32x2 dx = f32x2{ex, ex} - f32x2{px0, px0 + 1.0f};
      if (__float_as_uint(dx.x) != __float_as_uint(ex - px0) || __float_as_uint(dx.y) != __float_as_uint(ex - (px0 + 1.0f))) bad |= 1 << 30;
    }
  }
  if (bad) atomicOr(result, bad);
}

hipError_t launch_selftest(int* result_dev, hipStream_t s) {
  hipLaunchKernelGGL(selftest_kernel, dim3(1), dim3(64), 0, s, result_dev);
  return hipGetLastError();
}

// Known instruction mix per wave and iteration: 64 v_fma_f32, 8 v_mfma_f32_32x32x2_f32, 4 ds_read_b32 (+ loop overhead:
// one s_add / s_cmp / s_cbranch).  256 workgroups x 4 waves.  scripts/sq_counters.py divides the counters of this
// kernel by (256 * 4 * iters) and expects 64 / 8 / 4 before it trusts a pass.
__global__ void __launch_bounds__(256) calibration_kernel(int iters, float* __restrict__ sink) {
  using f32x16 = __attribute__((ext_vector_type(16))) float;
  __shared__ float lds[1024];
  const int tid = threadIdx.x;
  for (int i = tid; i < 1024; i += 256) lds[i] = (float)i * 1e-3f;
  __syncthreads();
  float v[8];
#pragma unroll
  for (int i = 0; i < 8; i++) v[i] = (float)(tid + i) * 1e-6f;
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; i++) acc[i] = 0.f;
  float l0 = 0.f, l1 = 0.f, l2 = 0.f, l3 = 0.f;
  const float m = 0.999f;
  for (int it = 0; it < iters; it++) {
#pragma unroll
    for (int k = 0; k < 8; k++) {
#pragma unroll
      for (int i = 0; i < 8; i++) asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(v[i]) : "v"(m), "v"(v[(i + 1) & 7]));
      asm volatile("v_mfma_f32_32x32x2_f32 %0, %1, %2, %0" : "+v"(acc) : "v"(v[k]), "v"(m));
    }
    asm volatile("ds_read_b32 %0, %1" : "=v"(l0) : "v"((tid & 255) * 4));
    asm volatile("ds_read_b32 %0, %1 offset:1024" : "=v"(l1) : "v"((tid & 255) * 4));
    asm volatile("ds_read_b32 %0, %1 offset:2048" : "=v"(l2) : "v"((tid & 255) * 4));
    asm volatile("ds_read_b32 %0, %1 offset:3072" : "=v"(l3) : "v"((tid & 255) * 4));
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }
  float r = l0 + l1 + l2 + l3 + lds[tid];
#pragma unroll
  for (int i = 0; i < 8; i++) r += v[i];
#pragma unroll
  for (int i = 0; i < 16; i++) r += acc[i];
  sink[(size_t)blockIdx.x * 256 + tid] = r;
}

hipError_t launch_calibration(int iters, float* sink, hipStream_t s) {
  hipLaunchKernelGGL(calibration_kernel, dim3(256), dim3(256), 0, s, iters, sink);
  return hipGetLastError();
}

}  // namespace mgs
