// mgs_optim.hip -- one LAMB step for any number of parameter tensors, in two launches.
// Reference: helpers/optim/lamb.py:47-111 (the cybertronai LAMB: no bias correction, weight norm clamped to [0, 10], trust
// ratio 1 where either norm is zero).  The reference loops over the tensors in Python: about a dozen small kernels, three
// temporaries and two device reads per tensor.  Here the tensors are cut into chunks of LAMB_CHUNK elements (a chunk never
// straddles tensors) and one workgroup takes one chunk:
//   lamb_moments_kernel  reads p, g, m, v; writes m, v (and zeroes g if asked); ONE pair {sum p^2, sum u^2} per chunk
//   lamb_apply_kernel    every workgroup adds its tensor's pairs in the same fixed order, forms the trust ratio with the two
//                        == 0 tests, re-forms u from m, v, p and writes p; chunk 0 of a tensor writes its three statistics
// 16 + 12 bytes read and 8 + 4 written per parameter.  Stream order is the only synchronisation: no atomics, no host read, no
// allocation; results are bit-identical from run to run and the two launches can be captured into a HIP graph as they are.
// Every table (tensors, groups, chunk map) is read from device memory, so a captured step follows what the caller writes there.
#include "mgs_common.h"
#include "mgs_device.h"

namespace mgs {

constexpr int LAMB_WG = 256;                             // 4 x wave64
constexpr int LAMB_Q = 4;                                // 16-byte groups per thread
constexpr int LAMB_CHUNK = LAMB_WG * 4 * LAMB_Q;         // 4096 elements = 16 KB of each of p, g, m, v

struct LambArgs {
  const MgsLambTensor* tensors;
  const MgsLambGroup* groups;
  const int2* chunk_map;   // {tensor, chunk inside the tensor}
  float *m, *v;            // flat moments
  float* stats;            // [n_tensors][3]
  float2* partials;        // [n_chunks] {sum p^2, sum u^2}
  float grad_scale;
  int zero_grad;
};

// Four consecutive elements from element i of a tensor of n: one 16-byte access where the base is aligned and the group is
// whole, else element by element (0 past the end).  The element -> thread mapping is the same either way, so a tensor gives the
// same bits whether or not its pointers happen to be aligned.
__device__ __forceinline__ void ld4(const float* __restrict__ b, int64_t i, int64_t n, bool vec, float (&o)[4]) {
  if (vec && i + 4 <= n) {
    const float4 q = *reinterpret_cast<const float4*>(b + i);
    o[0] = q.x; o[1] = q.y; o[2] = q.z; o[3] = q.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++) o[j] = (i + j < n) ? b[i + j] : 0.f;
  }
}

__device__ __forceinline__ void st4(float* __restrict__ b, int64_t i, int64_t n, bool vec, const float (&o)[4]) {
  if (vec && i + 4 <= n) {
    *reinterpret_cast<float4*>(b + i) = make_float4(o[0], o[1], o[2], o[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (i + j < n) b[i + j] = o[j];
  }
}

// lamb.py:94-96
__device__ __forceinline__ float lamb_u(float m, float v, float p, float eps, float wd) {
  float u = m / (sqrtf(v) + eps);
  if (wd != 0.f) u += wd * p;
  return u;
}

__global__ void __launch_bounds__(LAMB_WG) lamb_moments_kernel(LambArgs a) {
  const int2 cm = a.chunk_map[blockIdx.x];
  const MgsLambTensor t = a.tensors[cm.x];
  if (t.g == nullptr) return;  // no gradient: the tensor is skipped entirely (lamb.py:59-60)
  const MgsLambGroup h = a.groups[t.group];
  const bool p_vec = t.flags & MGS_LAMB_P_ALIGNED, g_vec = t.flags & MGS_LAMB_G_ALIGNED;
  const int64_t n = t.numel, n4 = (n + 3) & ~(int64_t)3;  // the moments' slot is padded to whole 16-byte groups
  float* __restrict__ m = a.m + t.state_off;
  float* __restrict__ v = a.v + t.state_off;
  const int64_t base = (int64_t)cm.y * LAMB_CHUNK + 4 * (int64_t)threadIdx.x;
  float s_p = 0.f, s_u = 0.f;
  const float zero[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int q = 0; q < LAMB_Q; q++) {
    const int64_t i = base + (int64_t)q * (LAMB_WG * 4);
    if (i >= n) break;
    float p[4], g[4], mm[4], vv[4];
    ld4(t.p, i, n, p_vec, p);
    ld4(t.g, i, n, g_vec, g);
    ld4(m, i, n4, true, mm);
    ld4(v, i, n4, true, vv);
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const float gs = g[j] * a.grad_scale;
      mm[j] = mm[j] * h.beta1 + gs * h.one_minus_beta1;
      vv[j] = vv[j] * h.beta2 + gs * gs * h.one_minus_beta2;
      if (i + j < n) {  // (the padding of the last group holds zeros: 0 / (0 + eps) must not reach the sums when eps = 0)
        const float u = lamb_u(mm[j], vv[j], p[j], h.eps, h.weight_decay);
        s_p += p[j] * p[j];
        s_u += u * u;
      }
    }
    st4(m, i, n4, true, mm);
    st4(v, i, n4, true, vv);
    if (a.zero_grad) st4(t.g, i, n, g_vec, zero);
  }
  // ---- workgroup reduction: wave butterflies, four waves through LDS, one plain store ----
  s_p = wave_sum_shfl(s_p);
  s_u = wave_sum_shfl(s_u);
  __shared__ float s_part[LAMB_WG / WAVE][2];
  const int wave = threadIdx.x / WAVE;
  if ((threadIdx.x & (WAVE - 1)) == 0) { s_part[wave][0] = s_p; s_part[wave][1] = s_u; }
  __syncthreads();
  if (threadIdx.x == 0)
    a.partials[t.chunk0 + cm.y] = make_float2((s_part[0][0] + s_part[1][0]) + (s_part[2][0] + s_part[3][0]),
                                              (s_part[0][1] + s_part[1][1]) + (s_part[2][1] + s_part[3][1]));
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

__global__ void __launch_bounds__(LAMB_WG) lamb_apply_kernel(LambArgs a) {
  const int2 cm = a.chunk_map[blockIdx.x];
  const MgsLambTensor t = a.tensors[cm.x];
  if (t.g == nullptr) return;
  const MgsLambGroup h = a.groups[t.group];
  // ---- the tensor's norms: thread i adds pairs i, i + 256, ... in index order, then butterfly and the four waves in order.
  // The same sequence in every workgroup of the tensor, so all of them hold bit-identical norms.  (A 512 x 512 weight has 64
  // pairs, 100 000 x 32 Gaussian features 782: 6 KB from L2 per workgroup, against the 48 KB it streams.)
  double sp = 0.0, su = 0.0;
  for (int c = threadIdx.x; c < t.n_chunks; c += LAMB_WG) {
    const float2 q = a.partials[t.chunk0 + c];
    sp += (double)q.x;
    su += (double)q.y;
  }
  sp = wave_sum_f64(sp);
  su = wave_sum_f64(su);
  __shared__ double s_part[LAMB_WG / WAVE][2];
  const int wave = threadIdx.x / WAVE;
  if ((threadIdx.x & (WAVE - 1)) == 0) { s_part[wave][0] = sp; s_part[wave][1] = su; }
  __syncthreads();
  sp = (s_part[0][0] + s_part[1][0]) + (s_part[2][0] + s_part[3][0]);
  su = (s_part[0][1] + s_part[1][1]) + (s_part[2][1] + s_part[3][1]);
  const float wn = (float)sqrt(sp);
  const float weight_norm = wn > 10.0f ? 10.0f : wn;  // clamp(0, 10), lamb.py:92; a comparison: a NaN norm stays NaN (fminf drops it)
  const float adam_norm = (float)sqrt(su);
  const float trust = (weight_norm == 0.f || adam_norm == 0.f) ? 1.0f : weight_norm / adam_norm;  // lamb.py:99-102
  if (cm.y == 0 && threadIdx.x == 0) {
    float* s = a.stats + 3 * (size_t)cm.x;
    s[0] = weight_norm; s[1] = adam_norm; s[2] = trust;
  }
  const float lr = h.lr_dev ? *h.lr_dev : h.lr;
  const float step = lr * (h.adam ? 1.0f : trust);  // adam: the applied ratio is 1, the recorded one is not (lamb.py:103-107)
  const bool p_vec = t.flags & MGS_LAMB_P_ALIGNED;
  const int64_t n = t.numel, n4 = (n + 3) & ~(int64_t)3;
  const float* __restrict__ m = a.m + t.state_off;
  const float* __restrict__ v = a.v + t.state_off;
  const int64_t base = (int64_t)cm.y * LAMB_CHUNK + 4 * (int64_t)threadIdx.x;
#pragma unroll
  for (int q = 0; q < LAMB_Q; q++) {
    const int64_t i = base + (int64_t)q * (LAMB_WG * 4);
    if (i >= n) break;
    float p[4], mm[4], vv[4];
    ld4(t.p, i, n, p_vec, p);
    ld4(m, i, n4, true, mm);
    ld4(v, i, n4, true, vv);
#pragma unroll
    for (int j = 0; j < 4; j++) p[j] -= step * lamb_u(mm[j], vv[j], p[j], h.eps, h.weight_decay);
    st4(t.p, i, n, p_vec, p);
  }
}

}  // namespace mgs

using namespace mgs;

extern "C" {

int mgs_lamb_chunk_elems(void) { return LAMB_CHUNK; }

size_t mgs_lamb_workspace_bytes(int64_t n_chunks) {
  if (n_chunks < 1) return 0;
  return align_up((size_t)n_chunks * sizeof(float2));
}

int mgs_lamb_step(int n_tensors, int n_groups, int64_t n_chunks, const MgsLambTensor* tensors, const MgsLambGroup* groups,
                  const int32_t* chunk_map, float* exp_avg, float* exp_avg_sq, float* stats, float grad_scale, int zero_grad,
                  void* workspace, size_t workspace_bytes, mgs_stream_t stream) {
  const char* fn = "lamb_step";
  if (n_tensors < 1 || n_groups < 1 || n_chunks < n_tensors || n_chunks >= ((int64_t)1 << 31)) {
    set_error("%s: %d tensors, %d groups, %lld chunks (every tensor has at least one chunk; fewer than 2^31)", fn, n_tensors,
              n_groups, (long long)n_chunks);
    return MGS_ERR_INVALID_ARG;
  }
  if (!tensors || !groups || !chunk_map || !exp_avg || !exp_avg_sq || !stats || !workspace) {
    set_error("%s: NULL pointer", fn);
    return MGS_ERR_INVALID_ARG;
  }
  if ((reinterpret_cast<uintptr_t>(exp_avg) | reinterpret_cast<uintptr_t>(exp_avg_sq) | reinterpret_cast<uintptr_t>(workspace) |
       reinterpret_cast<uintptr_t>(tensors) | reinterpret_cast<uintptr_t>(groups) | reinterpret_cast<uintptr_t>(chunk_map)) & 15u) {
    set_error("%s: the moment buffers, the tables and the workspace must be 16-byte aligned", fn);
    return MGS_ERR_INVALID_ARG;
  }
  if (int rc = workspace_short(fn, workspace_bytes, mgs_lamb_workspace_bytes(n_chunks))) return rc;
  LambArgs a = {};
  a.tensors = tensors; a.groups = groups; a.chunk_map = reinterpret_cast<const int2*>(chunk_map);
  a.m = exp_avg; a.v = exp_avg_sq; a.stats = stats; a.partials = reinterpret_cast<float2*>(workspace);
  a.grad_scale = grad_scale; a.zero_grad = zero_grad;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(lamb_moments_kernel, dim3((unsigned)n_chunks), dim3(LAMB_WG), 0, s, a);
  hipLaunchKernelGGL(lamb_apply_kernel, dim3((unsigned)n_chunks), dim3(LAMB_WG), 0, s, a);
  return launch_done(fn);
}

}  // extern "C"
