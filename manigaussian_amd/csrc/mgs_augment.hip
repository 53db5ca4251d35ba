// mgs_augment.hip -- the agent's SE(3) augmentation (voxel/augmentation.py:11-377) without a host read: the reference's rejection
// loop (draw a perturbation, compose it with the gripper pose, discretise, retry while a sample left the bounds) and its
// transform of every camera's cloud and pose, in two launches whatever the batch, the camera count or the attempts.
//
//   se3_select_kernel  ONE workgroup.  All attempts x samples candidates are evaluated side by side (a candidate depends on
//                      nothing but its draw), the first attempt in which every sample is valid is found through LDS, and the
//                      chosen candidates are evaluated once more to write the actions and one transform record per sample.
//   se3_apply_kernel   one thread per point, planes read and written coalesced; the last block column of every (sample, source)
//                      transforms that source's camera pose.
//   se3_draws_kernel   the draw table of a (seed, offset): what select generates, as a test and debug aid.
//
// Precision follows the reference line by line (include/mgsplat.h): the composition is fp32 as torch runs it, the discretisation
// fp64 on those fp32 values as numpy and scipy run it.  The work is tiny; what this file buys is the missing synchronisation
// (no device read, no host loop), determinism and capturability -- not bandwidth.
#include <math.h>

#include "mgs_common.h"
#include "mgs_device.h"

namespace mgs {

constexpr int SE3_WG = 256;
constexpr int SE3_REC = 16;  // floats of a transform record: S[9] row-major, pivot[3], target[3], 1.0f = transform / 0.0f = identity

struct Se3K {
  int B, A, retry, layer, V, bounds_rows, rot_bins, trans_f64, action_i64;
  int k[3];
  float step_rad;
  double rot_res;
  double tar[3];
  const float* pose;
  const void* act_trans;
  const void* act_rot;
  const float* bounds;
  const unsigned long long* rng;
  const float* draws;
  long long* out_trans;
  long long* out_rot;
  int* info;
  float* rec;
};

struct Se3Apply {
  int B, n_src, n_pose;
  const float* rec;
  const float* src[MGS_SE3_MAX_SOURCES];
  float* dst[MGS_SE3_MAX_SOURCES];
  int n[MGS_SE3_MAX_SOURCES];
  int64_t sb[MGS_SE3_MAX_SOURCES], sc[MGS_SE3_MAX_SOURCES];
  const float* pose_in[MGS_SE3_MAX_SOURCES];
  float* pose_out[MGS_SE3_MAX_SOURCES];
};

// ---- the draw of (attempt a, sample b): d[0..2] = trans_u in [-1, 1), d[3..5] = roll, pitch, yaw steps as floats
__device__ __forceinline__ float se3_step(uint32_t word, int k) {
  return (float)((int)(((unsigned long long)word * (unsigned)(2 * k + 1)) >> 32) - k);
}
__device__ __forceinline__ float se3_unit(uint32_t word) { return (float)(word >> 8) * 0x1p-23f - 1.f; }

__device__ __forceinline__ void se3_generate(const Philox& ph, const int (&k)[3], int a, int b, float (&d)[6]) {
  const uint4 w0 = philox4(ph, 0u, (uint32_t)a, (uint32_t)b), w1 = philox4(ph, 1u, (uint32_t)a, (uint32_t)b);
  d[0] = se3_unit(w0.x); d[1] = se3_unit(w0.y); d[2] = se3_unit(w0.z);
  d[3] = se3_step(w0.w, k[0]); d[4] = se3_step(w1.x, k[1]); d[5] = se3_step(w1.y, k[2]);
}

__device__ __forceinline__ void mat3_mul(const float (&x)[9], const float (&y)[9], float (&o)[9]) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) o[3 * i + j] = fmaf(x[3 * i + 2], y[6 + j], fmaf(x[3 * i + 1], y[3 + j], x[3 * i] * y[j]));
}

struct Se3Cand {
  bool valid;
  long long trans[3], rot[3];
  float S[9], shift[3], pivot[3];
};

// One candidate, start to end (see the header for every step's precision).
__device__ void se3_candidate(const Se3K& p, const Philox& ph, int a, int b, Se3Cand& c) {
  float d[6];
  if (p.draws) {
    const float* __restrict__ row = p.draws + ((int64_t)a * p.B + b) * 6;
#pragma unroll
    for (int i = 0; i < 6; i++) d[i] = row[i];
  } else {
    se3_generate(ph, p.k, a, b, d);
  }
  // gripper pose -> rotation G (fp32) and translation
  const float* __restrict__ g = p.pose + (int64_t)b * 7;
  const float qi = g[3], qj = g[4], qk = g[5], qr = g[6];
  const float two_s = 2.f / (qr * qr + qi * qi + qj * qj + qk * qk);
  const float G[9] = {1.f - two_s * (qj * qj + qk * qk), two_s * (qi * qj - qk * qr), two_s * (qi * qk + qj * qr),
                      two_s * (qi * qj + qk * qr), 1.f - two_s * (qi * qi + qk * qk), two_s * (qj * qk - qi * qr),
                      two_s * (qi * qk - qj * qr), two_s * (qj * qk + qi * qr), 1.f - two_s * (qi * qi + qj * qj)};
  // S = Rx(roll) Ry(pitch) Rz(yaw); sine and cosine correctly rounded to fp32
  float cs[3], sn[3];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const float ang = (p.k[i] > 0 ? rintf(d[3 + i]) : 0.f) * p.step_rad;
    cs[i] = (float)cos((double)ang);
    sn[i] = (float)sin((double)ang);
  }
  const float Rx[9] = {1.f, 0.f, 0.f, 0.f, cs[0], -sn[0], 0.f, sn[0], cs[0]};
  const float Ry[9] = {cs[1], 0.f, sn[1], 0.f, 1.f, 0.f, -sn[1], 0.f, cs[1]};
  const float Rz[9] = {cs[2], -sn[2], 0.f, sn[2], cs[2], 0.f, 0.f, 0.f, 1.f};
  float Rxy[9], M[9];
  mat3_mul(Rx, Ry, Rxy);
  mat3_mul(Rxy, Rz, c.S);
  mat3_mul(G, c.S, M);
  // translation, and its voxel index against the bounds row of the layer
  const float* __restrict__ br = p.bounds + (p.bounds_rows > 1 ? (int64_t)b * 6 : 0);
  const float* __restrict__ bd = p.bounds + ((p.layer > 0 && p.bounds_rows > 1) ? (int64_t)b * 6 : 0);
  c.valid = true;
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const float range = br[3 + i] - br[i];
    float pt;
    if (p.trans_f64) {
      const double sh = (double)range * p.tar[i] * (double)d[i];
      c.shift[i] = (float)sh;
      pt = (float)((double)g[i] + sh);
    } else {
      c.shift[i] = range * (float)p.tar[i] * d[i];
      pt = g[i] + c.shift[i];
    }
    c.pivot[i] = g[i];
    const double res = (double)(bd[3 + i] - bd[i]) / ((double)p.V + 1e-12);
    const double f = floor((double)(pt - bd[i]) / (res + 1e-12));
    if (!(f >= 0.0)) c.valid = false;  // (NaN is invalid too)
    c.trans[i] = f >= 0.0 ? (long long)fmin(f, (double)(p.V - 1)) : -1;
  }
  // rotation -> quaternion xyzw (fp64, the largest of the four candidates), rounded to fp32 as the reference hands it to numpy
  double m[3][3];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) m[i][j] = (double)M[3 * i + j];
  const double tr = m[0][0] + m[1][1] + m[2][2];
  double q[4];
  if (tr >= m[0][0] && tr >= m[1][1] && tr >= m[2][2]) {
    q[0] = m[2][1] - m[1][2]; q[1] = m[0][2] - m[2][0]; q[2] = m[1][0] - m[0][1]; q[3] = 1.0 + tr;
  } else if (m[0][0] >= m[1][1] && m[0][0] >= m[2][2]) {
    q[0] = 1.0 - tr + 2.0 * m[0][0]; q[1] = m[1][0] + m[0][1]; q[2] = m[2][0] + m[0][2]; q[3] = m[2][1] - m[1][2];
  } else if (m[1][1] >= m[2][2]) {
    q[1] = 1.0 - tr + 2.0 * m[1][1]; q[2] = m[2][1] + m[1][2]; q[0] = m[0][1] + m[1][0]; q[3] = m[0][2] - m[2][0];
  } else {
    q[2] = 1.0 - tr + 2.0 * m[2][2]; q[0] = m[0][2] + m[2][0]; q[1] = m[1][2] + m[2][1]; q[3] = m[1][0] - m[0][1];
  }
  const double qn = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  float qf[4];
#pragma unroll
  for (int i = 0; i < 4; i++) qf[i] = (float)(q[i] / qn);
  const float fn = sqrtf(qf[0] * qf[0] + qf[1] * qf[1] + qf[2] * qf[2] + qf[3] * qf[3]);
#pragma unroll
  for (int i = 0; i < 4; i++) qf[i] = qf[i] / fn;
  if (qf[3] < 0.f) {
#pragma unroll
    for (int i = 0; i < 4; i++) qf[i] = -qf[i];
  }
  // fp64 again: extrinsic xyz Euler angles in degrees, + 180, in bins of rot_res, half to even, the last bin is the first
  double x = qf[0], y = qf[1], z = qf[2], w = qf[3];
  const double dn = sqrt(x * x + y * y + z * z + w * w);
  x /= dn; y /= dn; z /= dn; w /= dn;
  const double RAD2DEG = 57.295779513082320876798154814105;
  double sp = 2.0 * (w * y - z * x);
  sp = sp > 1.0 ? 1.0 : (sp < -1.0 ? -1.0 : sp);
  const double e[3] = {atan2(2.0 * (w * x + y * z), 1.0 - 2.0 * (x * x + y * y)) * RAD2DEG + 180.0, asin(sp) * RAD2DEG + 180.0,
                       atan2(2.0 * (w * z + x * y), 1.0 - 2.0 * (y * y + z * z)) * RAD2DEG + 180.0};
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const long long bin = (long long)rint(e[i] / p.rot_res);
    c.rot[i] = bin == (long long)p.rot_bins ? 0 : bin;
  }
}

__device__ __forceinline__ long long se3_action(const void* base, int i64, int64_t idx) {
  return i64 ? reinterpret_cast<const long long*>(base)[idx] : (long long)reinterpret_cast<const int*>(base)[idx];
}

__global__ void __launch_bounds__(SE3_WG) se3_select_kernel(Se3K p) {
  __shared__ int bad[MGS_SE3_MAX_ATTEMPTS];       // attempt a has an invalid sample
  __shared__ int first[MGS_SE3_MAX_BATCH];        // sample b's first valid attempt (A: none)
  __shared__ float red[6][SE3_WG];                // partial min / max of the bounds
  __shared__ float ext[6];
  const int tid = threadIdx.x;
  Philox ph = {};
  if (!p.draws) ph = philox_init(p.rng);
  for (int a = tid; a < p.A; a += SE3_WG) bad[a] = 0;
  for (int b = tid; b < p.B; b += SE3_WG) first[b] = p.A;
  // the extremes of the bounds over the whole batch (the reference clamps every sample's target to them)
  {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int r = tid; r < p.bounds_rows; r += SE3_WG) {
#pragma unroll
      for (int i = 0; i < 3; i++) {
        lo[i] = fminf(lo[i], p.bounds[(int64_t)r * 6 + i]);
        hi[i] = fmaxf(hi[i], p.bounds[(int64_t)r * 6 + 3 + i]);
      }
    }
#pragma unroll
    for (int i = 0; i < 3; i++) { red[i][tid] = lo[i]; red[3 + i][tid] = hi[i]; }
  }
  __syncthreads();
  if (tid < 6) {
    float v = red[tid][0];
    for (int t = 1; t < SE3_WG; t++) v = tid < 3 ? fminf(v, red[tid][t]) : fmaxf(v, red[tid][t]);
    ext[tid] = v;
  }
  // every candidate's validity (LDS integer atomics: the results do not depend on their order)
  const int total = p.A * p.B;
  for (int c = tid; c < total; c += SE3_WG) {
    const int a = c / p.B, b = c - a * p.B;
    Se3Cand cand;
    se3_candidate(p, ph, a, b, cand);
    if (cand.valid) atomicMin(&first[b], a);
    else atomicOr(&bad[a], 1);
  }
  __syncthreads();
  int batch_a = -1;
  for (int a = p.A - 1; a >= 0; a--)
    if (!bad[a]) batch_a = a;
  if (tid == 0) p.info[0] = batch_a;
  for (int b = tid; b < p.B; b += SE3_WG) {
    const int a = p.retry == 0 ? batch_a : (first[b] < p.A ? first[b] : -1);
    p.info[1 + b] = a;
    float* __restrict__ rec = p.rec + (int64_t)b * SE3_REC;
    if (a < 0) {
#pragma unroll
      for (int i = 0; i < 3; i++) p.out_trans[(int64_t)b * 3 + i] = se3_action(p.act_trans, p.action_i64, (int64_t)b * 3 + i);
#pragma unroll
      for (int i = 0; i < 4; i++) p.out_rot[(int64_t)b * 4 + i] = se3_action(p.act_rot, p.action_i64, (int64_t)b * 4 + i);
#pragma unroll
      for (int i = 0; i < SE3_REC; i++) rec[i] = (i == 0 || i == 4 || i == 8) ? 1.f : 0.f;
      rec[15] = 0.f;
      continue;
    }
    Se3Cand cand;
    se3_candidate(p, ph, a, b, cand);
#pragma unroll
    for (int i = 0; i < 3; i++) {
      p.out_trans[(int64_t)b * 3 + i] = cand.trans[i];
      p.out_rot[(int64_t)b * 4 + i] = cand.rot[i];
      rec[9 + i] = cand.pivot[i];
      rec[12 + i] = fminf(fmaxf(cand.pivot[i] + cand.shift[i], ext[i]), ext[3 + i]);
    }
    p.out_rot[(int64_t)b * 4 + 3] = se3_action(p.act_rot, p.action_i64, (int64_t)b * 4 + 3);
#pragma unroll
    for (int i = 0; i < 9; i++) rec[i] = cand.S[i];
    rec[15] = 1.f;
  }
}

__global__ void __launch_bounds__(SE3_WG) se3_draws_kernel(Se3K p, float* __restrict__ out) {
  const int c = blockIdx.x * SE3_WG + threadIdx.x;
  if (c >= p.A * p.B) return;
  const Philox ph = philox_init(p.rng);
  const int a = c / p.B, b = c - a * p.B;
  float d[6];
  se3_generate(ph, p.k, a, b, d);
#pragma unroll
  for (int i = 0; i < 6; i++) out[(int64_t)c * 6 + i] = d[i];
}

// grid (point blocks + 1, B, sources): block column gridDim.x - 1 of (b, s) transforms pose s of sample b
__global__ void __launch_bounds__(SE3_WG) se3_apply_kernel(Se3Apply p) {
  const int b = blockIdx.y, s = blockIdx.z, tid = threadIdx.x;
  const float* __restrict__ rec = p.rec + (int64_t)b * SE3_REC;
  float S[9], pv[3], tg[3];
#pragma unroll
  for (int i = 0; i < 9; i++) S[i] = rec[i];
#pragma unroll
  for (int i = 0; i < 3; i++) { pv[i] = rec[9 + i]; tg[i] = rec[12 + i]; }
  const bool identity = rec[15] == 0.f;
  if (blockIdx.x == gridDim.x - 1) {
    if (s >= p.n_pose || tid >= 16) return;
    const float* __restrict__ in = p.pose_in[s] + (int64_t)b * 16;
    const int i = tid >> 2, j = tid & 3;
    float v = in[tid];
    if (!identity && i < 3) {
      if (j < 3) {  // (S^T R)[i][j]
        v = fmaf(in[8 + j], S[6 + i], fmaf(in[4 + j], S[3 + i], in[j] * S[i]));
      } else {      // S^T (T - pivot) + target
        const float d0 = in[3] - pv[0], d1 = in[7] - pv[1], d2 = in[11] - pv[2];
        v = fmaf(d2, S[6 + i], fmaf(d1, S[3 + i], d0 * S[i])) + tg[i];
      }
    }
    p.pose_out[s][(int64_t)b * 16 + tid] = v;
    return;
  }
  if (s >= p.n_src) return;
  const int n = p.n[s], pt = blockIdx.x * SE3_WG + tid;
  if (pt >= n) return;
  const float* __restrict__ in = p.src[s] + (int64_t)b * p.sb[s] + pt;
  float* __restrict__ out = p.dst[s] + (int64_t)b * 3 * n + pt;
  const float x = in[0], y = in[p.sc[s]], z = in[2 * p.sc[s]];
  if (identity) {
    out[0] = x; out[n] = y; out[2 * (int64_t)n] = z;
    return;
  }
  const float d0 = x - pv[0], d1 = y - pv[1], d2 = z - pv[2];
#pragma unroll
  for (int j = 0; j < 3; j++) out[(int64_t)j * n] = fmaf(d2, S[6 + j], fmaf(d1, S[3 + j], d0 * S[j])) + tg[j];
}

static int se3_check(const char* fn, const MgsSe3Args* a, bool need_pose) {
  if (!a) { set_error("%s: NULL arguments", fn); return MGS_ERR_INVALID_ARG; }
  if (a->B < 1 || a->B > MGS_SE3_MAX_BATCH || a->attempts < 1 || a->attempts > MGS_SE3_MAX_ATTEMPTS) {
    set_error("%s: B = %d, attempts = %d (1 <= B <= %d, 1 <= attempts <= %d)", fn, a->B, a->attempts, MGS_SE3_MAX_BATCH,
              MGS_SE3_MAX_ATTEMPTS);
    return MGS_ERR_INVALID_ARG;
  }
  if (a->rot_steps[0] < 0 || a->rot_steps[1] < 0 || a->rot_steps[2] < 0 || a->rot_steps[0] > (1 << 20) ||
      a->rot_steps[1] > (1 << 20) || a->rot_steps[2] > (1 << 20)) {
    set_error("%s: rot_steps = (%d, %d, %d) (each 0 .. 2^20)", fn, a->rot_steps[0], a->rot_steps[1], a->rot_steps[2]);
    return MGS_ERR_INVALID_ARG;
  }
  if (!need_pose) return MGS_OK;
  if (a->voxel_size < 1 || (a->bounds_rows != 1 && a->bounds_rows != a->B) || (a->retry != 0 && a->retry != 1) ||
      !(a->rot_resolution > 0.0)) {
    set_error("%s: voxel_size = %d, bounds_rows = %d for B = %d, retry = %d, rot_resolution = %g (voxel_size >= 1, bounds_rows "
              "1 or B, retry 0 or 1, rot_resolution > 0)", fn, a->voxel_size, a->bounds_rows, a->B, a->retry, a->rot_resolution);
    return MGS_ERR_INVALID_ARG;
  }
  if (!a->gripper_pose || !a->action_trans || !a->action_rot_grip || !a->bounds) {
    set_error("%s: NULL gripper_pose, action_trans, action_rot_grip or bounds", fn);
    return MGS_ERR_INVALID_ARG;
  }
  return MGS_OK;
}

static int se3_check_rng(const char* fn, const MgsSe3Args* a, bool table_allowed) {
  if (table_allowed && a->draws) return MGS_OK;
  if (!a->rng_state || (reinterpret_cast<uintptr_t>(a->rng_state) & 7u)) {
    set_error("%s: needs %srng_state, 8-byte aligned", fn, table_allowed ? "draws or " : "");
    return MGS_ERR_INVALID_ARG;
  }
  return MGS_OK;
}

static Se3K se3_args(const MgsSe3Args* a) {
  Se3K k = {};
  k.B = a->B; k.A = a->attempts; k.retry = a->retry; k.layer = a->layer; k.V = a->voxel_size; k.bounds_rows = a->bounds_rows;
  k.rot_bins = a->rot_bins; k.trans_f64 = a->trans_f64; k.action_i64 = a->action_i64;
  for (int i = 0; i < 3; i++) { k.k[i] = a->rot_steps[i]; k.tar[i] = a->trans_aug_range[i]; }
  k.step_rad = a->rot_step_rad; k.rot_res = a->rot_resolution;
  k.pose = a->gripper_pose; k.act_trans = a->action_trans; k.act_rot = a->action_rot_grip; k.bounds = a->bounds;
  k.rng = reinterpret_cast<const unsigned long long*>(a->rng_state);
  k.draws = a->draws;
  return k;
}

}  // namespace mgs

using namespace mgs;

extern "C" {

size_t mgs_se3_workspace_bytes(int B) {
  if (B < 1 || B > MGS_SE3_MAX_BATCH) return 0;
  return align_up((size_t)B * SE3_REC * sizeof(float)) + ALIGN;
}

int mgs_se3_select(const MgsSe3Args* a, int64_t* out_trans, int64_t* out_rot_grip, int32_t* info, void* workspace,
                   size_t workspace_bytes, mgs_stream_t stream) {
  const char* fn = "se3_select";
  int rc = se3_check(fn, a, true);
  if (rc == MGS_OK) rc = se3_check_rng(fn, a, true);
  if (rc != MGS_OK) return rc;
  if (!out_trans || !out_rot_grip || !info || !workspace || misaligned16(workspace) ||
      (reinterpret_cast<uintptr_t>(out_trans) & 7u) || (reinterpret_cast<uintptr_t>(out_rot_grip) & 7u)) {
    set_error("%s: out_trans, out_rot_grip (8-byte aligned), info and the workspace (16-byte aligned) must be given", fn);
    return MGS_ERR_INVALID_ARG;
  }
  if (int rc = workspace_short(fn, workspace_bytes, mgs_se3_workspace_bytes(a->B))) return rc;
  Se3K k = se3_args(a);
  k.out_trans = reinterpret_cast<long long*>(out_trans);
  k.out_rot = reinterpret_cast<long long*>(out_rot_grip);
  k.info = info;
  k.rec = reinterpret_cast<float*>(workspace);
  hipLaunchKernelGGL(se3_select_kernel, dim3(1), dim3(SE3_WG), 0, (hipStream_t)stream, k);
  return launch_done(fn);
}

int mgs_se3_apply(const MgsSe3Args* a, const void* workspace, size_t workspace_bytes, mgs_stream_t stream) {
  const char* fn = "se3_apply";
  if (!a) { set_error("%s: NULL arguments", fn); return MGS_ERR_INVALID_ARG; }
  if (a->B < 1 || a->B > MGS_SE3_MAX_BATCH || a->n_sources < 0 || a->n_sources > MGS_SE3_MAX_SOURCES || a->n_poses < 0 ||
      a->n_poses > MGS_SE3_MAX_SOURCES) {
    set_error("%s: B = %d, %d sources, %d poses (1 <= B <= %d, 0 .. %d sources and poses)", fn, a->B, a->n_sources, a->n_poses,
              MGS_SE3_MAX_BATCH, MGS_SE3_MAX_SOURCES);
    return MGS_ERR_INVALID_ARG;
  }
  if (!workspace || misaligned16(workspace)) { set_error("%s: the workspace must be given, 16-byte aligned", fn); return MGS_ERR_INVALID_ARG; }
  if (int rc = workspace_short(fn, workspace_bytes, mgs_se3_workspace_bytes(a->B))) return rc;
  Se3Apply k = {};
  k.B = a->B; k.n_src = a->n_sources; k.n_pose = a->n_poses;
  k.rec = reinterpret_cast<const float*>(workspace);
  int64_t most = 0;
  for (int i = 0; i < a->n_sources; i++) {
    const int64_t n = a->n_points[i];
    if (!a->src[i] || !a->dst[i] || a->src[i] == a->dst[i]) { set_error("%s: source %d is NULL or written in place", fn, i); return MGS_ERR_INVALID_ARG; }
    if (n < 1 || n > ((int64_t)1 << 24) || a->stride_c[i] < n || a->stride_b[i] < 0) {
      set_error("%s: source %d has %lld points, plane stride %lld, sample stride %lld (1 .. 2^24 points, planes that do not "
                "overlap, a sample stride >= 0)", fn, i, (long long)n, (long long)a->stride_c[i], (long long)a->stride_b[i]);
      return MGS_ERR_INVALID_ARG;
    }
    k.src[i] = a->src[i]; k.dst[i] = a->dst[i]; k.n[i] = (int)n; k.sb[i] = a->stride_b[i]; k.sc[i] = a->stride_c[i];
    most = n > most ? n : most;
  }
  for (int i = 0; i < a->n_poses; i++) {
    if (!a->pose_in[i] || !a->pose_out[i] || a->pose_in[i] == a->pose_out[i]) {
      set_error("%s: pose %d is NULL or written in place", fn, i);
      return MGS_ERR_INVALID_ARG;
    }
    k.pose_in[i] = a->pose_in[i]; k.pose_out[i] = a->pose_out[i];
  }
  const int layers = a->n_sources > a->n_poses ? a->n_sources : a->n_poses;
  if (layers == 0) return MGS_OK;
  const unsigned blocks = (unsigned)((most + SE3_WG - 1) / SE3_WG) + 1;  // (+ 1: the pose column)
  hipLaunchKernelGGL(se3_apply_kernel, dim3(blocks, (unsigned)a->B, (unsigned)layers), dim3(SE3_WG), 0, (hipStream_t)stream, k);
  return launch_done(fn);
}

int mgs_se3_draws(const MgsSe3Args* a, float* draws, mgs_stream_t stream) {
  const char* fn = "se3_draws";
  int rc = se3_check(fn, a, false);
  if (rc == MGS_OK) rc = se3_check_rng(fn, a, false);
  if (rc != MGS_OK) return rc;
  if (!draws) { set_error("%s: NULL draws", fn); return MGS_ERR_INVALID_ARG; }
  const Se3K k = se3_args(a);
  const int total = a->attempts * a->B;
  hipLaunchKernelGGL(se3_draws_kernel, dim3((total + SE3_WG - 1) / SE3_WG), dim3(SE3_WG), 0, (hipStream_t)stream, k, draws);
  return launch_done(fn);
}

}  // extern "C"
