// mgs_voxelize.hip -- the agent's voxel grid: scatter-mean of a point cloud into V^3 voxels, deterministic, in four launches.
// Reference: voxel/voxel_grid.py:168-229 (VoxelGrid.coords_to_bounding_voxel_grid: floor((p - (min - res)) / (res + 1e-12))
// clamped to [0, V + 1], scatter_add_ of [features | xyz | 1] into a (V + 2)^3 grid, divide by the count, crop one voxel from
// every face, append index / V and the occupancy).  The reference's GPU grid depends on the order its float atomics land in;
// here every voxel's points are added in ascending point index from 0.0f and divided once -- the order of the reference's CPU
// scatter_add_ -- so the grid is the same bits from run to run and the same bits as the reference module on a CPU.
//   voxelize_clear_kernel   zeroes the int32 head grid [B V^3]
//   voxelize_link_kernel    one thread per point: the index arithmetic (every step its own fp32 operation, the divisions
//                           correctly rounded); a point of the cropped shell (index 0 or V + 1: outside, NaN, +-inf) is dropped
//                           here; a kept point pushes itself on its voxel's list: next[p] = atomicExch(head[voxel], p + 1)
//   voxelize_mean_kernel    a list's head point (the one that pushed last) walks it.  Up to VOX_SHORT points: sorted in
//                           registers, added in that order, divided.  More: the whole wave sums it -- it scans the batch
//                           item's voxel ids in point order, lane c adds channel c of every match.  Either way the means go
//                           to the head point's row of a table [B N][stride].  Any multiplicity, all N in one voxel included
//   voxelize_write_*_kernel every output float exactly once, 16 bytes per store: background (0, index / V, 0) or, for an occupied
//                           voxel, head -> the row of its means
// Integer atomics order nothing that reaches the result: a list's order is discarded by the sort or never used, and which of
// its points heads a list only decides the row its means pass through.  No float atomics, no host read, no allocation:
// capturable into a HIP graph as it is.
#include "mgs_common.h"
#include "mgs_device.h"

#pragma clang fp contract(off)  // nothing here may become an FMA: the index arithmetic and the sums are the reference's, op by op

namespace mgs {

constexpr int VOX_WG = 256;
constexpr int VOX_SHORT = 8;          // lists up to this length are sorted and summed in registers by their head point's thread
constexpr int VOX_BLOCK = 8;          // channels a head thread sums at a time (their loads are independent: one wait per block)
constexpr int VOX_ROW_MAX = 68;       // floats the workspace keeps per point for the means: Fc + 3 <= 67, padded to 16 bytes
constexpr int VOX_MAX_SRC = MGS_VOXELIZE_MAX_SOURCES;

// Where point p of batch item b keeps channel j: source p / per_src (one flat array, or one image per camera), element
// b * sb + (p % per_src) * sp + j * sc of it.  [B,N,3]: sp = 3, sc = 1, sb = 3 N.  [B,3,H,W] images: sp = 1, sc = HW, sb = 3 HW.
struct VoxInput {
  const float* src[VOX_MAX_SRC];
  int64_t sp, sc, sb;
};

struct VoxArgs {
  int B, N, V, Fc, V3, per_src, stride;  // stride: floats per row of `mean`, Fc + 3 rounded up to 4
  VoxInput coords, feats;
  const float* bounds;  // device [B,6]
  float* grid;
  int* head;            // [B V3]  0: empty, p + 1: the point (inside its batch item) that pushed last
  int* vid;             // [B N]   voxel of the point inside its batch item, -1: dropped
  int* next;            // [B N]   p + 1 of the next point of the list, 0: end
  float* mean;          // [B N][stride]  row b N + p: the means of the voxel whose list point p heads
};

__device__ __forceinline__ float vox_ld(const VoxInput& in, int per_src, int b, int p, int j) {
  const int s = p / per_src, q = p - s * per_src;
  return in.src[s][(int64_t)b * in.sb + (int64_t)q * in.sp + (int64_t)j * in.sc];
}

// channel c of [features | xyz] of a point
__device__ __forceinline__ float vox_val(const VoxArgs& a, int b, int p, int c) {
  return c < a.Fc ? vox_ld(a.feats, a.per_src, b, p, c) : vox_ld(a.coords, a.per_src, b, p, c - a.Fc);
}

__global__ void __launch_bounds__(VOX_WG) voxelize_clear_kernel(int4* __restrict__ p, int n4) {
  const int i = blockIdx.x * VOX_WG + threadIdx.x;
  if (i < n4) p[i] = make_int4(0, 0, 0, 0);
}

// voxel_grid.py:170-183 for one axis; the index as a float (NaN stays NaN and fails both comparisons of the caller)
__device__ __forceinline__ float vox_axis_index(float x, float mn, float mx, float v) {
  const float res = (mx - mn) / (v + 1e-12f);
  const float den = res + 1e-12f;
  const float shift = mn - res;
  return floorf((x - shift) / den);
}

__global__ void __launch_bounds__(VOX_WG) voxelize_link_kernel(VoxArgs a) {
  const int i = blockIdx.x * VOX_WG + threadIdx.x;
  if (i >= a.B * a.N) return;
  const int b = i / a.N, p = i - b * a.N;
  const float* __restrict__ bd = a.bounds + 6 * b;
  const float v = (float)a.V;
  int lin = 0;
  bool keep = true;
#pragma unroll
  for (int ax = 0; ax < 3; ax++) {
    const float f = vox_axis_index(vox_ld(a.coords, a.per_src, b, p, ax), bd[ax], bd[3 + ax], v);
    keep = keep && f >= 1.0f && f <= v;  // 0 and V + 1 are the shell the reference crops; NaN, +-inf and 1e30 end there too
    lin = lin * a.V + ((int)fminf(fmaxf(f, 1.0f), v) - 1);
  }
  a.vid[i] = keep ? lin : -1;
  if (keep) a.next[i] = atomicExch(&a.head[(int64_t)b * a.V3 + lin], p + 1);
}

// The list of a voxel, summed by the thread of its head point (head[voxel] == p + 1: exactly one point of every list).
__global__ void __launch_bounds__(VOX_WG) voxelize_mean_kernel(VoxArgs a) {
  const int i = blockIdx.x * VOX_WG + threadIdx.x;
  const int lane = threadIdx.x & (WAVE - 1);
  const int Cm = a.Fc + 3;
  int b = 0, lin = -1;
  bool is_long = false;
  if (i < a.B * a.N) {
    b = i / a.N;
    const int p = i - b * a.N;
    lin = a.vid[i];
    if (lin >= 0 && a.head[(int64_t)b * a.V3 + lin] == p + 1) {
      const int* __restrict__ next = a.next + (int64_t)b * a.N;
      int id[VOX_SHORT];
      int k = 0, q = p + 1;
#pragma unroll
      for (int t = 0; t < VOX_SHORT; t++) {
        id[t] = 0x7fffffff;  // unused slots sort to the end
        if (q > 0) { id[t] = q - 1; q = next[q - 1]; k++; }
      }
      is_long = q > 0;
      if (!is_long) {
        if (k > 1) {
#pragma unroll
          for (int r = 0; r < VOX_SHORT; r++) {  // odd-even transposition sort: a fixed network, the array stays in registers
#pragma unroll
            for (int t = r & 1; t + 1 < VOX_SHORT; t += 2) {
              const int lo = min(id[t], id[t + 1]), hi = max(id[t], id[t + 1]);
              id[t] = lo; id[t + 1] = hi;
            }
          }
        }
        const float n = (float)k;
        float* __restrict__ row = a.mean + (int64_t)i * a.stride;
        for (int c0 = 0; c0 < Cm; c0 += VOX_BLOCK) {
          float acc[VOX_BLOCK];
#pragma unroll
          for (int u = 0; u < VOX_BLOCK; u++) acc[u] = 0.0f;
#pragma unroll
          for (int t = 0; t < VOX_SHORT; t++) {  // ascending point index
            if (t < k) {
#pragma unroll
              for (int u = 0; u < VOX_BLOCK; u++)
                if (c0 + u < Cm) acc[u] += vox_val(a, b, id[t], c0 + u);
            }
          }
#pragma unroll
          for (int u = 0; u < VOX_BLOCK; u++)
            if (c0 + u < Cm) row[c0 + u] = acc[u] / n;
        }
      }
    }
  }
  unsigned long long todo = __ballot(is_long);
  while (todo) {
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const int lb = __shfl(b, src, WAVE), lv = __shfl(lin, src, WAVE), li = __shfl(i, src, WAVE);
    const int* __restrict__ vid = a.vid + (int64_t)lb * a.N;
    float s0 = 0.0f, s1 = 0.0f;  // channels lane and lane + 64
    int cnt = 0;
    for (int base = 0; base < a.N; base += WAVE) {
      const int q = base + lane;
      unsigned long long m = __ballot(q < a.N && vid[q] == lv);
      while (m) {  // ascending point index
        const int pp = base + __ffsll((long long)m) - 1;
        m &= m - 1;
        cnt++;
        if (lane < Cm) s0 += vox_val(a, lb, pp, lane);
        if (lane + WAVE < Cm) s1 += vox_val(a, lb, pp, lane + WAVE);
      }
    }
    const float n = (float)cnt;
    float* __restrict__ row = a.mean + (int64_t)li * a.stride;
    if (lane < Cm) row[lane] = s0 / n;
    if (lane + WAVE < Cm) row[lane + WAVE] = s1 / n;
  }
}

// One output float: channel c of voxel lin of batch item b, whose head entry is h.
__device__ __forceinline__ float vox_out(const VoxArgs& a, int b, int lin, int h, int c) {
  const int Cm = a.Fc + 3;
  if (c < Cm) return h != 0 ? a.mean[((int64_t)b * a.N + (h - 1)) * a.stride + c] : 0.0f;
  if (c == Cm + 3) return h != 0 ? 1.0f : 0.0f;
  // channels Fc + 3 .. Fc + 5: the voxel's x, y, z index over V (voxel_grid.py:219-221)
  const int i = c == Cm ? lin / (a.V * a.V) : c == Cm + 1 ? (lin / a.V) % a.V : lin % a.V;
  return (float)i / (float)a.V;
}

// Channels-first [B,C,V,V,V]: one thread per four consecutive voxels of one channel plane of a batch item; a workgroup stays
// inside one plane (`per_plane` workgroups each), so the plane, the item and the channel are scalars.
__global__ void __launch_bounds__(VOX_WG) voxelize_write_cf_kernel(VoxArgs a, int groups, unsigned per_plane) {
  const int C = a.Fc + 7;
  const int plane = (int)(blockIdx.x / per_plane);
  const int g = (int)(blockIdx.x - (unsigned)plane * per_plane) * VOX_WG + threadIdx.x;
  if (g >= groups) return;
  const int lin0 = 4 * g;
  const int b = plane / C, c = plane - b * C;
  const bool vec = (a.V3 & 3) == 0;  // then every plane and every group starts on 16 bytes
  const int* __restrict__ head = a.head + (int64_t)b * a.V3;
  int h[4];
  if (vec) {
    const int4 q = *reinterpret_cast<const int4*>(head + lin0);
    h[0] = q.x; h[1] = q.y; h[2] = q.z; h[3] = q.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++) h[j] = lin0 + j < a.V3 ? head[lin0 + j] : 0;
  }
  float o[4];
#pragma unroll
  for (int j = 0; j < 4; j++) o[j] = vox_out(a, b, lin0 + j, h[j], c);
  float* __restrict__ dst = a.grid + (int64_t)plane * a.V3 + lin0;
  if (vec) {
    *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (lin0 + j < a.V3) dst[j] = o[j];
  }
}

// Channels-last [B,V,V,V,C] (the reference's layout): one thread per 16 bytes of the output, whatever voxels they belong to.
__global__ void __launch_bounds__(VOX_WG) voxelize_write_cl_kernel(VoxArgs a, int64_t total) {
  const int64_t e0 = 4 * ((int64_t)blockIdx.x * VOX_WG + threadIdx.x);
  if (e0 >= total) return;
  const int C = a.Fc + 7;
  const int vox0 = (int)(e0 / C), c0 = (int)(e0 - (int64_t)vox0 * C);  // (B V^3 < 2^31)
  float o[4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    int vox = vox0, c = c0 + j;
    if (c >= C) { c -= C; vox++; }  // C >= 7: at most one voxel further
    if (e0 + j >= total) { vox = vox0; c = c0; }
    const int b = vox / a.V3, lin = vox - b * a.V3;
    o[j] = vox_out(a, b, lin, a.head[vox], c);
  }
  if (e0 + 4 <= total) {
    *reinterpret_cast<float4*>(a.grid + e0) = make_float4(o[0], o[1], o[2], o[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (e0 + j < total) a.grid[e0 + j] = o[j];
  }
}

struct VoxCarve {
  size_t head, vid, next, mean, total;
};

static VoxCarve vox_carve(int B, int64_t N, int V) {
  VoxCarve c;
  const size_t v3 = (size_t)V * V * V, bn = (size_t)B * (size_t)N;
  size_t off = 0;
  c.head = off; off = align_up(off + (size_t)B * v3 * 4);
  c.vid = off;  off = align_up(off + bn * 4);
  c.next = off; off = align_up(off + bn * 4);
  c.mean = off; off = align_up(off + bn * VOX_ROW_MAX * 4);  // (for any feature width: the size is a function of B, N, V)
  c.total = off;
  return c;
}

// B <= 65 536 items, B V^3 < 2^31 voxels, N <= 2^24 points per batch item (a float count is exact up to there, as the reference's is), B N < 2^31
static bool vox_sizes_ok(int B, int64_t N, int V) {
  if (B < 1 || B > 65536 || N < 0 || V < 1 || V > 1290) return false;
  if (N > ((int64_t)1 << 24)) return false;
  const int64_t v3 = (int64_t)V * V * V;
  return (int64_t)B * v3 < ((int64_t)1 << 31) - 16 && (int64_t)B * N < ((int64_t)1 << 31) - VOX_WG;
}

static int vox_run(const char* fn, int B, int64_t N, int V, int Fc, int channels_first, const VoxInput& coords,
                   const VoxInput& feats, int per_src, const float* bounds, float* grid, void* workspace,
                   size_t workspace_bytes, mgs_stream_t stream) {
  const VoxCarve cv = vox_carve(B, N, V);
  if (int rc = workspace_short(fn, workspace_bytes, cv.total)) return rc;
  char* ws = reinterpret_cast<char*>(workspace);
  VoxArgs a = {};
  a.B = B; a.N = (int)N; a.V = V; a.Fc = Fc; a.V3 = V * V * V; a.per_src = per_src > 0 ? per_src : 1;
  a.stride = (Fc + 3 + 3) & ~3;
  a.coords = coords; a.feats = feats; a.bounds = bounds; a.grid = grid;
  a.head = reinterpret_cast<int*>(ws + cv.head);
  a.vid = reinterpret_cast<int*>(ws + cv.vid);
  a.next = reinterpret_cast<int*>(ws + cv.next);
  a.mean = reinterpret_cast<float*>(ws + cv.mean);
  hipStream_t s = (hipStream_t)stream;
  const int n4 = (int)((cv.vid - cv.head) / 16);  // (the head grid and its padding)
  hipLaunchKernelGGL(voxelize_clear_kernel, dim3((n4 + VOX_WG - 1) / VOX_WG), dim3(VOX_WG), 0, s, reinterpret_cast<int4*>(ws), n4);
  const int64_t bn = (int64_t)B * N;
  if (bn > 0) {
    const unsigned blocks = (unsigned)((bn + VOX_WG - 1) / VOX_WG);
    hipLaunchKernelGGL(voxelize_link_kernel, dim3(blocks), dim3(VOX_WG), 0, s, a);
    hipLaunchKernelGGL(voxelize_mean_kernel, dim3(blocks), dim3(VOX_WG), 0, s, a);
  }
  if (channels_first) {
    const int groups = (a.V3 + 3) / 4;
    const unsigned per_plane = (unsigned)((groups + VOX_WG - 1) / VOX_WG);  // B C per_plane <= 71 (2^31 / 1024 + B) with B <= 65 536: below 2^32
    hipLaunchKernelGGL(voxelize_write_cf_kernel, dim3((unsigned)(B * (Fc + 7)) * per_plane), dim3(VOX_WG), 0, s, a, groups,
                       per_plane);
  } else {
    const int64_t total = (int64_t)B * a.V3 * (Fc + 7), threads = (total + 3) / 4;
    hipLaunchKernelGGL(voxelize_write_cl_kernel, dim3((unsigned)((threads + VOX_WG - 1) / VOX_WG)), dim3(VOX_WG), 0, s, a, total);
  }
  return launch_done(fn);
}

static int vox_check(const char* fn, int B, int64_t N, int V, int Fc, const float* bounds, const float* grid, const void* workspace) {
  if (!vox_sizes_ok(B, N, V)) {
    set_error("%s: B = %d, N = %lld, V = %d (1 <= B <= 65536, 0 <= N <= 2^24, V >= 1, B V^3 and B N below 2^31)", fn, B, (long long)N, V);
    return MGS_ERR_INVALID_ARG;
  }
  if (Fc < 0 || Fc > MGS_VOXELIZE_MAX_FEATURES) {
    set_error("%s: feature width %d (0 .. %d)", fn, Fc, MGS_VOXELIZE_MAX_FEATURES);
    return MGS_ERR_INVALID_ARG;
  }
  if (!bounds || !grid || !workspace) {
    set_error("%s: NULL pointer", fn);
    return MGS_ERR_INVALID_ARG;
  }
  if ((reinterpret_cast<uintptr_t>(grid) | reinterpret_cast<uintptr_t>(workspace)) & 15u) {
    set_error("%s: the grid and the workspace must be 16-byte aligned", fn);
    return MGS_ERR_INVALID_ARG;
  }
  return MGS_OK;
}

}  // namespace mgs

using namespace mgs;

extern "C" {

size_t mgs_voxelize_workspace_bytes(int B, int64_t N, int V) {
  if (!vox_sizes_ok(B, N, V)) return 0;
  return vox_carve(B, N, V).total;
}

int mgs_voxelize_forward(int B, int64_t N, int V, int Fc, int channels_first, const float* coords, const float* features,
                         const float* bounds, float* grid, void* workspace, size_t workspace_bytes, mgs_stream_t stream) {
  const char* fn = "voxelize_forward";
  int rc = vox_check(fn, B, N, V, Fc, bounds, grid, workspace);
  if (rc != MGS_OK) return rc;
  if ((N > 0 && !coords) || (N > 0 && Fc > 0 && !features) || (Fc == 0 && features)) {
    set_error("%s: coords NULL, or features NULL with Fc > 0, or features given with Fc = 0", fn);
    return MGS_ERR_INVALID_ARG;
  }
  VoxInput c = {}, f = {};
  c.src[0] = coords; c.sp = 3; c.sc = 1; c.sb = 3 * N;
  f.src[0] = features; f.sp = Fc; f.sc = 1; f.sb = (int64_t)Fc * N;
  return vox_run(fn, B, N, V, Fc, channels_first, c, f, N > 0 ? (int)N : 1, bounds, grid, workspace, workspace_bytes, stream);
}

int mgs_voxelize_forward_images(int B, int n_images, int64_t HW, int V, int Fc, int channels_first, const float* const* coords,
                                const float* const* features, const float* bounds, float* grid, void* workspace,
                                size_t workspace_bytes, mgs_stream_t stream) {
  const char* fn = "voxelize_forward_images";
  if (n_images < 1 || n_images > VOX_MAX_SRC || HW < 1 || HW > ((int64_t)1 << 24)) {
    set_error("%s: %d images of %lld pixels (1 .. %d images, 1 .. 2^24 pixels)", fn, n_images, (long long)HW, VOX_MAX_SRC);
    return MGS_ERR_INVALID_ARG;
  }
  const int64_t N = (int64_t)n_images * HW;
  int rc = vox_check(fn, B, N, V, Fc, bounds, grid, workspace);
  if (rc != MGS_OK) return rc;
  if (!coords || (Fc > 0 && !features)) {
    set_error("%s: NULL pointer", fn);
    return MGS_ERR_INVALID_ARG;
  }
  VoxInput c = {}, f = {};
  for (int i = 0; i < n_images; i++) {
    c.src[i] = coords[i];
    f.src[i] = Fc > 0 ? features[i] : nullptr;
    if (!c.src[i] || (Fc > 0 && !f.src[i])) {
      set_error("%s: image %d is NULL", fn, i);
      return MGS_ERR_INVALID_ARG;
    }
  }
  c.sp = 1; c.sc = HW; c.sb = 3 * HW;
  f.sp = 1; f.sc = HW; f.sb = (int64_t)Fc * HW;
  return vox_run(fn, B, N, V, Fc, channels_first, c, f, (int)HW, bounds, grid, workspace, workspace_bytes, stream);
}

}  // extern "C"
