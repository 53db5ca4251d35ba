// mgs_records.hip -- the partial records of a weight | bias gradient, shared by the four Conv3d families (mgs_conv3d.hip,
// mgs_pointwise.hip, mgs_narrow.hip, mgs_dense.hip).
//
// A family's tiles or segments, in their linear order, are cut into at most MAX_REC runs whose number and length depend on the shape
// alone (cut_runs).  The family's own kernel writes one RECORD [rows, cols] per run into the workspace; `split` is the number of
// workgroups that share the runs: it decides who computes a record, not what the record is.  The merge launch then sums the records
// in ascending order in double and rounds once: dw and db are the same bits for every split.  A record is written before it is read
// within one call (the merge follows the family's kernel on the same stream), so the workspace needs no zeroing and carries nothing
// from one call to the next.  tests/test_poisoned_memory.py holds the families to that: every split and every combination of requested
// gradients with the workspace and the results filled with 0xFF and with 0x7F bytes beforehand, against the bits of the clean run.
#include "mgs_common.h"

namespace mgs {

// records [nrec, rows, cols] -> dw [rows, wcols], db [rows] (either may be nullptr), in ascending order in double; total = rows cols
__global__ __launch_bounds__(256) void records_merge_kernel(uint32_t nrec, uint32_t cols, uint32_t wcols, uint32_t total,
                                                            const float* __restrict__ records, float* __restrict__ dw,
                                                            float* __restrict__ db) {
  const uint32_t e = blockIdx.x * 256u + threadIdx.x;
  if (e >= total) return;
  const uint32_t row = e / cols, c = e - row * cols;
  if (c < wcols ? dw == nullptr : db == nullptr) return;
  double s = 0.0;
  for (uint32_t r = 0; r < nrec; ++r) s += (double)records[(size_t)r * total + e];
  if (c < wcols) dw[(size_t)row * wcols + c] = (float)s;
  else db[row] = (float)s;
}

void launch_records_merge(int64_t nrec, int rows, int cols, int wcols, const float* records, float* dw, float* db, hipStream_t s) {
  const uint32_t total = (uint32_t)rows * (uint32_t)cols;
  hipLaunchKernelGGL(records_merge_kernel, dim3((total + 255u) / 256u), dim3(256), 0, s, (uint32_t)nrec, (uint32_t)cols, (uint32_t)wcols,
                     total, records, dw, db);
}

Runs cut_runs(int64_t items, int64_t most) {
  const int64_t want = items < most ? items : most;
  Runs r;
  r.per = (items + want - 1) / want;
  r.n = (items + r.per - 1) / r.per;
  return r;
}

int split_check(const char* fn, int split) {
  if (split >= 0 && split <= MAX_REC) return MGS_OK;
  set_error("%s: split = %d (0: chosen by the library, at most %d)", fn, split, MAX_REC);
  return MGS_ERR_INVALID_ARG;
}

int64_t split_clamp(int split, int64_t dflt, int64_t nrec) {
  const int64_t wgs = split ? split : dflt;
  return wgs > nrec ? nrec : wgs;
}

bool row_too_long(int64_t d, int64_t h, int64_t w) {
  const int64_t lim = 0x7fffffff;
  return d > lim || h > lim || w > lim || d * h > lim || d * h * w > lim;
}

int records_workspace(const char* fn, const void* workspace, size_t have, size_t need) {
  if (!workspace || misaligned16(workspace)) { set_error("%s: NULL or misaligned workspace", fn); return MGS_ERR_INVALID_ARG; }
  return workspace_short(fn, have, need);
}

}  // namespace mgs
