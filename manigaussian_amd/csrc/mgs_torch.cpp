// mgs_torch.cpp -- the COMPILED binding of the rasterizer's autograd path: manigaussian_amd/_mgs_torch.so.
//
// What the reference's own binding is (RAST/rasterize_points.cu:35-128 RasterizeGaussiansCUDA, :130-225
// RasterizeGaussiansBackwardCUDA; RAST = third_party/gaussian-splatting/submodules/diff-gaussian-rasterization): compiled code
// that takes torch tensors, allocates outputs and workspaces, and calls the rasterizer.  Rounds 1-4 did that job in Python over
// ctypes (manigaussian_amd/_C.py) at 125-133 us of host time per forward + backward -- as much as the 150 us of GPU work, so
// ManiGaussian's eager caller (MG/neural_rendering.py:283,324 -> MG/gaussian_renderer/__init__.py:74) was host-bound.  This file
// is the same job in C++ over the SAME C ABI (include/mgsplat.h; no kernel, no HIP code here): argument marshalling, ONE
// workspace arena and a torch::autograd::Node whose backward the autograd engine calls without entering Python.  _C.py stays: it
// is the raw three-function surface of the reference's `_C` module, the multi-view path, HIP-graph capture, debug /
// prefiltered calls and the fallback when this module is not built.  The status slots, the workspace marks, the outstanding
// reports, the budget and every message of the protocol are the library's (csrc/mgs_ledger.hip, "the report ledger" of
// include/mgsplat.h): this file and _C.py ask the same store.
//
// Host-side protocol (manigaussian_amd/_state.py documents the modes at length):
//   mode safe   shapes whose worst-case workspace fits the budget: enqueue and return (cannot overflow).  Every other shape:
//               workspace from the shape's marks, everything enqueued, then wait for the PREPROCESS's report only (status
//               words 0 and 2); too small -> bin + render again with room (what RAST/cuda_rasterizer/rasterizer_impl.cu:282-289
//               does by blocking on a cudaMemcpy -- here binning and render are already running while the call returns).
//   mode async  workspace from the marks x head-room, nothing waited for; overflow repaired at backward entry or raised late.
//   mode blocking, debug, prefiltered, graph capture, padded feature widths, non-contiguous inputs: not handled here (None).
#include <Python.h>
#include <torch/extension.h>
#include <torch/csrc/autograd/function.h>
#include <torch/csrc/autograd/functions/utils.h>
#include <torch/csrc/autograd/saved_variable.h>
#include <torch/csrc/autograd/variable.h>
#include <c10/hip/HIPGuard.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/mgsplat.h"

namespace py = pybind11;
using torch::autograd::Node;
using torch::autograd::SavedVariable;
using torch::autograd::variable_list;

namespace {

constexpr int NSLOTS = 1024;  // status slots of a ring this binding gives a device (MGS_LEDGER_SLOT_WORDS 64-bit words each)

// What is this binding's alone: the switch, and the per-call options every forward carries.  Mode, overflow policy, head-room
// and budget are the ledger's configuration (mgs_ledger_get_config).
struct Config {
  std::atomic<bool> enabled{true};
  MgsOptions opt;       // (manigaussian_amd._lib.DEFAULT_OPTIONS)
  std::mutex mu;
};
Config& cfg() { static Config c; return c; }

struct Counters {
  std::atomic<int64_t> forwards{0}, backwards{0}, declined{0}, waited{0}, retried{0}, recovered{0}, budget_fallbacks{0};
};
Counters& counters() { static Counters c; return c; }

// ---- where the host time of a call goes (diagnostics: set_profile(true), profile_read()) ----
enum Seg { SG_CHECKS = 0, SG_STREAM, SG_DRAIN, SG_SIZES, SG_ALLOC, SG_ARGS, SG_LIBRARY, SG_NODE, SG_RETURN,
           SB_UNPACK, SB_SETTLE, SB_ALLOC, SB_LIBRARY, SB_VIEWS, SG_COUNT };
const char* const kSegNames[SG_COUNT] = {"fwd.checks", "fwd.guard+stream+capture", "fwd.drain", "fwd.sizes", "fwd.alloc",
                                         "fwd.args", "fwd.library", "fwd.node", "fwd.return",
                                         "bwd.unpack+cotangents", "bwd.settle", "bwd.alloc", "bwd.library", "bwd.views"};
std::atomic<bool> g_profile{false};
std::atomic<int64_t> g_seg_ns[SG_COUNT];
std::atomic<int64_t> g_seg_n[SG_COUNT];
struct SegClock {
  bool on;
  std::chrono::steady_clock::time_point t;
  SegClock() : on(g_profile.load(std::memory_order_relaxed)) { if (on) t = std::chrono::steady_clock::now(); }
  void lap(int seg) {
    if (!on) return;
    auto n = std::chrono::steady_clock::now();
    g_seg_ns[seg] += std::chrono::duration_cast<std::chrono::nanoseconds>(n - t).count();
    g_seg_n[seg]++;
    t = n;
  }
};

[[noreturn]] void fail(const std::string& what) { throw std::runtime_error(what); }

void check_rc(int rc, const char* what) {
  if (rc != MGS_OK) fail(std::string(what) + ": " + mgs_last_error() + " (code " + std::to_string(rc) + ")");
}

// Release the GIL for a blocking wait -- only if this thread holds it (the autograd engine's threads do not).
struct MaybeReleaseGil {
  PyThreadState* saved = nullptr;
  MaybeReleaseGil() { if (PyGILState_Check()) saved = PyEval_SaveThread(); }
  ~MaybeReleaseGil() { if (saved) PyEval_RestoreThread(saved); }
};

void warn_runtime(const std::string& msg) {
  py::gil_scoped_acquire gil;
  if (PyErr_WarnEx(PyExc_RuntimeWarning, msg.c_str(), 2) < 0) throw py::error_already_set();
}

// What this binding keeps per device beside the ledger: the pinned block it gave the ledger as the device's ring (if it was the
// first to touch the device) and the default budget.
struct DeviceState {
  std::once_flag ring_once;
  at::Tensor status;
  std::atomic<int64_t> auto_safe_bytes{0};  // the default worst-case-workspace budget: 1/32 of the memory, at least 1 GB
};
DeviceState& state(int idx) {
  static DeviceState states[MGS_LEDGER_MAX_DEVICES];
  if (idx < 0 || idx >= MGS_LEDGER_MAX_DEVICES) fail("device index " + std::to_string(idx) + " is beyond the report ledger");
  return states[idx];
}
void ensure_ring(int idx) {
  DeviceState& st = state(idx);
  std::call_once(st.ring_once, [&] {
    if (mgs_ledger_ring(idx, nullptr, 0)) return;  // (the ctypes shim was first)
    at::Tensor t = at::full({NSLOTS * MGS_LEDGER_SLOT_WORDS}, -1, at::TensorOptions().dtype(at::kLong).device(at::kCPU)).pin_memory();
    uint64_t* words = reinterpret_cast<uint64_t*>(t.data_ptr<int64_t>());
    if (mgs_ledger_ring(idx, words, NSLOTS) == words) st.status = t;
  });
}

// A worst-case workspace that mgs_ledger_hold granted, charged against its device's budget for as long as somebody holds this.
struct Lease {
  int device;
  int64_t bytes;
  Lease(int d, int64_t b) : device(d), bytes(b) {}
  ~Lease() { mgs_ledger_unhold(device, bytes); }
  Lease(const Lease&) = delete;
  Lease& operator=(const Lease&) = delete;
};

struct ReleaseTicket { void operator()(MgsTicket* t) const { mgs_ledger_release(t); } };
using Ticket = std::unique_ptr<MgsTicket, ReleaseTicket>;

void sync_device(void* ctx) {
  MaybeReleaseGil nogil;
  c10::hip::HIPGuard g(*static_cast<int*>(ctx));
  (void)hipDeviceSynchronize();
}

// Read every report of the device that has arrived (wait: all of them): the ledger learns, this binding says what it hands back.
// `deferred`: append the warnings there instead of issuing them (callers that hold a lock of their own -- a node's -- issue them
// after dropping it: warn_runtime takes the GIL).
void drain(int dev, bool wait, std::vector<std::string>* deferred = nullptr) {
  MgsLedgerOut out;
  if (mgs_ledger_drain(dev, wait, &sync_device, &dev, &out) != MGS_OK) fail(mgs_last_error());
  if (!out.error && !out.n_warnings) return;
  const std::string failed = out.error ? out.error : "";  // (copies: the texts live until this thread's next ledger call)
  const std::vector<std::string> warnings(out.warnings, out.warnings + out.n_warnings);
  if (deferred) deferred->insert(deferred->end(), warnings.begin(), warnings.end());
  else for (const std::string& w : warnings) warn_runtime(w);
  if (!failed.empty()) fail(failed);
}

bool is_capturing(hipStream_t s) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &cs) != hipSuccess) { (void)hipGetLastError(); return true; }  // when in doubt: the Python path
  return cs != hipStreamCaptureStatusNone;
}

bool supported_F(int64_t F) { return F == 3 || F == 4 || F == 8 || F == 16 || F == 32 || F == 64; }

// The single-view shape the library's plan is asked about (include/mgsplat.h "the workspace plan"; F: channels rendered).
MgsPlanShape plan_shape(int64_t P, int64_t M, int64_t F, int64_t W, int64_t H) {
  return MgsPlanShape{(int32_t)P, (int32_t)M, (int32_t)F, (int32_t)W, (int32_t)H, 0, 0, 0};
}

const char* kBackwardTwice =
    "Trying to backward through the graph a second time (or directly access saved tensors after they have already been freed). "
    "Saved intermediate values of the graph are freed when you call .backward() or autograd.grad(). Specify retain_graph=True "
    "if you need to backward through the graph a second time or if you need to access saved tensors after calling backward.";

// ---- the autograd node: what _RasterizeGaussians.backward is in the reference (RAST/diff_gaussian_rasterization/__init__.py:
// 104-164), called by the engine without entering Python -------------------------------------------------------------------
struct MgsRasterizeBackward : public Node {
  MgsRasterArgs a;                       // the forward's arguments, reused as they were
  Ticket pending;                        // its outstanding device report in the ledger (nullptr: settled in the forward)
  MgsMarkKey key{};                      // the marks key of its shape
  std::vector<SavedVariable> saved;      // the reference's saved inputs: colors, feature, means3D, scales, rotations, cov3D, sh
  at::Tensor opacities, bg, viewmatrix, projmatrix, campos;  // kept alive (the argument struct holds their addresses)
  at::Tensor radii, ws, binning2, grad_buffer;
  std::shared_ptr<Lease> lease;          // the budget charge of a worst-case workspace (released with `ws`)
  // the images, weakly (they own this node through their grad_fn): a recovery re-renders into them if they still live
  c10::weak_intrusive_ptr<c10::TensorImpl> out_color{c10::intrusive_ptr<c10::TensorImpl>()}, out_feat{c10::intrusive_ptr<c10::TensorImpl>()};
  int device_index = 0;
  int32_t num_rendered = -1;             // the reference's count if the forward waited for it, else -1
  int64_t P = 0, M = 0, F = 0, H = 0, W = 0;
  bool include_feature = false;
  bool released = false;
  std::mutex mu;

  std::string name() const override { return "MgsRasterizeBackward"; }
  void release_variables() override {
    std::lock_guard<std::mutex> lk(mu);
    for (auto& s : saved) s.reset_data();
    saved.clear();
    opacities = bg = viewmatrix = projmatrix = campos = radii = ws = binning2 = grad_buffer = at::Tensor();
    lease.reset();
    released = true;
  }
  variable_list apply(variable_list&& grads) override;
  variable_list apply_locked(variable_list&& grads, std::vector<std::string>* warnings);
  void settle(hipStream_t stream, std::vector<std::string>* warnings);
  void recover(hipStream_t stream, bool handshake_only, int32_t binned);
};

// The asynchronous forward of this backward outgrew its workspace and the report is in: bin and render it AGAIN with room
// (capacity from the count the device reported, worst-case chunk pool: cannot overflow) into the same output tensors, so that the
// backward runs on a complete state (manigaussian_amd/_C.py recover_forward).
void MgsRasterizeBackward::recover(hipStream_t stream, bool handshake_only, int32_t binned) {
  if (handshake_only) {
    // the scene did not outgrow anything: a workgroup of the preprocess launch gave up waiting for workgroup 0's zeroed tables.
    // Same workspace, tables zeroed by a launch of their own this time (no workgroup waits for another).
    a.opt.set = 1;
    a.opt.table_init = 1;
  } else {
    const MgsPlanShape shape = plan_shape(P, M, include_feature ? F : 0, W, H);
    int64_t cap = 0, pool = 0;
    check_rc(mgs_plan_capacity(&shape, MGS_SIZE_COUNT, std::max<int64_t>(binned, 0), 0, 1.0, 1.0, &cap, &pool),
             "mgs_plan_capacity");
    const size_t nbytes = mgs_plan_binning_bytes(&shape, cap, 0, 0);
    if (!nbytes) fail(mgs_last_error());
    binning2 = at::empty({(int64_t)nbytes}, ws.options());
    a.binning = binning2.data_ptr();
    a.binning_bytes = nbytes;
    a.binning_capacity = (int32_t)cap;
    a.chunk_pool = 0;
  }
  a.async_forward = 0;
  a.bwd_accum = nullptr;  // the first run's preprocess zeroed the accumulators; nothing touched them since
  a.bwd_accum_bytes = 0;
  uint64_t* slot;
  uint32_t tag;
  check_rc(mgs_ledger_take_slot(device_index, &slot, &tag), "status slot");
  a.status_tag = tag;
  int32_t nr = 0;
  const auto f32 = radii.options().dtype(at::kFloat);
  auto alive = [&](const c10::weak_intrusive_ptr<c10::TensorImpl>& w, at::IntArrayRef shape) {
    c10::intrusive_ptr<c10::TensorImpl> p = w.lock();
    return p ? at::Tensor(std::move(p)) : at::empty(shape, f32);  // (nobody will read a fresh one; the kernels need a target)
  };
  at::Tensor oc = alive(out_color, {3, H, W});
  at::Tensor of = include_feature ? alive(out_feat, {F, H, W}) : at::Tensor();
  {
    MaybeReleaseGil nogil;
    check_rc(mgs_rasterize_forward(&a, radii.data_ptr<int32_t>(), oc.data_ptr<float>(),
                                   include_feature ? of.data_ptr<float>() : nullptr, &nr, slot, stream),
             "rasterizer forward (re-run after a workspace overflow)");
  }
  Ticket rerun(mgs_ledger_add(device_index, &a, 0, slot, &key, 0));  // (the marks learn the binned count from its report)
  if (!rerun) fail(mgs_last_error());
  mgs_ledger_superseded(pending.get());
  pending = std::move(rerun);
  num_rendered = nr;
  counters().recovered++;
}

// Backward entry: what is known about this backward's forward?  (manigaussian_amd/_C.py _settle)
void MgsRasterizeBackward::settle(hipStream_t stream, std::vector<std::string>* warnings) {
  if (!pending) return;
  MgsReport report;
  const int rc = mgs_ledger_poll(pending.get(), &report);
  if (rc == MGS_NEED_CAPACITY || rc == MGS_RETRY_TABLE_INIT) {
    MgsLedgerConfig config;
    mgs_ledger_get_config(&config);
    if (config.overflow_policy == MGS_OVERFLOW_RAISE) {
      drain(device_index, false, warnings);  // folds the report into the marks and raises ... unless an earlier drain already did
      fail(mgs_ledger_lost_step_message(rc));
    }
    drain(device_index, false, warnings);  // learn + warn (this ticket is recoverable and its backward has not been enqueued: no raise)
    recover(stream, rc == MGS_RETRY_TABLE_INIT, report.num_rendered);
    return;
  }
  if (rc != MGS_OK && rc != MGS_PENDING) drain(device_index, false, warnings);
  if (rc == MGS_PENDING) mgs_ledger_backward_enqueued(pending.get());  // too late to repair: if this forward overflowed, the next drain raises
}

// The node's mutex is never held while a warning is issued (warn_runtime takes the GIL; a Python thread that holds the GIL may
// be waiting for this mutex in release_variables): apply_locked collects them, apply issues them after the lock is gone.
variable_list MgsRasterizeBackward::apply(variable_list&& grads) {
  std::vector<std::string> warnings;
  variable_list out;
  std::exception_ptr err;
  try {
    out = apply_locked(std::move(grads), &warnings);
  } catch (...) {
    err = std::current_exception();
  }
  for (const std::string& w : warnings) warn_runtime(w);
  if (err) std::rethrow_exception(err);
  return out;
}

variable_list MgsRasterizeBackward::apply_locked(variable_list&& grads, std::vector<std::string>* warnings) {
  SegClock clk;
  std::lock_guard<std::mutex> lk(mu);
  TORCH_CHECK(!released, kBackwardTwice);
  variable_list out(9);
  at::Tensor g_color = grads.size() > 0 ? grads[0] : at::Tensor();
  at::Tensor g_feat = grads.size() > 1 ? grads[1] : at::Tensor();
  if (!g_color.defined() && !g_feat.defined()) return out;  // nothing flows back
  for (auto& s : saved) (void)s.unpack(shared_from_this());  // raises if a saved input was modified in place since the forward
  c10::hip::HIPGuard guard(device_index);
  const auto f32 = radii.options().dtype(at::kFloat);
  if (!g_color.defined()) g_color = at::zeros({3, H, W}, f32);
  if (g_color.scalar_type() != at::kFloat) fail("expected scalar type Float for dL_dout_color");
  if (!g_color.is_contiguous()) g_color = g_color.contiguous();
  if (include_feature) {
    if (!g_feat.defined()) g_feat = at::zeros({F, H, W}, f32);
    if (g_feat.scalar_type() != at::kFloat) fail("expected scalar type Float for dL_dout_language_feature");
    if (!g_feat.is_contiguous()) g_feat = g_feat.contiguous();
  }
  hipStream_t stream = c10::hip::getCurrentHIPStream(device_index).stream();
  clk.lap(SB_UNPACK);
  settle(stream, warnings);
  clk.lap(SB_SETTLE);
  const MgsPlanShape shape = plan_shape(P, M, include_feature ? F : 0, W, H);
  MgsGradientPlan L;
  check_rc(mgs_plan_gradients(&shape, &L), "mgs_plan_gradients");
  const bool prezeroed = grad_buffer.defined() && grad_buffer.numel() == L.total;
  at::Tensor flat = prezeroed ? grad_buffer : at::empty({L.total}, f32);
  grad_buffer = at::Tensor();  // pre-zeroed for ONE backward; a second one (retain_graph) allocates and fills
  float* base = flat.data_ptr<float>();
  a.accum_prezeroed = prezeroed ? 1 : 0;
  clk.lap(SB_ALLOC);
  check_rc(mgs_rasterize_backward(&a, num_rendered, radii.data_ptr<int32_t>(), g_color.data_ptr<float>(),
                                  include_feature ? g_feat.data_ptr<float>() : nullptr, base + L.means2D, nullptr,
                                  base + L.opacity, base + L.colors, include_feature ? base + L.feature : nullptr,
                                  base + L.means3D, base + L.cov3D, M ? base + L.sh : nullptr, base + L.scales,
                                  base + L.rotations, base + L.scratch, (size_t)(L.colors - L.scratch) * 4, stream),
           "rasterize_gaussians_backward");
  clk.lap(SB_LIBRARY);
  // order of the forward's inputs (reference: __init__.py:151-162): means3D, means2D, sh, colors_precomp, language_feature,
  // opacities, scales, rotations, cov3D_precomp -- only what somebody asked for
  auto view = [&](int i, at::IntArrayRef sizes, at::IntArrayRef strides, int64_t off) {
    if (task_should_compute_output(i)) out[i] = flat.as_strided(sizes, strides, off);
  };
  view(0, {P, 3}, {3, 1}, L.means3D);
  view(1, {P, 3}, {3, 1}, L.means2D);
  if (M) view(2, {P, M, 3}, {3 * M, 3, 1}, L.sh);
  view(3, {P, 3}, {3, 1}, L.colors);
  if (include_feature) view(4, {P, F}, {F, 1}, L.feature);
  view(5, {P, 1}, {1, 1}, L.opacity);
  view(6, {P, 3}, {3, 1}, L.scales);
  view(7, {P, 4}, {4, 1}, L.rotations);
  view(8, {P, 6}, {6, 1}, L.cov3D);
  clk.lap(SB_VIEWS);
  counters().backwards++;
  return out;
}

// a tensor the C ABI can take as it is: float32, on `dev`, contiguous -- or empty (a NULL pointer, like the reference's
// .data<float>() of torch.Tensor([]))
inline bool plain(const at::Tensor& t, const c10::Device& dev) {
  if (!t.defined()) return false;
  if (t.numel() == 0) return true;
  return t.scalar_type() == at::kFloat && t.device() == dev && t.is_contiguous();
}
inline const float* fptr(const at::Tensor& t) { return t.numel() == 0 ? nullptr : t.data_ptr<float>(); }

// GaussianRasterizer.forward -> _RasterizeGaussians.apply (RAST/diff_gaussian_rasterization/__init__.py:21-103), the hot path.
// Returns None when the call is not one this binding handles; the caller then takes manigaussian_amd/_C.py.
py::object rasterize(const at::Tensor& means3D, const at::Tensor& means2D, const at::Tensor& sh, const at::Tensor& colors,
                     const at::Tensor& feat, const at::Tensor& opacities, const at::Tensor& scales, const at::Tensor& rotations,
                     const at::Tensor& cov3D, const at::Tensor& bg, const at::Tensor& viewmatrix, const at::Tensor& projmatrix,
                     const at::Tensor& campos, int64_t H, int64_t W, double tanfovx, double tanfovy, double scale_modifier,
                     int64_t degree, bool prefiltered, bool debug, bool include_feature) {
  SegClock clk;
  Config& C = cfg();
  MgsLedgerConfig ledger;
  mgs_ledger_get_config(&ledger);
  const int mode = ledger.mode;
  auto decline = [&]() { counters().declined++; return py::none(); };
  if (!C.enabled.load() || debug || prefiltered || mode == MGS_MODE_BLOCKING) return decline();
  if (!means3D.defined() || !means3D.is_cuda() || means3D.dim() != 2 || means3D.size(1) != 3) return decline();  // (Python raises)
  const int64_t P = means3D.size(0);
  if (P == 0 || H <= 0 || W <= 0) return decline();
  const c10::Device dev = means3D.device();
  if (!plain(means3D, dev) || !plain(sh, dev) || !plain(colors, dev) || !plain(opacities, dev) || !plain(scales, dev) ||
      !plain(rotations, dev) || !plain(cov3D, dev) || !plain(bg, dev) || !plain(viewmatrix, dev) || !plain(projmatrix, dev) ||
      !plain(campos, dev) || opacities.numel() == 0 || bg.numel() == 0 || !means2D.defined())
    return decline();
  const int64_t M = sh.numel() != 0 ? (sh.dim() == 3 ? sh.size(1) : -1) : 0;
  if (M < 0) return decline();
  int64_t F = 0;
  if (include_feature) {
    if (!plain(feat, dev) || feat.dim() != 2 || feat.size(0) != P || !supported_F(feat.size(1)) ||
        (reinterpret_cast<uintptr_t>(feat.data_ptr()) & 15u))
      return decline();  // padded widths, odd offsets: the Python path copies
    F = feat.size(1);
  }
  const int di = dev.index();
  clk.lap(SG_CHECKS);
  c10::hip::HIPGuard guard(di);
  hipStream_t stream = c10::hip::getCurrentHIPStream(di).stream();
  if (is_capturing(stream)) return decline();
  DeviceState& st = state(di);
  ensure_ring(di);  // (the device's one ring of status slots: this binding's pinned block, or the ctypes shim's)
  clk.lap(SG_STREAM);
  drain(di, false);  // reports of earlier forwards (either binding's) that have arrived: learn their counts, raise if one overflowed
  clk.lap(SG_DRAIN);

  MgsOptions opt;
  {
    std::lock_guard<std::mutex> lk(C.mu);
    opt = C.opt;
  }
  int64_t safe_bytes = ledger.safe_bytes;
  if (safe_bytes < 0) {  // the default budget: 1/32 of this device's memory, at least 1 GB
    if (st.auto_safe_bytes == 0) {
      size_t total = 0;
      if (hipDeviceTotalMem(&total, di) != hipSuccess) { (void)hipGetLastError(); total = 0; }
      st.auto_safe_bytes = std::max<int64_t>((int64_t)1 << 30, (int64_t)(total / 32));
    }
    safe_bytes = st.auto_safe_bytes;
  }
  // (V = 0: a single view; the ctypes shim's batches have keys of their own)
  const MgsMarkKey key{0, 0, (int32_t)P, (int32_t)W, (int32_t)H, (int32_t)F, opt.tight_bins};
  // the arena's sizes, and the worst case: every Gaussian in every tile, every chunk of every block visited
  const MgsPlanShape shape = plan_shape(P, M, F, W, H);
  struct ArenaMemo { MgsPlanShape shape; int64_t budget; int rc; MgsArenaPlan plan; };  // the library's answer for the last shape
  static thread_local ArenaMemo memo{{-1, 0, 0, 0, 0, 0, 0, 0}, 0, MGS_ERR_INVALID_ARG, {}};
  if (std::memcmp(&memo.shape, &shape, sizeof(shape)) != 0 || memo.budget != safe_bytes) {
    memo.shape = shape; memo.budget = safe_bytes;
    memo.rc = mgs_plan_arena(&shape, safe_bytes, &memo.plan);
  }
  if (memo.rc != MGS_OK) return decline();  // (the Python path raises the library's message)
  const MgsArenaPlan& plan = memo.plan;
  // The worst-case workspace is taken only while the worst cases live forwards of this device still hold, plus this one, stay
  // within the budget (round 5 tested the budget per call: V forwards before the first backward pinned V x 4 GB at
  // configs[2]) -- and only if the allocator can give it; otherwise the shape goes by its marks, like any shape whose
  // worst case does not fit (the reference never allocates more than the count needs, rasterize_points.cu:27-33,84-89).
  const auto u8 = at::TensorOptions().dtype(at::kByte).device(dev);
  const auto f32 = at::TensorOptions().dtype(at::kFloat).device(dev);
  const size_t gb = plan.geom_bytes, ib = plan.img_bytes;
  const bool want_grad = torch::autograd::compute_requires_grad(means3D, means2D, sh, colors, feat, opacities, scales, rotations, cov3D);
  at::AutoDispatchBelowADInplaceOrView below_autograd;  // plain tensors from here on; the node is attached by hand
  at::Tensor ws;
  std::shared_ptr<Lease> lease;
  size_t bb = 0;
  bool worst = mode != MGS_MODE_ASYNC && plan.worst_fits;
  if (worst) {
    bb = plan.worst_bytes;
    if (!mgs_ledger_hold(di, (int64_t)bb, safe_bytes)) {
      worst = false;
    } else {
      lease = std::make_shared<Lease>(di, (int64_t)bb);  // (the node's if a backward follows; else it ends with this call)
      try {
        ws = at::empty({(int64_t)(gb + ib + bb)}, u8);
      } catch (const c10::OutOfMemoryError&) {
        worst = false;
        ws = at::Tensor();
        lease.reset();
      }
    }
    if (!worst) counters().budget_fallbacks++;
  }
  int64_t cap = 0, pool = 0, mark_R = 0;
  bool have_guess = worst;
  if (worst) { cap = plan.worst_capacity; pool = plan.worst_pool; }
  else have_guess = mgs_marks_guess(di, &key, &cap, &pool) == 1;
  (void)mgs_marks_get(di, &key, &mark_R, nullptr);
  const bool lazy = have_guess && (mode == MGS_MODE_ASYNC || (mode == MGS_MODE_SAFE && worst));
  if (mode == MGS_MODE_ASYNC && !lazy) return decline();  // first calls of a shape in async mode: the Python path learns the marks
  // wait for the preprocess: capacity from the mark (0: none yet), worst-case pool for that capacity (cannot overflow)
  if (!lazy) check_rc(mgs_plan_capacity(&shape, MGS_SIZE_COUNT, mark_R ? mark_R : -1, 0, 1.0, 1.0, &cap, &pool), "mgs_plan_capacity");

  clk.lap(SG_SIZES);
  // ONE allocation for the three opaque workspaces [geom | img | binning] (each a multiple of 256 bytes)
  if (!worst) {
    // (+ room for the forward preprocess to write the tile keys itself: no bin scatter launch, include/mgsplat.h
    //  mgs_binning_direct_extra; a worst-case capacity, above, covers them by itself)
    bb = mgs_plan_binning_bytes(&shape, cap, pool, 1);
    if (!bb) return decline();  // (a capacity of 2^31 or more, or such a pool: the Python path raises the library's message)
    ws = at::empty({(int64_t)(gb + ib + bb)}, u8);
  }
  at::Tensor out_color, out_feat;
  if (include_feature) {
    at::Tensor out = at::empty({3 + F, H, W}, f32);
    out_color = out.narrow(0, 0, 3);
    out_feat = out.narrow(0, 3, F);
  } else {
    out_color = at::empty({3, H, W}, f32);
    out_feat = at::zeros({1}, f32);  // rasterize_points.cu:71-79: a [1] placeholder
  }
  at::Tensor radii = at::empty({P}, at::TensorOptions().dtype(at::kInt).device(dev));
  at::Tensor grad_buffer;
  MgsGradientPlan GL{};
  if (want_grad) {
    check_rc(mgs_plan_gradients(&shape, &GL), "mgs_plan_gradients");
    grad_buffer = at::empty({GL.total}, f32);
  }
  clk.lap(SG_ALLOC);

  MgsRasterArgs a;
  std::memset(&a, 0, sizeof(a));
  a.P = (int32_t)P; a.D = (int32_t)degree; a.M = (int32_t)M; a.F = (int32_t)F; a.W = (int32_t)W; a.H = (int32_t)H;
  a.tanfovx = (float)tanfovx; a.tanfovy = (float)tanfovy; a.scale_modifier = (float)scale_modifier;
  a.prefiltered = 0; a.debug = 0; a.include_feature = include_feature ? 1 : 0;
  a.background = fptr(bg); a.means3D = fptr(means3D); a.shs = fptr(sh); a.colors_precomp = fptr(colors);
  a.language_feature = include_feature ? fptr(feat) : nullptr;
  a.opacities = fptr(opacities); a.scales = fptr(scales); a.rotations = fptr(rotations); a.cov3D_precomp = fptr(cov3D);
  a.viewmatrix = fptr(viewmatrix); a.projmatrix = fptr(projmatrix); a.campos = fptr(campos);
  char* wsp = reinterpret_cast<char*>(ws.data_ptr());
  a.geom = wsp; a.geom_bytes = gb; a.img = wsp + gb; a.img_bytes = ib; a.binning = wsp + gb + ib; a.binning_bytes = bb;
  a.binning_capacity = (int32_t)cap; a.chunk_pool = (int32_t)pool;
  a.async_forward = lazy ? 1 : 0;
  a.opt = opt;
  (void)mgs_plan_options(&shape, mark_R, &a.opt);  // seg and bin_mode for long per-tile lists
  if (want_grad) {
    a.bwd_accum = grad_buffer.data_ptr();
    a.bwd_accum_bytes = GL.accum_bytes;
  }
  uint64_t* slot;
  uint32_t tag;
  check_rc(mgs_ledger_take_slot(di, &slot, &tag), "status slot");
  a.status_tag = tag;
  int32_t nr = 0;
  int rc;
  float* feat_ptr = include_feature ? out_feat.data_ptr<float>() : nullptr;
  clk.lap(SG_ARGS);
  if (lazy) {
    rc = mgs_rasterize_forward(&a, radii.data_ptr<int32_t>(), out_color.data_ptr<float>(), feat_ptr, &nr, slot, stream);
  } else {
    py::gil_scoped_release nogil;  // the call polls a pinned word until the preprocess has reported
    rc = mgs_rasterize_forward(&a, radii.data_ptr<int32_t>(), out_color.data_ptr<float>(), feat_ptr, &nr, slot, stream);
    counters().waited++;
  }
  Ticket pending;
  at::Tensor binning2;
  if (rc == MGS_NEED_CAPACITY) {  // (waiting path) first call of the shape, or the scene grew: bin + render again with room
    const int64_t binned = (int64_t)(uint32_t)(*(volatile uint64_t*)slot);
    int64_t cap2 = 0, pool2 = 0;  // (nr: the reference's 3-sigma-rect count, at least the instances binned)
    check_rc(mgs_plan_capacity(&shape, MGS_SIZE_COUNT, nr, 0, 1.0, 1.0, &cap2, &pool2), "mgs_plan_capacity");
    const size_t nb = mgs_plan_binning_bytes(&shape, cap2, 0, 0);
    if (!nb) fail(mgs_last_error());
    binning2 = at::empty({(int64_t)nb}, u8);
    a.binning = binning2.data_ptr(); a.binning_bytes = nb; a.binning_capacity = (int32_t)cap2; a.chunk_pool = 0;
    check_rc(mgs_rasterize_forward_render(&a, nr, radii.data_ptr<int32_t>(), out_color.data_ptr<float>(), feat_ptr, stream),
             "rasterize_gaussians");
    (void)mgs_marks_learn(di, &key, binned, -1, 0);
    counters().retried++;
  } else {
    check_rc(rc, "rasterize_gaussians");
    // a forward that a backward will follow can be repaired there if it overflowed (recover)
    pending.reset(mgs_ledger_add(di, &a, 0, slot, &key, want_grad ? MGS_TICKET_RECOVERABLE : 0));
    if (!pending) fail(mgs_last_error());
  }
  counters().forwards++;
  clk.lap(SG_LIBRARY);
  if (want_grad) {
    std::shared_ptr<MgsRasterizeBackward> node(new MgsRasterizeBackward(), torch::autograd::deleteNode);
    node->set_next_edges(torch::autograd::collect_next_edges(means3D, means2D, sh, colors, feat, opacities, scales, rotations, cov3D));
    node->a = a; node->pending = std::move(pending); node->key = key; node->device_index = di;
    node->num_rendered = lazy ? -1 : nr;
    node->P = P; node->M = M; node->F = F; node->H = H; node->W = W; node->include_feature = include_feature;
    node->saved.reserve(7);
    for (const at::Tensor* t : {&colors, &feat, &means3D, &scales, &rotations, &cov3D, &sh}) node->saved.emplace_back(*t, false);
    node->opacities = opacities; node->bg = bg; node->viewmatrix = viewmatrix; node->projmatrix = projmatrix; node->campos = campos;
    node->radii = radii; node->ws = ws; node->binning2 = binning2; node->grad_buffer = grad_buffer;
    node->lease = lease;
    node->out_color = c10::weak_intrusive_ptr<c10::TensorImpl>(out_color.getIntrusivePtr());
    node->out_feat = c10::weak_intrusive_ptr<c10::TensorImpl>(out_feat.getIntrusivePtr());
    torch::autograd::set_history(out_color, node);
    torch::autograd::set_history(out_feat, node);
  }
  clk.lap(SG_NODE);
  py::object ret = py::make_tuple(out_color, out_feat, radii);
  clk.lap(SG_RETURN);
  return ret;
}

// ---- this binding's own switches, driven by manigaussian_amd/_lib.py and _C.py ---------------------------------------------
void set_options(int tight_bins, int fast_exp, int exact_cull, int bin_mode, int seg, int gm_waves, int dbg, int table_init) {
  Config& C = cfg();
  std::lock_guard<std::mutex> lk(C.mu);
  C.opt.set = 1; C.opt.tight_bins = tight_bins; C.opt.fast_exp = fast_exp; C.opt.exact_cull = exact_cull; C.opt.bin_mode = bin_mode;
  C.opt.seg = seg; C.opt.gm_waves = gm_waves; C.opt.dbg = dbg; C.opt.table_init = table_init;
}
bool set_enabled(bool on) { return cfg().enabled.exchange(on); }

void check_status(int dev, bool wait) {  // dev < 0: every device that has a ring
  for (int d = 0; d < MGS_LEDGER_MAX_DEVICES; d++)
    if ((dev < 0 || d == dev) && mgs_ledger_ring(d, nullptr, 0)) drain(d, wait);
}
int pending_count(int dev) { return mgs_ledger_outstanding(dev); }
int64_t held_bytes(int dev) { return mgs_ledger_held(dev); }

py::dict profile_read(bool reset) {
  py::dict d;
  for (int i = 0; i < SG_COUNT; i++) {
    d[kSegNames[i]] = py::make_tuple(g_seg_ns[i].load(), g_seg_n[i].load());
    if (reset) { g_seg_ns[i] = 0; g_seg_n[i] = 0; }
  }
  return d;
}

py::dict counters_dict(bool reset) {
  Counters& c = counters();
  py::dict d;
  d["forwards"] = c.forwards.load(); d["backwards"] = c.backwards.load(); d["declined"] = c.declined.load();
  d["waited"] = c.waited.load(); d["retried"] = c.retried.load(); d["recovered"] = c.recovered.load();
  d["budget_fallbacks"] = c.budget_fallbacks.load();
  if (reset) { c.forwards = 0; c.backwards = 0; c.declined = 0; c.waited = 0; c.retried = 0; c.recovered = 0; c.budget_fallbacks = 0; }
  return d;
}

}  // namespace

PYBIND11_MODULE(_mgs_torch, m) {
  m.doc() = "compiled autograd binding of libmgsplat.so (include/mgsplat.h); see manigaussian_amd/csrc/mgs_torch.cpp";
  if (mgs_abi_version() != MGS_ABI_VERSION)
    throw std::runtime_error("libmgsplat ABI version " + std::to_string(mgs_abi_version()) + " != the binding's " +
                             std::to_string(MGS_ABI_VERSION) + "; rebuild");
  mgs_options_default(&cfg().opt);
  m.attr("ABI_VERSION") = MGS_ABI_VERSION;
  m.def("build_id", []() { return std::string(mgs_build_id()); });
  m.def("rasterize", &rasterize);
  m.def("set_options", &set_options);
  m.def("set_enabled", &set_enabled);
  m.def("enabled", []() { return cfg().enabled.load(); });
  m.def("check_status", &check_status, py::arg("device") = -1, py::arg("wait") = true);
  m.def("pending_count", &pending_count);
  m.def("held_bytes", &held_bytes);
  m.def("counters", &counters_dict, py::arg("reset") = false);
  m.def("set_profile", [](bool on) { return g_profile.exchange(on); });
  m.def("profile_read", &profile_read, py::arg("reset") = true);
}
