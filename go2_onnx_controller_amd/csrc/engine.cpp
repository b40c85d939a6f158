// go2pi engine: C-ABI implementation (include/go2pi.h).
//
// Replaces the onnxruntime session behind ONNXActor
// (onnx_inference/src/cpp/onnx_actor.cpp:6-48) with an MI355X-native runtime:
//  - load: parse the .onnx with our own reader (onnx_model.cpp), lower it to a
//    program of dense layers (+ optional GRU), pack weights once into MFMA
//    fragment order (plan.cpp, program.hpp) and upload them to HBM (one arena);
//  - host path (go2pi_run): small batches replay a captured hipGraph whose
//    kernels read the observation from / write the action to pinned,
//    host-mapped staging (no memcpy nodes); larger batches stage through
//    device buffers and launch the fused batched kernel;
//  - device path (go2pi_run_device): enqueue on the caller's stream, no sync.
// No CPU fallback exists: without a HIP device, go2pi_create fails loudly.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <limits>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

#include <immintrin.h>
#include <sys/mman.h>

#include "../../include/go2pi.h"
#include "onnx_model.hpp"
#include "plan.hpp"
#include "program.hpp"

namespace {

using go2pi::ApiError;
using go2pi::ResForm;
using go2pi::Switches;

thread_local std::string g_last_error;

// Spin with the host's pause cadence until done() holds; the clock is read every 1024
// turns and the wait gives up after 2 s. Returns done()'s last word.
template <class F>
bool spin_until(F &&done) {
  const auto t0 = std::chrono::steady_clock::now();
  for (unsigned it = 0; !done(); ++it) {
    __builtin_ia32_pause();
    if ((it & 1023) == 1023 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) return done();
  }
  return true;
}

struct HipError : std::runtime_error {
  int code;
  HipError(const std::string &m, int c) : std::runtime_error(m), code(c) {}
};

void hip_check(hipError_t e, const char *what) {
  if (e != hipSuccess) throw HipError(std::string("HIP error in ") + what + ": " + hipGetErrorString(e), GO2PI_E_DEVICE);
}
void hip_check(int e, const char *what) { hip_check(static_cast<hipError_t>(e), what); }

// Pinned host-mapped blocks are never returned to HIP while the process runs:
// hipHostFree (like hipFree) performs an implicit hipDeviceSynchronize, which
// waits for every live resident kernel of every other engine on the device (and
// never returns while another thread keeps one of them busy). A destroyed
// engine's blocks go to this process-wide cache and the next engine reuses them.
std::mutex g_pin_mu;
std::vector<std::pair<size_t, void *>> g_pin_free;  // (bytes, block)

// bytes: in, the size wanted; out, the size of the block handed out (a reused block
// may be larger), which is what pin_give must get back
void *pin_take(size_t &bytes) {
  bytes = (bytes + 4095) & ~(size_t)4095;
  {
    std::lock_guard<std::mutex> lk(g_pin_mu);
    size_t best = g_pin_free.size();
    for (size_t i = 0; i < g_pin_free.size(); ++i)
      if (g_pin_free[i].first >= bytes && (best == g_pin_free.size() || g_pin_free[i].first < g_pin_free[best].first))
        best = i;
    if (best < g_pin_free.size()) {
      void *p = g_pin_free[best].second;
      bytes = g_pin_free[best].first;
      g_pin_free.erase(g_pin_free.begin() + (long)best);
      return p;
    }
  }
  void *p = nullptr;
  hip_check(hipHostMalloc(&p, bytes, hipHostMallocMapped | hipHostMallocCoherent), "hipHostMalloc");
  return p;
}

void pin_give(void *p, size_t bytes) {
  std::lock_guard<std::mutex> lk(g_pin_mu);
  g_pin_free.emplace_back(bytes, p);
}

// The resident kernels' request ring in fine-grained device memory that the host
// writes through its large-BAR mapping of VRAM: a request then reaches the polling
// wave as posted PCIe writes into the GPU's own memory, instead of the wave reading
// pinned host memory across PCIe (a read round trip per poll). tools/bar_probe.hip,
// profiles/r05_bar_probe.txt: live-kernel host -> GPU -> host round trip p50 1.78 us
// against 2.47 us. Whether an allocation is mapped into the host's address space is
// checked with msync() on its pages, never by touching it; without large BAR the ring
// stays in pinned host memory (GO2PI_REQ_HOST=1 forces that, for A/B). Like pinned
// blocks, these are never freed (hipFree synchronises the device): cached per device.
std::vector<std::tuple<int, size_t, void *>> g_bar_free;  // (device, bytes, block), under g_pin_mu
std::vector<int> g_bar_absent;                            // devices whose VRAM the host cannot map

// true when [p, p + bytes) lies inside mappings of this process that are readable
// and writable from the CPU. ROCm's thunk reserves the GPU's virtual aperture with
// PROT_NONE mappings, so an address range being mapped (msync succeeds) does not make
// it host-accessible: without large BAR a fine-grained VRAM block sits in such a range
// and a host store to it faults. /proc/self/maps gives the protection.
bool host_mapped(const void *p, size_t bytes) {
  uintptr_t a = reinterpret_cast<uintptr_t>(p);
  const uintptr_t end = a + bytes;
  FILE *f = std::fopen("/proc/self/maps", "r");
  if (!f) return false;
  char line[512];
  bool ok = false;
  while (a < end && std::fgets(line, sizeof line, f)) {  // (ascending address order)
    unsigned long lo = 0, hi = 0;
    char perm[8] = {0};
    if (std::sscanf(line, "%lx-%lx %7s", &lo, &hi, perm) != 3) continue;
    if (hi <= a) continue;
    if (lo > a || perm[0] != 'r' || perm[1] != 'w') break;  // a hole, or not read-write
    a = hi;  // covered up to hi; the rest must follow in the next mapping(s)
  }
  ok = a >= end;
  std::fclose(f);
  return ok;
}

// a host-writable device block of at least `bytes` (out: its size) on the current
// device `device`, zeroed; nullptr when the host cannot map this device's memory, or
// with req_host (Switches: no block wanted)
void *bar_take(int device, size_t &bytes, bool req_host) {
  bytes = (bytes + 4095) & ~(size_t)4095;
  if (req_host) return nullptr;
  void *p = nullptr;
  {
    std::lock_guard<std::mutex> lk(g_pin_mu);
    if (std::find(g_bar_absent.begin(), g_bar_absent.end(), device) != g_bar_absent.end()) return nullptr;
    for (size_t i = 0; i < g_bar_free.size(); ++i)
      if (std::get<0>(g_bar_free[i]) == device && std::get<1>(g_bar_free[i]) >= bytes) {
        bytes = std::get<1>(g_bar_free[i]);
        p = std::get<2>(g_bar_free[i]);
        g_bar_free.erase(g_bar_free.begin() + (long)i);
        break;
      }
  }
  if (!p) {
    if (hipExtMallocWithFlags(&p, bytes, hipDeviceMallocFinegrained) != hipSuccess) {
      (void)hipGetLastError();
      return nullptr;  // (this engine only: an allocation failure may be transient)
    }
    if (!host_mapped(p, bytes)) {  // the host cannot map this device's memory: for the whole process
      std::lock_guard<std::mutex> lk(g_pin_mu);
      g_bar_absent.push_back(device);
      g_bar_free.emplace_back(device, bytes, p);  // (kept: hipFree would synchronise the device)
      return nullptr;
    }
  }
  std::memset(p, 0, bytes);  // (through the mapping: a reused ring holds another engine's tags)
  _mm_sfence();
  return p;
}

void bar_give(int device, void *p, size_t bytes) {
  std::lock_guard<std::mutex> lk(g_pin_mu);
  g_bar_free.emplace_back(device, bytes, p);
}

// Every entry point leaves the calling thread's current HIP device as it found it
// (the engine switches to its own device for its work).
struct DeviceRestore {
  int prev = -1;
  DeviceRestore() {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
  }
  ~DeviceRestore() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

}  // namespace

namespace {
void res_register(go2pi_engine *e);
unsigned *yield_word(int device);
void res_unregister(go2pi_engine *e);
std::unique_lock<std::mutex> evict_residents(const go2pi_engine *self, int64_t batch);
// The process-wide registry of engines that may hold a resident kernel, and the lock
// that orders a batched launch's eviction + enqueue against every resident relaunch
// (evict_residents, resident_start)
std::mutex g_res_mu;
}  // namespace

struct go2pi_engine {
  go2pi::Model model;
  go2pi_opts opts{};
  Switches sw{};  // as the environment stood when build() began (plan.hpp)
  int device = 0;
  int waves = 8;
  int small_batch = 8;
  hipStream_t stream = nullptr;
  go2pi::DevProgram prog{};
  std::vector<void *> allocs;  // device allocations
  std::vector<std::pair<size_t, void *>> pinned;  // pinned host blocks (returned to the cache)
  float *d_hidden = nullptr;   // [max_batch][H]
  float *d_obs = nullptr;      // host-path staging [max_batch][in]
  float *d_act = nullptr;      // [max_batch][out]
  float *d_tmp[2] = {nullptr, nullptr};  // small-batch activations [SMALL_MAXB][maxw]
  // a program with residual connections only: the GEMV chain's carried rows [SMALL_MAXB][maxw],
  // cleared once at build; two, alternated, so a layer never reads the buffer it writes
  float *d_carry[2] = {nullptr, nullptr};
  int tmp_stride = 0;
  float *h_obs = nullptr, *h_act = nullptr;  // pinned, host-mapped
  float *m_obs = nullptr, *m_act = nullptr;  // device aliases of the above
  unsigned long long *h_actg = nullptr, *m_actg = nullptr;  // resident act(): {epoch, value} action granules
  size_t n_actg = 0;
  hipGraphExec_t graphs[GO2PI_SMALL_MAXB + 1] = {};
  hipGraph_t graph_defs[GO2PI_SMALL_MAXB + 1] = {};
  go2pi_cost cost{};
  int64_t n_stamps = 0;
  // single-launch small-batch path (policy_latency_kernel)
  bool latency_ok = false;
  unsigned long long *d_gran = nullptr;  // [nl-1][gstride] {tag, value} granules
  int gstride = 0;
  unsigned *h_err = nullptr, *m_err = nullptr;    // host-mapped error words: [0] batch-1 hand-off, [64] batched
                                                   // kernel layer hand-off (each on its own cache line)
  unsigned *h_done = nullptr, *m_done = nullptr;  // host-mapped completion word (own cache line)
  bool done_ok = false;                            // final layer is one tile: WG 0 signals completion
  go2pi::DevProgram *d_prog = nullptr;             // device copy of prog (what every kernel reads)
  unsigned epoch = 1, last_epoch = 0;
  // resident batch <= SMALL_MAXB path (resident.hip, opts.resident_ms > 0)
  bool resident_ok = false, resident_live = false;
  std::atomic<int> res_flag{0};  // resident_live, readable from other threads (evict_residents)
  // the kernel that serves act() and the one that serves a controller tick (program.hpp
  // ResForm), decided by the planner (plan.cpp plan_resident); res_ctl None: ticks are served by a launch each (the
  // controller form applies to dense policies without LayerNormalization)
  ResForm res_act = ResForm::None, res_ctl = ResForm::None;
  unsigned long long *d_hgran = nullptr;  // GRU form: [2][SMALL_MAXB][H] hidden-row granules (two buffers)
  bool resident_ctl = false;  // the live kernel is the controller-tick form
  int64_t res_launches = 0;   // resident kernel launches (go2pi_resident_launches)
  std::vector<float> res_rows = std::vector<float>(GO2PI_SMALL_MAXB * (GO2PI_CTL_RAW + 16 * GO2PI_CTL_STEP_DIM));
  unsigned long long *h_req = nullptr, *m_req = nullptr;  // request granules: host view, device view
  size_t req_bar_bytes = 0;  // > 0: the ring is in device memory the host writes through the BAR (bar_take)
  unsigned long long *d_mirror = nullptr;                 // device copy of the request (workgroup 0 -> the rest)
  unsigned long long res_idle_ticks = 0;                  // 100 MHz wall-clock ticks
  std::chrono::steady_clock::time_point res_last{};
  // controller tick (go2pi_controller_step*)
  int ctl_hist = 0;                        // kHistory when the policy's I/O is a Go2 controller's, else 0
  go2pi::DevCtlParams *d_ctl = nullptr;    // device copy of the parameters
  char *h_ctl = nullptr, *m_ctl = nullptr; // host path, batch <= SMALL_MAXB: pinned host-mapped staging
  char *d_ctlbuf = nullptr;                // host path, larger batches: device staging (lazy)

  // Teardown touches only this engine's stream: no hipFree / hipHostFree /
  // hipDeviceSynchronize, each of which would wait for every other engine's live
  // resident kernel on the device (device memory is stream-ordered, pinned
  // blocks go back to the process-wide cache).
  ~go2pi_engine() {
    DeviceRestore keep;
    if (resident_ok) res_unregister(this);
    (void)hipSetDevice(device);
    if (resident_live) {  // tell the resident kernel to leave (the sync below waits for it)
      __atomic_store_n(h_req, (unsigned long long)GO2PI_RES_LEAVE << 32, __ATOMIC_SEQ_CST);
      resident_live = false;
    }
    if (stream) (void)hipStreamSynchronize(stream);
    for (int i = 0; i <= GO2PI_SMALL_MAXB; ++i) {
      if (graphs[i]) (void)hipGraphExecDestroy(graphs[i]);
      if (graph_defs[i]) (void)hipGraphDestroy(graph_defs[i]);
    }
    for (void *p : allocs) (void)hipFreeAsync(p, stream);
    for (auto &b : pinned) pin_give(b.second, b.first);
    if (req_bar_bytes) bar_give(device, h_req, req_bar_bytes);
    if (stream) {
      (void)hipStreamSynchronize(stream);
      (void)hipStreamDestroy(stream);
    }
  }

  // device memory: stream-ordered on the engine's stream (usable by any stream once
  // dalloc returns)
  template <class T>
  T *dalloc(size_t count) {
    void *p = nullptr;
    hip_check(hipMallocAsync(&p, std::max<size_t>(count, 1) * sizeof(T), stream), "hipMallocAsync");
    allocs.push_back(p);
    hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
    return static_cast<T *>(p);
  }
  // pinned, host-mapped (fine-grained) memory and its device alias
  template <class T>
  void palloc(T **host, T **dev, size_t bytes) {
    size_t got = bytes;
    void *p = pin_take(got);
    pinned.emplace_back(got, p);  // the block's real size goes back to the cache
    std::memset(p, 0, bytes);
    *host = static_cast<T *>(p);
    if (dev) hip_check(hipHostGetDevicePointer((void **)dev, p, 0), "hipHostGetDevicePointer");
  }
  template <class T>
  T *upload(const std::vector<T> &v) {
    T *p = dalloc<T>(v.size());
    if (!v.empty()) hip_check(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice), "hipMemcpy");
    return p;
  }

  bool use_chain(int64_t batch) const {
    return !model.has_gru && small_batch > 0 && batch <= small_batch;
  }

  bool use_latency(int64_t batch) const { return latency_ok && batch <= GO2PI_SMALL_MAXB; }

  // Enqueue one forward over `batch` rows (obs/act: device-accessible pointers).
  // done (single-launch path only): host-mapped word the kernel sets to the call's epoch.
  // granule tags of the next single-launch call (layer l of this call: e0 + l)
  unsigned next_epoch(hipStream_t s) {
    const unsigned n = (unsigned)prog.nl;
    if (epoch > 0xFFFFFFFFu - 2 * n) {  // tag space exhausted (~1e9 calls): clear granules, restart
      hip_check(hipMemsetAsync(d_gran, 0, sizeof(unsigned long long) * (size_t)(prog.nl - 1) * gstride, s),
                "hipMemsetAsync");
      epoch = 1;
    }
    const unsigned e0 = epoch;
    epoch += n;
    last_epoch = e0;
    return e0;
  }

  // Host spin on the host-mapped completion word of the single-launch path;
  // false: not observed within 2 s (the caller falls back to a stream sync).
  bool spin_done() {
    const unsigned want = last_epoch;
    const unsigned *done = h_done;
    return spin_until([=] { return __atomic_load_n(done, __ATOMIC_ACQUIRE) == want; });
  }

  // ---- resident path: one launch serves every batch <= SMALL_MAXB go2pi_run
  // until another call needs the stream (resident_stop) or it idles out.
  void resident_stop() {
    if (!resident_live) return;
    __atomic_store_n(h_req, (unsigned long long)GO2PI_RES_LEAVE << 32, __ATOMIC_SEQ_CST);
    resident_live = false;
    res_flag.store(0);
    hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize (resident kernel leaving)");
  }
  void resident_start(const go2pi::DevCtl *ctl) {
    // (never between another thread's eviction and its batched launch: evict_residents)
    std::lock_guard<std::mutex> res_lk(g_res_mu);
    const size_t ng = (size_t)std::max(1, prog.nl - 1) * gstride;
    hip_check(hipMemsetAsync(d_gran, 0, ng * sizeof(unsigned long long), stream), "hipMemsetAsync");
    hip_check(hipMemsetAsync(d_mirror, 0, sizeof(unsigned long long) * (1 + GO2PI_SMALL_MAXB * (size_t)model.in_dim),
                             stream),
              "hipMemsetAsync");
    if (d_hgran)
      hip_check(hipMemsetAsync(d_hgran, 0, sizeof(unsigned long long) * 2 * GO2PI_SMALL_MAXB * (size_t)model.gru.H,
                               stream),
                "hipMemsetAsync");
    __atomic_store_n(h_req, 0ull, __ATOMIC_SEQ_CST);
    __atomic_store_n(h_done, 0u, __ATOMIC_SEQ_CST);
    std::memset(h_actg, 0, sizeof(unsigned long long) * n_actg);
    const ResForm form = ctl ? res_ctl : res_act;
    switch (form) {
      case ResForm::Act1:
      case ResForm::R1:
        hip_check(go2pi::launch_resident1(prog, d_prog, m_req, m_actg, m_err, m_done, res_idle_ticks, prog.yield, ctl,
                                          form, sw.a1_depth, sw.a1_cw, stream),
                  "resident launch (one workgroup)");
        break;
      case ResForm::Wide:
        hip_check(go2pi::launch_resident_wide(prog, d_prog, m_req, m_actg, d_gran, gstride, m_err, m_done,
                                              res_idle_ticks, prog.yield, stream),
                  "resident launch (wide policy)");
        break;
      case ResForm::Multi:
        hip_check(go2pi::launch_resident(prog, d_prog, m_req, m_actg, d_gran, gstride, d_mirror, m_err, m_done,
                                         res_idle_ticks, ctl, d_hgran, d_hidden, prog.yield, sw.res_tiled0, stream),
                  "resident launch");
        break;
      case ResForm::None: throw ApiError("no resident kernel serves this request", GO2PI_E_INVALID);
    }
    ++res_launches;
    resident_live = true;
    res_flag.store(1);
    resident_ctl = ctl != nullptr;
    res_last = std::chrono::steady_clock::now();
  }
  // One request to the resident kernel. ctl null: act(), `rows` = obs [batch][in_dim];
  // the action lands in h_act. ctl: a controller tick, `rows` = its inputs concatenated
  // (state | joystick | obs | action, each batch rows); the outputs land in the staging
  // ctl names; flags = GO2PI_RES_* bits. The rows travel as tagged granules.
  // false: not served because the kernel kept being told to leave (a batched launch
  // on the device evicts live resident kernels, evict_residents): the caller serves
  // the request by a launch instead; the kernel is relaunched by a later call.
  // go2pi_run's fast path makes no HIP call while a live kernel serves it (lazy_dev):
  // need_device() switches the calling thread to the engine's device the first time a
  // stop or relaunch needs the runtime, and dev_done() switches it back.
  bool lazy_dev = false, dev_switched = false;
  int dev_saved = -1;
  void need_device() {
    if (!lazy_dev || dev_switched) return;
    if (hipGetDevice(&dev_saved) != hipSuccess) dev_saved = -1;
    hip_check(hipSetDevice(device), "hipSetDevice");
    dev_switched = true;
  }
  void dev_done() {
    if (dev_switched && dev_saved >= 0 && dev_saved != device) (void)hipSetDevice(dev_saved);
    lazy_dev = dev_switched = false;
  }
  // the live kernel serves the next request as it is (no stop or relaunch due first)
  bool resident_ready(const go2pi::DevCtl *ctl) const {
    const auto idle = std::chrono::microseconds(1000LL * opts.resident_ms);
    return resident_live && resident_ctl == (ctl != nullptr) && std::chrono::steady_clock::now() - res_last <= idle / 2 &&
           __atomic_load_n(h_done, __ATOMIC_ACQUIRE) != GO2PI_RES_LEAVE &&
           epoch <= 0xFFFFFFF0u - 2 * ((unsigned)prog.nl + 2);
  }
  // The granules of one request's answer: {offset, count} ranges of h_actg (act(): the
  // action rows; the controller form's: the requested outputs, the observation rows
  // first, as the kernel stores them first). The scan resumes where it stopped.
  struct GranScan {
    int r[6][2];
    int nr = 0, ri = 0, k = 0;
    void add(int off, int n) {
      r[nr][0] = off;
      r[nr++][1] = n;
    }
  };
  GranScan gran_scan(bool ctl, int64_t batch, unsigned flags) const {
    GranScan sc;
    const int b = (int)batch;
    if (!ctl) {
      sc.add(0, b * model.out_dim);
      return sc;
    }
    const go2pi::CtlGran G = go2pi::ctl_gran(model.in_dim);
    sc.add(G.obs, b * model.in_dim);
    if (flags & GO2PI_RES_STATUS) sc.add(G.status, b);
    sc.add(G.act, b * GO2PI_CTL_DOF);
    if (flags & GO2PI_RES_QDES) sc.add(G.qdes, 2 * b * GO2PI_CTL_DOF);
    if (flags & GO2PI_RES_KP) sc.add(G.kp, 2 * b * GO2PI_CTL_DOF);
    if (flags & GO2PI_RES_KD) sc.add(G.kd, 2 * b * GO2PI_CTL_DOF);
    return sc;
  }
  // true once every granule of sc carries tag e0
  bool gran_done(GranScan &sc, unsigned e0) const {
    for (; sc.ri < sc.nr; ++sc.ri, sc.k = 0) {
      const unsigned long long *g = h_actg + sc.r[sc.ri][0];
      const int n = sc.r[sc.ri][1];
      while (sc.k < n && (unsigned)(__atomic_load_n(g + sc.k, __ATOMIC_ACQUIRE) >> 32) == e0) ++sc.k;
      if (sc.k < n) return false;
    }
    return true;
  }
  // the act() answer's values to h_act
  void act_take(int64_t batch) {
    const int nout = (int)batch * model.out_dim;
    for (int j = 0; j < nout; ++j) {
      const unsigned bits = (unsigned)__atomic_load_n(h_actg + j, __ATOMIC_RELAXED);
      std::memcpy(h_act + j, &bits, 4);
    }
  }
  // the controller form's answer granules to the caller's buffers (res_ctl Act1)
  void ctl_take(int64_t batch, float *obs, float *action, double *q_des, double *kp, double *kd,
                uint32_t *status) const {
    const go2pi::CtlGran G = go2pi::ctl_gran(model.in_dim);
    const int b = (int)batch, nd = b * GO2PI_CTL_DOF;
    auto lo = [&](int i) { return (uint32_t)__atomic_load_n(h_actg + i, __ATOMIC_RELAXED); };
    auto f64 = [&](int off, double *dst) {
      for (int i = 0; i < nd; ++i) {
        const uint64_t bits = (uint64_t)lo(off + 2 * i) | ((uint64_t)lo(off + 2 * i + 1) << 32);
        std::memcpy(dst + i, &bits, 8);
      }
    };
    for (int i = 0; i < b * model.in_dim; ++i) {
      const uint32_t bits = lo(G.obs + i);
      std::memcpy(obs + i, &bits, 4);
    }
    for (int i = 0; i < nd; ++i) {
      const uint32_t bits = lo(G.act + i);
      std::memcpy(action + i, &bits, 4);
    }
    if (q_des) f64(G.qdes, q_des);
    if (kp) f64(G.kp, kp);
    if (kd) f64(G.kd, kd);
    if (status)
      for (int i = 0; i < b; ++i) status[i] = lo(G.status + i);
  }
  bool resident_serve(const go2pi::DevCtl *ctl, const float *rows, int64_t batch, unsigned flags) {
    if (resident_live && resident_ctl != (ctl != nullptr)) {  // the other form is live
      need_device();
      resident_stop();
    }
    const int n = (int)batch * (model.in_dim + (ctl ? GO2PI_CTL_RAW : 0));
    const auto idle = std::chrono::microseconds(1000LL * opts.resident_ms);  // (us: idle / 2 stays > 0 at 1 ms)
    for (int attempt = 0;; ++attempt) {
      // layer tags e + 1 + l: an epoch spans nl + 2 tags
      const unsigned span = (unsigned)prog.nl + 2;
      if (epoch > 0xFFFFFFF0u - 2 * span) {  // tag space exhausted: restart with zeroed granules
        need_device();
        resident_stop();
        epoch = 1;
      }
      const unsigned e0 = epoch;
      epoch += span;
      last_epoch = e0;
      const auto now = std::chrono::steady_clock::now();
      // the kernel leaves after resident_ms idle: past half of it, relaunch rather than race its exit
      if (resident_live && (now - res_last > idle / 2 || __atomic_load_n(h_done, __ATOMIC_ACQUIRE) == GO2PI_RES_LEAVE)) {
        need_device();
        resident_stop();
      }
      if (!resident_live) {
        need_device();
        resident_start(ctl);
      }
      for (int i = 0; i < n; ++i) {
        unsigned bits;
        std::memcpy(&bits, rows + i, 4);
        __atomic_store_n(h_req + 1 + i, ((unsigned long long)e0 << 32) | bits, __ATOMIC_RELAXED);
      }
      __atomic_store_n(h_req, ((unsigned long long)e0 << 32) | (unsigned)batch | flags, __ATOMIC_RELEASE);
      if (req_bar_bytes) _mm_sfence();  // the BAR mapping is write-combined: send the request now
      unsigned d = 0;
      // act() and the granule controller form: the answer granules themselves, every tag =
      // this request's epoch; the r04 / multi-workgroup controller forms: a done word
      // behind the drained outputs
      const bool gran = !ctl || res_ctl == ResForm::Act1;
      // a scan of the whole answer from its start: true when the kernel served this request
      auto answered = [&] {
        GranScan all = gran_scan(ctl != nullptr, batch, flags);
        return gran_done(all, e0);
      };
      if (!gran) {
        spin_until([&] { return (d = __atomic_load_n(h_done, __ATOMIC_ACQUIRE)) == e0 || d == GO2PI_RES_LEAVE; });
      } else {
        GranScan sc = gran_scan(ctl != nullptr, batch, flags);  // (resumes where it stopped)
        spin_until([&] {
          if (gran_done(sc, e0)) {
            d = e0;
            return true;
          }
          if ((d = __atomic_load_n(h_done, __ATOMIC_ACQUIRE)) != GO2PI_RES_LEAVE) return false;
          // the kernel may have answered this request and then left (a LEAVE header
          // from evict_residents, or a moved yield counter): its answer granules are
          // acknowledged before the LEAVE done word (resident.hip: vmcnt(0), barrier,
          // then done), so a rescan after seeing LEAVE finds them if it served the
          // request. Treating a served request as unserved would run it twice: for a
          // GRU / LSTM policy, advancing the hidden state twice.
          if (answered()) d = e0;
          return true;
        });
      }
      res_last = std::chrono::steady_clock::now();
      bool served = d == e0;
      if (!served) {
        // the kernel left: wait for it to drain. An idle exit racing this request is
        // benign (serve it from a fresh launch with a fresh epoch); a hand-off timeout
        // (h_err set) is a device-side protocol fault and is reported, not retried
        need_device();
        resident_stop();
        // the kernel has exited (stream synced): a request it served has every granule
        served = gran && answered();
      }
      if (served) {
        if (!ctl) act_take(batch);
        return true;
      }
      if (__atomic_load_n(h_err, __ATOMIC_ACQUIRE)) {
        __atomic_store_n(h_err, 0u, __ATOMIC_RELEASE);
        throw HipError("resident kernel: a layer hand-off timed out (request not served)", GO2PI_E_DEVICE);
      }
      if (d != GO2PI_RES_LEAVE)
        throw HipError("resident kernel did not answer within 2 s (request not served)", GO2PI_E_DEVICE);
      if (attempt >= 1) return false;  // evicted again (or idle exit twice): serve by a launch
    }
  }

  void check_handoff() {
    if (h_err && __atomic_load_n(h_err, __ATOMIC_ACQUIRE)) {
      __atomic_store_n(h_err, 0u, __ATOMIC_RELEASE);
      throw HipError("batch-1 kernel hand-off timed out (workgroups not co-resident?)", GO2PI_E_DEVICE);
    }
    if (h_err && __atomic_load_n(h_err + 64, __ATOMIC_ACQUIRE)) {
      __atomic_store_n(h_err + 64, 0u, __ATOMIC_RELEASE);
      throw HipError("batched kernel: a layer hand-off between waves timed out (outputs invalid)", GO2PI_E_DEVICE);
    }
  }

  // act() by the resident kernel, the action into the caller's buffer; false: not served
  // (resident_serve)
  bool resident_act(const float *obs, float *act, int64_t batch) {
    if (!resident_serve(nullptr, obs, batch, 0u)) return false;
    check_handoff();
    std::memcpy(act, h_act, sizeof(float) * (size_t)batch * model.out_dim);
    return true;
  }

  // Enqueue one controller tick (device-accessible pointers in c).
  void enqueue_ctl(const go2pi::DevCtl &c, int64_t batch, hipStream_t s, unsigned *done = nullptr) {
    if (use_latency(batch) && done_ok) {
      const unsigned e0 = next_epoch(s);
      hip_check(go2pi::launch_latency_ctl(prog, d_prog, c, (int)batch, e0, d_gran, gstride, m_err, done, s),
                "controller latency launch");
    } else {
      hip_check(go2pi::launch_policy_fused_ctl(prog, d_prog, waves, c, d_hidden, (int)batch, s),
                "controller fused launch");
    }
  }

  void enqueue(const float *obs, float *act, int64_t batch, hipStream_t s, unsigned *done = nullptr) {
    if (use_latency(batch)) {
      const unsigned e0 = next_epoch(s);
      hip_check(go2pi::launch_latency(prog, d_prog, obs, act, (int)batch, e0, d_gran, gstride, m_err, done, s),
                "latency launch");
    } else if (use_chain(batch)) {
      const float *x = obs;
      int xs = prog.in_dim;
      // residual connections (DevProgram::res): one carried value is live at a time; the
      // layer that writes the next one writes the other buffer
      int srcm = 0, cur = 0;
      for (int l = 0; l < prog.nl; ++l) srcm |= prog.res[l] ? 1 << (prog.res[l] - 1) : 0;
      for (int l = 0; l < prog.nl; ++l) {
        const bool last = l == prog.nl - 1;
        float *y = last ? act : d_tmp[l & 1];
        const int ys = last ? prog.out_dim : tmp_stride;
        const float *cin = prog.res[l] ? d_carry[cur] : nullptr;
        float *cout = nullptr;
        if ((srcm >> l) & 1) cout = d_carry[cur ^= 1];
        hip_check(go2pi::launch_gemv_layer(prog, l, obs, x, xs, y, ys, (int)batch, s, cin, cout, tmp_stride),
                  "gemv_layer launch");
        x = y;
        xs = ys;
      }
    } else {
      hip_check(go2pi::launch_policy_fused(prog, d_prog, waves, obs, act, d_hidden, (int)batch, 1, s), "fused launch");
    }
  }

  hipGraphExec_t graph_for(int b) {
    if (graphs[b]) return graphs[b];
    hip_check(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal), "hipStreamBeginCapture");
    try {
      enqueue(m_obs, m_act, b, stream);
    } catch (...) {
      hipGraph_t g = nullptr;
      (void)hipStreamEndCapture(stream, &g);
      if (g) (void)hipGraphDestroy(g);
      throw;
    }
    hip_check(hipStreamEndCapture(stream, &graph_defs[b]), "hipStreamEndCapture");
    hip_check(hipGraphInstantiate(&graphs[b], graph_defs[b], nullptr, nullptr, 0), "hipGraphInstantiate");
    return graphs[b];
  }
};

namespace {

// Live resident kernels of every engine in the process, by device. A resident
// kernel holds its workgroups' CUs while it waits for requests; a batched launch
// (which wants all 256 CUs, one workgroup each) on the same device then runs in two
// rounds: measured 37.8 -> 71.4 us per 4096-robot step (tools/interference.py,
// DESIGN §4.2b). So every batched launch first tells the other engines' live
// resident kernels on its device to leave (a LEAVE header; no wait), and their
// next act() relaunches.
std::vector<go2pi_engine *> g_res_engines;

void res_register(go2pi_engine *e) {
  std::lock_guard<std::mutex> lk(g_res_mu);
  g_res_engines.push_back(e);
}

void res_unregister(go2pi_engine *e) {
  std::lock_guard<std::mutex> lk(g_res_mu);
  g_res_engines.erase(std::remove(g_res_engines.begin(), g_res_engines.end(), e), g_res_engines.end());
}

// The batched-launch counter of each device (DevProgram::yield), one per process
// and device, never freed (hipFree would synchronise the device).
unsigned *yield_word(int device) {
  static std::mutex mu;
  static std::vector<unsigned *> words;
  std::lock_guard<std::mutex> lk(mu);
  if ((int)words.size() <= device) words.resize(device + 1, nullptr);
  if (!words[device]) {
    void *p = nullptr;
    hip_check(hipMalloc(&p, 256), "hipMalloc");
    hip_check(hipMemset(p, 0, 256), "hipMemset");
    words[device] = static_cast<unsigned *>(p);
  }
  return words[device];
}

// batch: the rows of the launch that follows (one 16-row workgroup each); a launch of
// at most GO2PI_YIELD_MIN_GRID workgroups fits beside the resident kernels and evicts
// none (the kernels' own yield bump has the same bound, program.hpp).
// The lock comes back held: the caller keeps it until its batched launch is enqueued.
// A resident kernel another thread relaunched in between (resident_start takes the same
// lock) could otherwise sit ahead of that launch in a hardware queue two streams share,
// and serve its own requests until it idles out while the launch waits behind it (it
// leaves on the launch's yield bump only once the launch has started).
std::unique_lock<std::mutex> evict_residents(const go2pi_engine *self, int64_t batch) {
  if ((batch + GO2PI_TILE_ROWS - 1) / GO2PI_TILE_ROWS <= GO2PI_YIELD_MIN_GRID) return {};
  std::unique_lock<std::mutex> lk(g_res_mu);
  for (go2pi_engine *o : g_res_engines)
    if (o != self && o->device == self->device && o->res_flag.load() == 1)
      __atomic_store_n(o->h_req, (unsigned long long)GO2PI_RES_LEAVE << 32, __ATOMIC_SEQ_CST);
  return lk;
}

void set_ctl_params(go2pi_engine &e, const go2pi_ctl_params &cp) {
  go2pi::DevCtlParams d{};
  for (int i = 0; i < GO2PI_CTL_DOF; ++i) d.q0[i] = cp.q0[i];
  d.action_scale = cp.action_scale;
  d.kp_run = (double)cp.kp;  // float members widened at send_command (controller.cpp:246-247)
  d.kd_run = (double)cp.kd;
  d.kp_stop = (double)cp.kp_stop;
  d.action_limit = cp.action_limit;
  d.contact_threshold = cp.contact_threshold;
  for (int i = 0; i < 3; ++i) d.gravity_w[i] = cp.gravity_w[i];
  d.hist = e.ctl_hist;
  hip_check(hipMemcpy(e.d_ctl, &d, sizeof(d), hipMemcpyHostToDevice), "hipMemcpy");
}

// Engine creation, the straight-line part: every choice is the planner's (plan.cpp); here
// its buffers are uploaded and what it says is allocated.
void build(go2pi_engine &e, const uint8_t *bytes, size_t n, const go2pi_opts *o) {
  const Switches &sw = e.sw = Switches::read();
  go2pi_default_opts(&e.opts);
  if (o) {
    if (o->struct_size < (int32_t)offsetof(go2pi_opts, obs_mean))
      throw ApiError("go2pi_opts.struct_size too small", GO2PI_E_INVALID);
    std::memcpy(&e.opts, o, std::min<size_t>(sizeof(go2pi_opts), (size_t)o->struct_size));
    e.opts.struct_size = sizeof(go2pi_opts);
  }
  if (e.opts.max_batch <= 0) e.opts.max_batch = 4096;
  if (e.opts.max_batch > (int64_t)std::numeric_limits<int>::max() / 2)
    throw ApiError("max_batch too large", GO2PI_E_INVALID);
  try {
    e.model = go2pi::parse_onnx(bytes, n);
  } catch (const std::exception &ex) {
    throw ApiError(ex.what(), GO2PI_E_MODEL);
  }
  const auto &m = e.model;
  go2pi::check_model(m);

  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    throw ApiError("no HIP device available (go2pi has no CPU fallback)", GO2PI_E_DEVICE);
  if (e.opts.device < 0 || e.opts.device >= ndev)
    throw ApiError("device ordinal " + std::to_string(e.opts.device) + " out of range", GO2PI_E_INVALID);
  e.device = e.opts.device;
  hip_check(hipSetDevice(e.device), "hipSetDevice");
  hip_check(hipStreamCreateWithFlags(&e.stream, hipStreamNonBlocking), "hipStreamCreate");

  const go2pi::Plan plan = go2pi::plan_program(m, e.opts, sw);
  const go2pi::HostBuffers &buf = plan.buf;
  go2pi::DevProgram &p = e.prog = plan.prog;
  e.waves = plan.waves;
  e.small_batch = plan.small_batch;
  const int maxw = e.tmp_stride = plan.tmp_stride;
  e.latency_ok = plan.latency_ok;
  e.done_ok = plan.done_ok;
  e.ctl_hist = plan.ctl_hist;
  e.cost = plan.cost;

  // the plan's buffers to device memory, the program's pointers to them (empty: null)
  auto opt_upload = [&](const std::vector<float> &v) { return v.empty() ? nullptr : e.upload(v); };
  for (int l = 0; l < p.nl; ++l) {
    p.L[l].bias = e.upload(buf.bias[l]);
    p.L[l].ln_g = opt_upload(buf.ln_g[l]);
    p.L[l].ln_b = opt_upload(buf.ln_b[l]);
    p.skip_idx[l] = buf.skip[l].empty() ? nullptr : e.upload(buf.skip[l]);  // the index table, beside the biases
  }
  const float *base = e.upload(buf.arena);
  for (int l = 0; l < p.nl; ++l) p.L[l].w = base + buf.off[l];
  if (p.has_gru) {
    p.gru.w = e.upload(buf.gru_w);
    p.gru.bzr = e.upload(buf.gru_bzr);
    p.gru.bh = e.upload(buf.gru_bh);
    const size_t nh = (size_t)e.opts.max_batch * p.gru.sw;
    e.d_hidden = e.dalloc<float>(nh);
    hip_check(hipMemsetAsync(e.d_hidden, 0, nh * sizeof(float), e.stream), "hipMemsetAsync");
  }
  p.w4_bpack = opt_upload(buf.bpack);
  const float *lnpack = opt_upload(buf.lnpack);  // the LN pipeline's pack (program.hpp w4ln_tpw)
  p.pre_sub = opt_upload(buf.pre_sub);
  p.pre_div = opt_upload(buf.pre_div);
  p.pre_mul = opt_upload(buf.pre_mul);

  // buffers
  e.d_obs = e.dalloc<float>((size_t)e.opts.max_batch * m.in_dim);
  e.d_act = e.dalloc<float>((size_t)e.opts.max_batch * m.out_dim);
  e.d_tmp[0] = e.dalloc<float>((size_t)GO2PI_SMALL_MAXB * maxw);
  e.d_tmp[1] = e.dalloc<float>((size_t)GO2PI_SMALL_MAXB * maxw);
  if (plan.has_res)
    for (float *&c : e.d_carry) {
      c = e.dalloc<float>((size_t)GO2PI_SMALL_MAXB * maxw);
      hip_check(hipMemsetAsync(c, 0, sizeof(float) * GO2PI_SMALL_MAXB * maxw, e.stream), "hipMemsetAsync");
    }
  e.palloc(&e.h_obs, &e.m_obs, sizeof(float) * GO2PI_SMALL_MAXB * m.in_dim);
  e.palloc(&e.h_act, &e.m_act, sizeof(float) * GO2PI_SMALL_MAXB * m.out_dim);
  e.palloc(&e.h_err, &e.m_err, 512);
  p.err = e.m_err + 64;  // batched kernel hand-off timeouts
  if (plan.latency_ok || plan.res_rnn) {
    e.gstride = GO2PI_SMALL_MAXB * maxw;
    const size_t ng = (size_t)std::max(1, p.nl - 1) * e.gstride;
    e.d_gran = e.dalloc<unsigned long long>(ng);
    hip_check(hipMemsetAsync(e.d_gran, 0, ng * sizeof(unsigned long long), e.stream), "hipMemsetAsync");
    e.h_done = e.h_err + 32;  // 128 B apart: its own cache line
    e.m_done = e.m_err + 32;
  }
  if (plan.res_rnn && plan.done_ok) e.d_hgran = e.dalloc<unsigned long long>(2 * (size_t)GO2PI_SMALL_MAXB * p.gru.H);
  // resident path: the latency kernel's program shape, the request ring in host memory
  if (plan.resident(e.opts)) {
    // room for a controller tick's rows too (GO2PI_CTL_RAW + in_dim floats per robot)
    const size_t nreq = 1 + GO2PI_SMALL_MAXB * (size_t)(m.in_dim + GO2PI_CTL_RAW);
    size_t rb = sizeof(unsigned long long) * nreq;
    if (void *bar = bar_take(e.device, rb, sw.req_host)) {  // large BAR: the ring in VRAM, written by the host
      e.h_req = e.m_req = static_cast<unsigned long long *>(bar);
      e.req_bar_bytes = rb;
    } else {
      e.palloc(&e.h_req, &e.m_req, sizeof(unsigned long long) * nreq);
    }
    // (the controller form's answer granules too: ctl_gran)
    e.n_actg = std::max((size_t)GO2PI_SMALL_MAXB * m.out_dim, (size_t)go2pi::ctl_gran(m.in_dim).total);
    e.palloc(&e.h_actg, &e.m_actg, sizeof(unsigned long long) * e.n_actg);
    e.d_mirror = e.dalloc<unsigned long long>(1 + GO2PI_SMALL_MAXB * (size_t)m.in_dim);
    int khz = 0;
    hip_check(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, e.device), "hipDeviceGetAttribute");
    if (khz <= 0) khz = 100000;
    e.res_idle_ticks = (unsigned long long)e.opts.resident_ms * (unsigned long long)khz;
    e.resident_ok = true;
    res_register(&e);
  }
  // GO2PI_EPOCH0=<u32>: the engine's first granule tag instead of 1 (diagnostics and tests: a
  // value near 2^32 puts the tag-space wrap of next_epoch / resident_serve a few calls away
  // instead of ~1e9; 0, the empty granule's tag, is ignored)
  if (sw.epoch0) e.epoch = sw.epoch0;
  if (sw.diag_stamps) {  // diagnostics: per-workgroup clock stamps
    e.n_stamps = GO2PI_STAMPS_PER_WG * ((e.opts.max_batch + GO2PI_TILE_ROWS - 1) / GO2PI_TILE_ROWS);
    p.stamps = e.dalloc<unsigned long long>(e.n_stamps);
    hip_check(hipMemsetAsync(p.stamps, 0, e.n_stamps * sizeof(unsigned long long), e.stream), "hipMemsetAsync");
  }
  {
    float *z = e.dalloc<float>(64);
    hip_check(hipMemsetAsync(z, 0, 64 * sizeof(float), e.stream), "hipMemsetAsync");
    p.zero = z;
  }
  if (e.ctl_hist) {  // controller tick
    e.d_ctl = e.dalloc<go2pi::DevCtlParams>(1);
    go2pi_ctl_params cp;
    go2pi_ctl_default_params(&cp);
    set_ctl_params(e, cp);
  }
  p.yield = yield_word(e.device);
  go2pi::fill_hot_block(p);  // (every pointer it mirrors is set)
  if (p.w4ln_tpw) p.bpack = lnpack;

  const go2pi::ResForms res = go2pi::plan_resident(plan, sw, e.resident_ok, e.req_bar_bytes > 0);
  e.res_act = res.act;
  e.res_ctl = res.ctl;
  hip_check(go2pi::configure_kernels(p, e.waves), "hipFuncSetAttribute");
  // the finished program, copied to device memory (what every kernel reads)
  e.d_prog = e.dalloc<go2pi::DevProgram>(1);
  hip_check(hipMemcpy(e.d_prog, &p, sizeof(p), hipMemcpyHostToDevice), "hipMemcpy");
  // (not hipDeviceSynchronize: that would wait for other engines' resident kernels)
  hip_check(hipStreamSynchronize(e.stream), "hipStreamSynchronize");
  hip_check(hipStreamSynchronize(nullptr), "hipStreamSynchronize");
}

// Every C-ABI entry point runs through here: exceptions become status codes, and
// the caller's current HIP device is restored on the way out.
// (no DeviceRestore: go2pi_run's resident fast path, which switches devices lazily)
template <class F>
int guarded_nodev(F &&f) {
  try {
    g_last_error.clear();
    return f();
  } catch (const ApiError &ex) {
    g_last_error = ex.what();
    return ex.code;
  } catch (const HipError &ex) {
    g_last_error = ex.what();
    return ex.code;
  } catch (const std::bad_alloc &) {
    g_last_error = "out of host memory";
    return GO2PI_E_INVALID;
  } catch (const std::exception &ex) {
    g_last_error = ex.what();
    return GO2PI_E_INVALID;
  }
}

template <class F>
int guarded(F &&f) {
  DeviceRestore keep;
  return guarded_nodev(f);
}

void check_engine(const go2pi_engine *e) {
  if (!e) throw ApiError("null engine", GO2PI_E_INVALID);
}
// Mutating calls: the resident kernel (if any) leaves first, so the stream is free.
void check_engine(go2pi_engine *e) {
  if (!e) throw ApiError("null engine", GO2PI_E_INVALID);
  (void)hipSetDevice(e->device);
  e->resident_stop();
}

void check_batch(const go2pi_engine *e, int64_t batch) {
  if (batch < 0) throw ApiError("negative batch", GO2PI_E_INVALID);
  if (batch > e->opts.max_batch)
    throw ApiError("batch " + std::to_string(batch) + " exceeds max_batch " + std::to_string(e->opts.max_batch),
                   GO2PI_E_CAPACITY);
}

}  // namespace

extern "C" {

void go2pi_default_opts(go2pi_opts *o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->struct_size = sizeof(go2pi_opts);
  o->device = 0;
  o->max_batch = 4096;
  o->use_graph = 1;
  o->log_level = 2;
  o->waves = 0;
  o->small_batch = 0;
  o->obs_clip = 0.f;
  o->action_tanh = 0;
  o->action_clip = 0.f;
  o->action_scale = 0.f;
  o->ln_small = 0;
}

int go2pi_create_from_memory(const void *bytes, size_t nbytes, const go2pi_opts *opts, go2pi_engine **out) {
  return guarded([&] {
    if (!out) throw ApiError("null output pointer", GO2PI_E_INVALID);
    *out = nullptr;
    if (!bytes || !nbytes) throw ApiError("empty model buffer", GO2PI_E_MODEL);
    auto e = std::make_unique<go2pi_engine>();
    build(*e, static_cast<const uint8_t *>(bytes), nbytes, opts);
    *out = e.release();
    return GO2PI_OK;
  });
}

int go2pi_create(const char *path, const go2pi_opts *opts, go2pi_engine **out) {
  return guarded([&] {
    if (!out) throw ApiError("null output pointer", GO2PI_E_INVALID);
    *out = nullptr;
    if (!path) throw ApiError("null model path", GO2PI_E_INVALID);
    std::ifstream f(path, std::ios::binary);
    if (!f) throw ApiError(std::string("cannot open model file '") + path + "'", GO2PI_E_MODEL);
    std::vector<uint8_t> buf((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    if (buf.empty()) throw ApiError(std::string("empty model file '") + path + "'", GO2PI_E_MODEL);
    auto e = std::make_unique<go2pi_engine>();
    build(*e, buf.data(), buf.size(), opts);
    *out = e.release();
    return GO2PI_OK;
  });
}

void go2pi_destroy(go2pi_engine *e) { delete e; }

int go2pi_num_io(const go2pi_engine *e, int32_t *ni, int32_t *no) {
  return guarded([&] {
    check_engine(e);
    if (ni) *ni = (int32_t)e->model.inputs.size();
    if (no) *no = (int32_t)e->model.outputs.size();
    return GO2PI_OK;
  });
}

int go2pi_io_name(const go2pi_engine *e, int32_t is_output, int32_t index, char *buf, size_t cap) {
  return guarded([&] {
    check_engine(e);
    const auto &v = is_output ? e->model.outputs : e->model.inputs;
    if (index < 0 || index >= (int32_t)v.size()) throw ApiError("io index out of range", GO2PI_E_INVALID);
    if (!buf || cap == 0) throw ApiError("null name buffer", GO2PI_E_INVALID);
    const std::string &s = v[index].name;
    const size_t k = std::min(cap - 1, s.size());
    std::memcpy(buf, s.data(), k);
    buf[k] = 0;
    return GO2PI_OK;
  });
}

int go2pi_io_shape(const go2pi_engine *e, int32_t is_output, int32_t index, int64_t *dims, int32_t cap,
                   int32_t *rank) {
  return guarded([&] {
    check_engine(e);
    const auto &v = is_output ? e->model.outputs : e->model.inputs;
    if (index < 0 || index >= (int32_t)v.size()) throw ApiError("io index out of range", GO2PI_E_INVALID);
    const auto &s = v[index].shape;
    if (rank) *rank = (int32_t)s.size();
    for (int32_t i = 0; dims && i < cap && i < (int32_t)s.size(); ++i) dims[i] = s[i];
    return GO2PI_OK;
  });
}

int go2pi_io_dims(const go2pi_engine *e, int64_t *in_dim, int64_t *out_dim) {
  return guarded([&] {
    check_engine(e);
    if (in_dim) *in_dim = e->model.in_dim;
    if (out_dim) *out_dim = e->model.out_dim;
    return GO2PI_OK;
  });
}

int go2pi_run(go2pi_engine *e, const float *obs, float *act, int64_t batch) {
  // batch <= 8 on a live resident kernel: served with no HIP runtime call (the device
  // switch and its restore were three HIP API entries per act(), on the 5 us path).
  // Invariant: this skips check_engine / check_batch because a live kernel
  // (resident_ready: resident_live) exists only after an earlier call on this engine
  // passed them in the guarded path below (resident_start is reached from there only),
  // and the fields read here (opts, resident_ok, model dims) never change after build.
  // The batch bounds are re-checked in the condition itself.
  bool res_try = true;
  if (e && obs && act && batch >= 1 && batch <= GO2PI_SMALL_MAXB && batch <= e->opts.max_batch && e->resident_ok &&
      e->resident_ready(nullptr)) {
    e->lazy_dev = true;
    const int rc = guarded_nodev([&] { return e->resident_act(obs, act, batch) ? GO2PI_OK : 1; });
    e->dev_done();
    if (rc != 1) return rc;
    res_try = false;  // not served (evicted twice): a launch serves it
  }
  return guarded([&] {
    check_engine(static_cast<const go2pi_engine *>(e));
    check_batch(e, batch);
    if (batch == 0) return GO2PI_OK;
    if (!obs || !act) throw ApiError("null obs/act buffer", GO2PI_E_INVALID);
    hip_check(hipSetDevice(e->device), "hipSetDevice");
    if (res_try && e->resident_ok && batch <= GO2PI_SMALL_MAXB && e->resident_act(obs, act, batch)) return GO2PI_OK;
    e->resident_stop();
    std::unique_lock<std::mutex> ev;  // (held until the launch below is enqueued)
    if (batch > GO2PI_SMALL_MAXB || !e->latency_ok) ev = evict_residents(e, batch);  // a batched (fused) launch follows
    const size_t in_b = sizeof(float) * (size_t)batch * e->model.in_dim;
    const size_t out_b = sizeof(float) * (size_t)batch * e->model.out_dim;
    if (batch <= GO2PI_SMALL_MAXB) {
      // pinned host-mapped staging: kernels read obs / write act over PCIe directly
      std::memcpy(e->h_obs, obs, in_b);
      bool synced = false;
      if (e->use_latency(batch)) {
        // one direct launch (per-call epoch argument); completion observed by spinning on
        // the host-mapped done word (a stream sync costs ~10 us more on this stack)
        e->enqueue(e->m_obs, e->m_act, batch, e->stream, e->done_ok ? e->m_done : nullptr);
        if (e->done_ok) synced = e->spin_done();
      } else if (!e->opts.use_graph) {
        e->enqueue(e->m_obs, e->m_act, batch, e->stream);
      } else {
        hip_check(hipGraphLaunch(e->graph_for((int)batch), e->stream), "hipGraphLaunch");
      }
      if (ev.owns_lock()) ev.unlock();  // (the launch is enqueued)
      if (!synced) hip_check(hipStreamSynchronize(e->stream), "hipStreamSynchronize");
      e->check_handoff();
      std::memcpy(act, e->h_act, out_b);
    } else {
      hip_check(hipMemcpyAsync(e->d_obs, obs, in_b, hipMemcpyHostToDevice, e->stream), "hipMemcpyAsync H2D");
      e->enqueue(e->d_obs, e->d_act, batch, e->stream);
      if (ev.owns_lock()) ev.unlock();  // (the launch is enqueued)
      hip_check(hipMemcpyAsync(act, e->d_act, out_b, hipMemcpyDeviceToHost, e->stream), "hipMemcpyAsync D2H");
      hip_check(hipStreamSynchronize(e->stream), "hipStreamSynchronize");
      e->check_handoff();
    }
    return GO2PI_OK;
  });
}

int go2pi_run_device(go2pi_engine *e, const float *obs_dev, float *act_dev, int64_t batch, void *hip_stream) {
  return guarded([&] {
    check_engine(e);
    check_batch(e, batch);
    if (batch == 0) return GO2PI_OK;
    if (!obs_dev || !act_dev) throw ApiError("null obs/act buffer", GO2PI_E_INVALID);
    hip_check(hipSetDevice(e->device), "hipSetDevice");
    e->check_handoff();  // a failure of an earlier asynchronous launch surfaces here (or at go2pi_sync)
    std::unique_lock<std::mutex> ev;  // (held until the launch is enqueued)
    if (!e->use_latency(batch)) ev = evict_residents(e, batch);
    e->enqueue(obs_dev, act_dev, batch, static_cast<hipStream_t>(hip_stream));
    return GO2PI_OK;
  });
}

int go2pi_run_sequence_device(go2pi_engine *e, const float *obs_dev, float *act_dev, int64_t steps, int64_t batch,
                              void *hip_stream) {
  return guarded([&] {
    check_engine(e);
    check_batch(e, batch);
    if (steps < 0) throw ApiError("negative steps", GO2PI_E_INVALID);
    if (batch == 0 || steps == 0) return GO2PI_OK;
    if (!obs_dev || !act_dev) throw ApiError("null obs/act buffer", GO2PI_E_INVALID);
    if ((double)steps * batch * std::max(e->model.in_dim, e->model.out_dim) > 2147483647.0 * 4)
      throw ApiError("sequence too large", GO2PI_E_INVALID);
    hip_check(hipSetDevice(e->device), "hipSetDevice");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const auto ev = evict_residents(e, batch);  // (held until the launch is enqueued)
    hip_check(go2pi::launch_policy_fused(e->prog, e->d_prog, e->waves, obs_dev, act_dev, e->d_hidden, (int)batch,
                                         (int)steps, s),
              "fused sequence launch");
    return GO2PI_OK;
  });
}

int go2pi_hidden_dim(const go2pi_engine *e, int64_t *hd) {
  return guarded([&] {
    check_engine(e);
    if (hd) *hd = e->model.has_gru ? e->prog.gru.sw : 0;  // LSTM: h | c
    return GO2PI_OK;
  });
}

int go2pi_reset_hidden(go2pi_engine *e, const uint8_t *mask, int64_t batch) {
  return guarded([&] {
    check_engine(e);
    if (!e->model.has_gru) return GO2PI_OK;
    hip_check(hipSetDevice(e->device), "hipSetDevice");
    const int H = e->prog.gru.sw;  // state floats per robot
    if (!mask) {
      hip_check(hipMemsetAsync(e->d_hidden, 0, sizeof(float) * (size_t)e->opts.max_batch * H, e->stream), "hipMemsetAsync");
    } else {
      check_batch(e, batch);
      // coalesce runs of reset rows into single memsets
      int64_t i = 0;
      while (i < batch) {
        if (!mask[i]) { ++i; continue; }
        int64_t j = i;
        while (j < batch && mask[j]) ++j;
        hip_check(hipMemsetAsync(e->d_hidden + (size_t)i * H, 0, sizeof(float) * (size_t)(j - i) * H, e->stream),
                  "hipMemsetAsync");
        i = j;
      }
    }
    hip_check(hipStreamSynchronize(e->stream), "hipStreamSynchronize");
    return GO2PI_OK;
  });
}

int go2pi_get_hidden(go2pi_engine *e, float *h, int64_t batch) {
  return guarded([&] {
    check_engine(e);
    check_batch(e, batch);
    if (!e->model.has_gru || batch == 0) return GO2PI_OK;
    if (!h) throw ApiError("null hidden buffer", GO2PI_E_INVALID);
    hip_check(hipSetDevice(e->device), "hipSetDevice");
    hip_check(hipStreamSynchronize(e->stream), "hipStreamSynchronize");
    hip_check(hipMemcpy(h, e->d_hidden, sizeof(float) * (size_t)batch * e->prog.gru.sw, hipMemcpyDeviceToHost),
              "hipMemcpy D2H");
    return GO2PI_OK;
  });
}

int go2pi_set_hidden(go2pi_engine *e, const float *h, int64_t batch) {
  return guarded([&] {
    check_engine(e);
    check_batch(e, batch);
    if (!e->model.has_gru || batch == 0) return GO2PI_OK;
    if (!h) throw ApiError("null hidden buffer", GO2PI_E_INVALID);
    hip_check(hipSetDevice(e->device), "hipSetDevice");
    hip_check(hipStreamSynchronize(e->stream), "hipStreamSynchronize");
    hip_check(hipMemcpy(e->d_hidden, h, sizeof(float) * (size_t)batch * e->prog.gru.sw, hipMemcpyHostToDevice),
              "hipMemcpy H2D");
    return GO2PI_OK;
  });
}

void go2pi_ctl_default_params(go2pi_ctl_params *p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->struct_size = sizeof(go2pi_ctl_params);
  p->kp = 28.f;  // controller.hpp:119-120
  p->kd = 0.5f;
  p->kp_stop = 5.f;           // controller.cpp:246
  p->action_limit = 1000.f;   // kActionLimit, controller.hpp:17
  p->contact_threshold = 22.f;  // controller.hpp:100-103
  p->gravity_w[2] = -1.f;     // gravity_w_, controller.hpp:131
  p->action_scale = 0.25;     // controller.cpp:244
  static const double q0[12] = {0.1, -0.1, 0.1, -0.1, 0.8, 0.8, 1.0, 1.0, -1.5, -1.5, -1.5, -1.5};  // controller.hpp:165
  std::memcpy(p->q0, q0, sizeof(q0));
}

int go2pi_ctl_history(const go2pi_engine *e, int32_t *hist) {
  return guarded([&] {
    check_engine(e);
    if (!e->ctl_hist)
      throw ApiError("policy I/O is not a Go2 controller's (obs " + std::to_string(e->model.in_dim) +
                         " not a multiple of 49, or action " + std::to_string(e->model.out_dim) + " != 12)",
                     GO2PI_E_MODEL);
    if (hist) *hist = e->ctl_hist;
    return GO2PI_OK;
  });
}

int go2pi_ctl_set_params(go2pi_engine *e, const go2pi_ctl_params *p) {
  return guarded([&] {
    check_engine(e);
    if (!p) throw ApiError("null params", GO2PI_E_INVALID);
    if (p->struct_size != (int32_t)sizeof(go2pi_ctl_params))
      throw ApiError("go2pi_ctl_params.struct_size mismatch", GO2PI_E_INVALID);
    if (!e->ctl_hist) throw ApiError("policy I/O is not a Go2 controller's", GO2PI_E_MODEL);
    hip_check(hipSetDevice(e->device), "hipSetDevice");
    hip_check(hipStreamSynchronize(e->stream), "hipStreamSynchronize");
    set_ctl_params(*e, *p);
    return GO2PI_OK;
  });
}

}  // extern "C"

namespace {
// byte offsets of the controller staging buffers for `rows` robots (256 B aligned)
struct CtlLayout {
  size_t state, joy, obs, action, q_des, kp, kd, status, total;
  CtlLayout(int64_t rows, int in_dim) {
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    size_t o = 0;
    state = o; o = al(o + sizeof(float) * rows * GO2PI_CTL_STATE_DIM);
    joy = o; o = al(o + sizeof(float) * rows * GO2PI_CTL_JOY_DIM);
    obs = o; o = al(o + sizeof(float) * rows * in_dim);
    action = o; o = al(o + sizeof(float) * rows * GO2PI_CTL_DOF);
    q_des = o; o = al(o + sizeof(double) * rows * GO2PI_CTL_DOF);
    kp = o; o = al(o + sizeof(double) * rows * GO2PI_CTL_DOF);
    kd = o; o = al(o + sizeof(double) * rows * GO2PI_CTL_DOF);
    status = o; o = al(o + sizeof(uint32_t) * rows);
    total = o;
  }
};

void check_ctl(const go2pi_engine *e, int64_t batch) {
  check_engine(e);
  check_batch(e, batch);
  if (!e->ctl_hist) throw ApiError("policy I/O is not a Go2 controller's (need 49*k obs, 12 actions)", GO2PI_E_MODEL);
  // (the tick's observation is assembled in LDS and published in place; a skip layer reads
  // the observation rows from memory)
  // (nor has any controller form a carried tile)
  if (go2pi::program_has_res(e->prog))
    throw ApiError("the controller tick does not serve a policy with residual connections "
                   "(assemble the observation and call go2pi_run)", GO2PI_E_INVALID);
  if (go2pi::program_has_skip(e->prog))
    throw ApiError("the controller tick does not serve a policy with observation skip inputs "
                   "(assemble the observation and call go2pi_run)", GO2PI_E_INVALID);
}

// One go2pi_controller_step call: the caller's rows, their byte counts, and how they
// travel (the staging laid out by a CtlLayout, or the resident kernel's request). On the
// stack: go2pi_controller_step's fast path allocates nothing.
struct CtlCall {
  const float *state, *joy;
  float *obs, *action;
  double *q_des, *kp, *kd;
  uint32_t *status;
  int64_t batch;
  int in_dim;
  size_t n_state = sizeof(float) * batch * GO2PI_CTL_STATE_DIM, n_joy = sizeof(float) * batch * GO2PI_CTL_JOY_DIM;
  size_t n_obs = sizeof(float) * batch * in_dim, n_act = sizeof(float) * batch * GO2PI_CTL_DOF;
  size_t n_d = sizeof(double) * batch * GO2PI_CTL_DOF, n_st = sizeof(uint32_t) * batch;

  // the optional rows this call passed, as the resident request's header says it
  unsigned flags() const {
    return (joy ? GO2PI_RES_JOY : 0u) | (q_des ? GO2PI_RES_QDES : 0u) | (kp ? GO2PI_RES_KP : 0u) |
           (kd ? GO2PI_RES_KD : 0u) | (status ? GO2PI_RES_STATUS : 0u);
  }
  // the resident request's rows: state | joystick | obs | action (no joystick: zeros)
  void pack(float *rows) const {
    std::memcpy(rows, state, n_state);
    if (joy) std::memcpy(rows + batch * GO2PI_CTL_STATE_DIM, joy, n_joy);
    else std::memset(rows + batch * GO2PI_CTL_STATE_DIM, 0, n_joy);
    std::memcpy(rows + batch * (GO2PI_CTL_STATE_DIM + GO2PI_CTL_JOY_DIM), obs, n_obs);
    std::memcpy(rows + batch * (GO2PI_CTL_STATE_DIM + GO2PI_CTL_JOY_DIM + in_dim), action, n_act);
  }
  // The kernels' view of the staging at `dev`. all: every optional row has its place (the
  // resident kernel's controller form: the request's flags say which this call passed);
  // else the optional rows as passed.
  go2pi::DevCtl view(const go2pi::DevCtlParams *prm, char *dev, const CtlLayout &L, bool all) const {
    go2pi::DevCtl c{};
    c.prm = prm;
    c.state = reinterpret_cast<const float *>(dev + L.state);
    c.joy = (all || joy) ? reinterpret_cast<const float *>(dev + L.joy) : nullptr;
    c.obs = reinterpret_cast<float *>(dev + L.obs);
    c.action = reinterpret_cast<float *>(dev + L.action);
    c.q_des = (all || q_des) ? reinterpret_cast<double *>(dev + L.q_des) : nullptr;
    c.kp = (all || kp) ? reinterpret_cast<double *>(dev + L.kp) : nullptr;
    c.kd = (all || kd) ? reinterpret_cast<double *>(dev + L.kd) : nullptr;
    c.status = (all || status) ? reinterpret_cast<uint32_t *>(dev + L.status) : nullptr;
    return c;
  }
  // the inputs into the staging: put(offset, source, bytes)
  template <class F>
  void put(const CtlLayout &L, F &&f) const {
    f(L.state, state, n_state);
    if (joy) f(L.joy, joy, n_joy);
    f(L.obs, obs, n_obs);
    f(L.action, action, n_act);
  }
  // the answers out of the staging: take(destination, offset, bytes)
  template <class F>
  void take(const CtlLayout &L, F &&f) const {
    f(obs, L.obs, n_obs);
    f(action, L.action, n_act);
    if (q_des) f(q_des, L.q_des, n_d);
    if (kp) f(kp, L.kp, n_d);
    if (kd) f(kd, L.kd, n_d);
    if (status) f(status, L.status, n_st);
  }
  void take_host(const CtlLayout &L, const char *stage) const {
    take(L, [&](void *dst, size_t off, size_t n) { std::memcpy(dst, stage + off, n); });
  }
};

// The tick by the resident kernel's controller form (batch <= GO2PI_SMALL_MAXB; all: the
// all-rows view of the pinned staging, laid out by L), its answers into the caller's
// buffers; false: not served (resident_serve). No HIP runtime call while a live kernel serves it.
bool resident_tick(go2pi_engine *e, const CtlCall &c, const CtlLayout &L, const go2pi::DevCtl &all) {
  float *rows = e->res_rows.data();
  c.pack(rows);
  if (!e->resident_serve(&all, rows, c.batch, c.flags())) return false;
  e->check_handoff();
  if (e->res_ctl == ResForm::Act1) e->ctl_take(c.batch, c.obs, c.action, c.q_des, c.kp, c.kd, c.status);
  else c.take_host(L, e->h_ctl);
  return true;
}
}  // namespace

extern "C" {

int go2pi_controller_step(go2pi_engine *e, const float *state, const float *joy, float *obs, float *action,
                          double *q_des, double *kp, double *kd, uint32_t *status, int64_t batch) {
  // batch <= 8 on a live controller-form resident kernel: no HIP runtime call and no
  // input staging (the rows travel in the request itself; go2pi_run's fast path).
  // Invariant: check_ctl is skipped; the condition itself requires ctl_hist
  // (a controller policy: check_ctl's model test), the batch bounds and the staging
  // (h_ctl), and resident_ready(&all) requires a live controller-form kernel, which only
  // the guarded path below starts.
  bool res_try = true;
  if (e && state && obs && action && batch >= 1 && batch <= GO2PI_SMALL_MAXB && batch <= e->opts.max_batch &&
      e->ctl_hist && e->res_ctl != ResForm::None && e->h_ctl) {
    const CtlCall c{state, joy, obs, action, q_des, kp, kd, status, batch, e->model.in_dim};
    const CtlLayout L(GO2PI_SMALL_MAXB, c.in_dim);
    const go2pi::DevCtl all = c.view(e->d_ctl, e->m_ctl, L, true);
    if (e->resident_ready(&all)) {
      e->lazy_dev = true;
      const int rc = guarded_nodev([&] { return resident_tick(e, c, L, all) ? GO2PI_OK : 1; });
      e->dev_done();
      if (rc != 1) return rc;
      res_try = false;  // not served (evicted twice): a launch serves it
    }
  }
  return guarded([&] {
    check_ctl(e, batch);
    if (batch == 0) return GO2PI_OK;
    if (!state || !obs || !action) throw ApiError("null state/obs/action buffer", GO2PI_E_INVALID);
    hip_check(hipSetDevice(e->device), "hipSetDevice");
    const CtlCall c{state, joy, obs, action, q_des, kp, kd, status, batch, e->model.in_dim};
    const bool small = batch <= GO2PI_SMALL_MAXB;
    const CtlLayout L(small ? GO2PI_SMALL_MAXB : e->opts.max_batch, c.in_dim);
    char *dev;  // device-side view of the staging
    if (small) {
      if (!e->h_ctl) e->palloc(&e->h_ctl, &e->m_ctl, L.total);
      c.put(L, [&](size_t off, const void *src, size_t n) { std::memcpy(e->h_ctl + off, src, n); });
      dev = e->m_ctl;
    } else {
      if (!e->d_ctlbuf) e->d_ctlbuf = e->dalloc<char>(L.total);
      dev = e->d_ctlbuf;
      c.put(L, [&](size_t off, const void *src, size_t n) {
        hip_check(hipMemcpyAsync(dev + off, src, n, hipMemcpyHostToDevice, e->stream), "hipMemcpyAsync H2D");
      });
    }
    // the resident kernel's controller form (a request it does not serve: by a launch)
    if (res_try && small && e->res_ctl != ResForm::None && resident_tick(e, c, L, c.view(e->d_ctl, dev, L, true)))
      return GO2PI_OK;
    e->resident_stop();
    const bool single = small && e->use_latency(batch) && e->done_ok;
    std::unique_lock<std::mutex> ev;
    if (!single) ev = evict_residents(e, batch);  // a batched (fused) launch follows
    e->enqueue_ctl(c.view(e->d_ctl, dev, L, false), batch, e->stream, single ? e->m_done : nullptr);
    if (ev.owns_lock()) ev.unlock();  // (the launch is enqueued)
    if (small) {
      if (!(single && e->spin_done())) hip_check(hipStreamSynchronize(e->stream), "hipStreamSynchronize");
      e->check_handoff();
      c.take_host(L, e->h_ctl);
    } else {
      c.take(L, [&](void *dst, size_t off, size_t n) {
        hip_check(hipMemcpyAsync(dst, dev + off, n, hipMemcpyDeviceToHost, e->stream), "hipMemcpyAsync D2H");
      });
      hip_check(hipStreamSynchronize(e->stream), "hipStreamSynchronize");
    }
    return GO2PI_OK;
  });
}

int go2pi_controller_step_device(go2pi_engine *e, const float *state, const float *joy, float *obs, float *action,
                                 double *q_des, double *kp, double *kd, uint32_t *status, int64_t batch,
                                 void *hip_stream) {
  return guarded([&] {
    check_ctl(e, batch);
    if (batch == 0) return GO2PI_OK;
    if (!state || !obs || !action) throw ApiError("null state/obs/action buffer", GO2PI_E_INVALID);
    // the buffer contract (go2pi.h): the batched tick's head lane writes its four joints of
    // action, q_des, kp and kd with 16-byte stores (ctl_fn.hpp ctl_store4), straight to these
    // pointers; refused here, before anything is enqueued
    auto aligned16 = [](const void *p, const char *name) {
      if (reinterpret_cast<uintptr_t>(p) & 15)
        throw ApiError(std::string("go2pi_controller_step_device: ") + name + " must be 16-byte aligned",
                       GO2PI_E_INVALID);
    };
    aligned16(action, "action_dev");
    aligned16(q_des, "q_des_dev");
    aligned16(kp, "kp_dev");
    aligned16(kd, "kd_dev");
    hip_check(hipSetDevice(e->device), "hipSetDevice");
    // a live resident kernel shares the granules, epoch and error words the batch <= 8
    // launch uses: it leaves first (as for every other call on the engine)
    e->resident_stop();
    std::unique_lock<std::mutex> ev;  // (held until the launch is enqueued)
    if (!(e->use_latency(batch) && e->done_ok)) ev = evict_residents(e, batch);
    go2pi::DevCtl c{e->d_ctl, state, joy, obs, action, q_des, kp, kd, status};
    e->enqueue_ctl(c, batch, static_cast<hipStream_t>(hip_stream));
    return GO2PI_OK;
  });
}

int go2pi_sync(go2pi_engine *e) {
  return guarded([&] {
    check_engine(e);
    hip_check(hipSetDevice(e->device), "hipSetDevice");
    hip_check(hipStreamSynchronize(e->stream), "hipStreamSynchronize");
    e->check_handoff();
    return GO2PI_OK;
  });
}

int go2pi_get_cost(const go2pi_engine *e, go2pi_cost *c) {
  return guarded([&] {
    check_engine(e);
    if (!c) throw ApiError("null cost", GO2PI_E_INVALID);
    *c = e->cost;
    return GO2PI_OK;
  });
}

// The reported kernel names are printed by the launcher modules, each from the dispatch
// that launches (kernels.hip batched_kernel_name, resident.hip resident_kernel_name).
int go2pi_batched_kernel(const go2pi_engine *e, char *buf, size_t cap) {
  return guarded([&] {
    check_engine(e);
    if (!buf || cap == 0) throw ApiError("null buffer", GO2PI_E_INVALID);
    go2pi::batched_kernel_name(e->prog, e->waves, buf, cap);
    return GO2PI_OK;
  });
}

int go2pi_resident_kernel(const go2pi_engine *e, char *buf, size_t cap) {
  return guarded([&] {
    check_engine(e);
    if (!buf || cap == 0) throw ApiError("null buffer", GO2PI_E_INVALID);
    go2pi::resident_kernel_name(e->res_act, e->prog, e->req_bar_bytes > 0, buf, cap);
    return GO2PI_OK;
  });
}

int go2pi_small_kernel(const go2pi_engine *e, char *buf, size_t cap) {
  return guarded([&] {
    check_engine(e);
    if (!buf || cap == 0) throw ApiError("null buffer", GO2PI_E_INVALID);
    go2pi::small_kernel_name(e->prog, e->waves, e->small_batch, e->latency_ok, e->opts.use_graph, buf, cap);
    return GO2PI_OK;
  });
}

int go2pi_resident_launches(const go2pi_engine *e, int64_t *n) {
  return guarded([&] {
    check_engine(e);
    if (!n) throw ApiError("null argument", GO2PI_E_INVALID);
    *n = e->res_launches;
    return GO2PI_OK;
  });
}

int go2pi_inspect_model(const char *path, char *buf, size_t cap) {
  return guarded([&] {
    if (!path || !buf || cap == 0) throw ApiError("null argument", GO2PI_E_INVALID);
    std::ifstream f(path, std::ios::binary);
    if (!f) throw ApiError(std::string("cannot open model file '") + path + "'", GO2PI_E_MODEL);
    std::vector<uint8_t> bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    go2pi::Model m;
    try {
      m = go2pi::parse_onnx(bytes.data(), bytes.size());
    } catch (const std::exception &ex) {
      throw ApiError(ex.what(), GO2PI_E_MODEL);
    }
    const std::string j = go2pi::inspect_json(m);
    const size_t k = std::min(cap - 1, j.size());
    std::memcpy(buf, j.data(), k);
    buf[k] = 0;
    return (int)j.size();
  });
}

int go2pi_diag_stamps(go2pi_engine *e, uint64_t *out, int64_t n) {
  return guarded([&] {
    check_engine(e);
    if (!e->prog.stamps) throw ApiError("stamps disabled (set GO2PI_DIAG_STAMPS before create)", GO2PI_E_INVALID);
    if (!out || n < 0) throw ApiError("bad stamps buffer", GO2PI_E_INVALID);
    hip_check(hipSetDevice(e->device), "hipSetDevice");
    hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
    const int64_t k = std::min(n, e->n_stamps);
    hip_check(hipMemcpy(out, e->prog.stamps, k * sizeof(uint64_t), hipMemcpyDeviceToHost), "hipMemcpy");
    return (int)k;
  });
}

const char *go2pi_last_error(void) { return g_last_error.c_str(); }

const char *go2pi_version(void) { return "go2pi 0.1.0 (gfx950)"; }

}  // extern "C"
