// The engine's planner (internal): every choice an engine makes for its life, made from
// the parsed model, the options and the diagnostic switches alone. Pure host code: no
// device, no HIP call, so the kernel choice is checked without a GPU
// (tests/cpp/plan_probe.cpp, tests/test_cpu_plan.py). engine.cpp build() uploads what the
// plan holds and allocates what it says.
#pragma once

#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/go2pi.h"
#include "onnx_model.hpp"
#include "program.hpp"

namespace go2pi {

struct ApiError : std::runtime_error {
  int code;
  ApiError(const std::string &m, int c) : std::runtime_error(m), code(c) {}
};

// The process's diagnostic switches (GO2PI_* environment variables; DESIGN §4.5 lists
// them), read once per engine at the top of build(): every choice an engine makes from
// them is made by the planner and holds for its life. Except where noted a switch is on
// when the variable is set, to any value.
struct Switches {
  bool req_host;               // REQ_HOST: the request ring in pinned host memory (bar_take)
  bool no_head_fuse, no_w4;    // NO_HEAD_FUSE: no head fusion, and so no 4-wave pipeline; NO_W4: no pipeline
  bool k0_pad64;               // K0_PAD64: the pipeline's layer 0 padded to 64 columns, not 16
  bool small_chain;            // SMALL_CHAIN: batch <= 8 by the GEMV chain (no single launch, no resident form)
  unsigned epoch0;             // EPOCH0=<u32>: the first granule tag instead of 1; 0 (unset, out of range): ignored
  bool diag_stamps;            // DIAG_STAMPS: per-workgroup clock stamps
  bool no_plain;               // NO_PLAIN: the general pipeline body, not the lean kernel
  bool lean_rt_act, lean_rt_nh;  // LEAN_RT_ACT / _NH: the lean kernel's activation / layer count read at run time
  // GRU_GENERAL: the general body, not the lean recurrent tick (r05 same-box A/B, GRU-256 at
  // 4096 robots: 56.7 against 60.5-60.9 us per one-tick launch); CTL_GENERAL: ... not the lean controller tick
  bool gru_general, ctl_general;
  bool res_multi;              // RES_MULTI: the multi-workgroup resident kernel for every form
  bool res_r1w;                // RES_R1W: never policy_act1_kernel (r04's policy_resident1_kernel where it fits)
  bool res_tiled0;             // RES_TILED0: the multi-workgroup kernel's layer 0 tiled, not local
  int a1_depth, a1_cw;         // A1_DEPTH: policy_act1_kernel's poll sweeps in flight, 1 for the value 1, else 2;
                               // A1_CW: its compute waves, 4 for the value 4, else 8
  // SKIP_SMALL (opt-in, not a diagnostic): a policy with observation skip inputs at batch <= 8 by the
  // single launch and the multi-workgroup resident kernel, not the GEMV chain
  bool skip_small;
  // RESIDUAL_SMALL (opt-in, not a diagnostic; RES_* means "resident" here): a policy with residual connections
  // at batch <= 8 by the single launch and the multi-workgroup resident kernel, not the GEMV chain
  bool residual_small;
  // RESIDUAL_BATCHED (opt-in, not a diagnostic): a policy with residual connections of the 4-wave
  // pipeline's shape on policy_mlp_res_kernel for batched launches, not policy_fused_res_kernel<8>
  // (plan.cpp plan_program). An environment switch for RESIDUAL_SMALL's reason: go2pi_opts ends in ln_small
  bool residual_batched;

  static Switches read() {
    auto env = [](const char *name) { return std::getenv(name); };  // (the engine's only look at the environment)
    auto on = [&](const char *name) { return env(name) != nullptr; };
    auto num = [&](const char *name) { return env(name) ? std::atoi(env(name)) : 0; };
    const unsigned long long e0 = env("GO2PI_EPOCH0") ? std::strtoull(env("GO2PI_EPOCH0"), nullptr, 0) : 0ull;
    return Switches{.req_host = on("GO2PI_REQ_HOST"), .no_head_fuse = on("GO2PI_NO_HEAD_FUSE"),
                    .no_w4 = on("GO2PI_NO_W4"), .k0_pad64 = on("GO2PI_K0_PAD64"),
                    .small_chain = on("GO2PI_SMALL_CHAIN"), .epoch0 = e0 <= 0xFFFFFFFFull ? (unsigned)e0 : 0u,
                    .diag_stamps = on("GO2PI_DIAG_STAMPS"), .no_plain = on("GO2PI_NO_PLAIN"),
                    .lean_rt_act = on("GO2PI_LEAN_RT_ACT"), .lean_rt_nh = on("GO2PI_LEAN_RT_NH"),
                    .gru_general = on("GO2PI_GRU_GENERAL"), .ctl_general = on("GO2PI_CTL_GENERAL"),
                    .res_multi = on("GO2PI_RES_MULTI"), .res_r1w = on("GO2PI_RES_R1W"),
                    .res_tiled0 = on("GO2PI_RES_TILED0"), .a1_depth = num("GO2PI_A1_DEPTH") == 1 ? 1 : 2,
                    .a1_cw = num("GO2PI_A1_CW") == 4 ? 4 : 8, .skip_small = on("GO2PI_SKIP_SMALL"),
                    .residual_small = on("GO2PI_RESIDUAL_SMALL"),
                    .residual_batched = on("GO2PI_RESIDUAL_BATCHED")};
  }
};

// What the program's pointer fields will point to once build() has uploaded it; an
// empty vector: the pointer stays null.
struct HostBuffers {
  std::vector<float> arena;      // every dense layer's fragments back to back: L[l].w = base + off[l]
  std::vector<size_t> off;
  std::vector<float> bias[GO2PI_MAX_LAYERS], ln_g[GO2PI_MAX_LAYERS], ln_b[GO2PI_MAX_LAYERS];  // [N_pad] each
  std::vector<float> bpack;      // the pipeline's bias pack (w4_bpack): the hidden layers' biases back to back
  // the LN pipeline's pack (program.hpp w4ln_tpw): biases | Scale | B of the hidden layers; the residual
  // pipeline's too (zeros for Scale / B of a layer without LN)
  std::vector<float> lnpack;
  std::vector<float> gru_w, gru_bzr, gru_bh;
  std::vector<float> pre_sub, pre_div, pre_mul;
  std::vector<int> skip[GO2PI_MAX_LAYERS];  // each layer's observation column indices (DevProgram::skip_idx)
};

struct Plan {
  DevProgram prog{};     // every scalar field final; every pointer field null
  HostBuffers buf;
  int waves = 8;         // waves per workgroup of the batched kernel
  int small_batch = 8;   // host batches <= this take the small-batch path (0: never)
  int tmp_stride = 0;    // the widest padded layer: floats per row of the small-batch buffers
  int ctl_hist = 0;      // kHistory when the policy's I/O is a Go2 controller's, else 0
  bool latency_shape = false;  // the single launch's grid and register slots hold every layer
  bool latency_ok = false;     // batch <= GO2PI_SMALL_MAXB by the single launch (policy_latency_kernel)
  bool res_rnn = false;        // the resident kernel's GRU / LSTM form applies
  bool done_ok = false;        // the final layer is one tile: workgroup 0 signals completion
  bool one_round = false;      // every layer past the first has K_pad <= 512: one sweep round
  bool has_ln = false;         // a LayerNormalization on any layer
  bool has_skip = false;       // an observation skip input on any layer (small-batch kernels: Switches::skip_small)
  // a residual connection on any layer (policy_fused_res_kernel<8> and the GEMV chain; small-batch kernels:
  // Switches::residual_small; the pipeline's policy_mlp_res_kernel: Switches::residual_batched)
  bool has_res = false;
  go2pi_cost cost{};
  // whether build() sets up the resident path (the request ring and its kernel)
  bool resident(const go2pi_opts &o) const { return (latency_ok || res_rnn) && done_ok && o.resident_ms > 0; }
};

// The checks a parsed model must pass before an engine is made of it (GO2PI_E_MODEL).
void check_model(const Model &m);
// The plan of model m under options o (defaults applied) and switches sw. Throws ApiError
// for a combination of options and graph that is not supported.
Plan plan_program(const Model &m, const go2pi_opts &o, const Switches &sw);
// The hot block's mirror of the program's other fields (program.hpp), pipeline and LN
// pipeline (w4ln_tpw) programs only: filled here and nowhere else (the LN pack's pointer,
// bpack, by build()). plan_program calls it for the scalars, build() again
// once the pointers are set.
void fill_hot_block(DevProgram &p);

// The resident kernel of each kind of request; None: served by a launch each.
struct ResForms {
  ResForm act = ResForm::None, ctl = ResForm::None;
};
// resident_ok: the engine has a resident path; ring_in_vram: its request ring ended up in
// device memory the host writes through the large BAR.
ResForms plan_resident(const Plan &pl, const Switches &sw, bool resident_ok, bool ring_in_vram);

// What go2pi_run launches at batch <= GO2PI_SMALL_MAXB (go2pi_small_kernel).
void small_kernel_name(const DevProgram &p, int waves, int small_batch, bool latency_ok, bool use_graph, char *buf,
                       size_t cap);

}  // namespace go2pi
