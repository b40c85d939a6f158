/*
 * go2pi — MI355X-native batched policy-inference engine, C ABI.
 *
 * This is the boundary the drop-in `ONNXActor` (include/onnx_actor.hpp) and any
 * FFI (ctypes, cgo, JNI …) bind to. Plain pointers and sizes only; no HIP or
 * torch types in any signature (a HIP stream travels as `void*`).
 *
 * Each entry point replaces one piece of the reference's onnxruntime-backed
 * operator (inria-paris-robotics-lab/go2_onnx_controller):
 *
 *   go2pi_create        <- ONNXActor::ONNXActor  onnx_inference/src/cpp/onnx_actor.cpp:6-36
 *                          (Ort::Session(env, path, SessionOptions{nullptr}) :16,
 *                           input/output name+shape discovery :23-28)
 *   go2pi_io_name /
 *   go2pi_io_shape      <- GetInputNameAllocated / GetInputTypeInfo … GetShape  onnx_actor.cpp:23-28
 *                          (consumed by print_model_info :60-66 and check_dims :50-58)
 *   go2pi_run           <- ONNXActor::act()  onnx_actor.cpp:38-48 (Session::Run :47),
 *                          generalised to a batch of robots (rows)
 *   go2pi_run_device    <- same, device-resident obs/action (many-robot path)
 *   go2pi_reset_hidden  <- (build-defined, recurrent policies)
 *   go2pi_last_error    <- Ort::Exception::what()  (the reference throws; the C ABI returns a
 *                          status and the C++ shim rethrows std::runtime_error)
 *   go2pi_destroy       <- ~ONNXActor  onnx_actor.hpp:38
 *
 * Return codes: 0 = OK, negative = error (message via go2pi_last_error(), per
 * thread). An engine instance is NOT re-entrant: one call at a time, exactly as
 * the reference binds fixed tensors per ONNXActor (onnx_actor.cpp:31-35).
 */
#ifndef GO2PI_H_
#define GO2PI_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GO2PI_OK 0
#define GO2PI_E_INVALID (-1)   /* bad argument */
#define GO2PI_E_MODEL (-2)     /* unreadable / unsupported ONNX model */
#define GO2PI_E_DEVICE (-3)    /* no HIP device / HIP runtime error */
#define GO2PI_E_CAPACITY (-4)  /* batch above the engine's capacity */

typedef struct go2pi_engine go2pi_engine;

/* the bits of go2pi_opts.ln_small */
#define GO2PI_LN_SMALL 1
#define GO2PI_LN_BATCHED 2

/* Engine options. Zero-initialise, then call go2pi_default_opts(). */
typedef struct go2pi_opts {
  int32_t struct_size;   /* = sizeof(go2pi_opts) */
  int32_t device;        /* HIP device ordinal, default 0 */
  int64_t max_batch;     /* robots per call capacity (device buffers), default 4096 */
  int32_t use_graph;     /* 1 (default): the small-batch host path replays a captured hipGraph */
  int32_t log_level;     /* OrtLoggingLevel-compatible: 0 VERBOSE … 4 FATAL, default 2 */
  int32_t waves;         /* waves per workgroup of the batched kernel: 4, 8 or 16 (0 = auto: 4 for a uniform MLP, else 8) */
  int32_t small_batch;   /* host batches <= this use the GEMV chain (0 = auto: 8; -1 = never) */
  /* Optional fused prologue / epilogue (north_star: obs normalisation, action tanh/clip).
     All OFF by default so act() stays comparable to the shipped graph. */
  const float *obs_mean; /* [in_dim] or NULL */
  const float *obs_std;  /* [in_dim] or NULL: x <- (x - mean) / std */
  float obs_clip;        /* > 0: clamp normalised obs to [-obs_clip, obs_clip] */
  int32_t action_tanh;   /* 1: action <- tanh(action) */
  float action_clip;     /* > 0: clamp action to [-action_clip, action_clip]
                            (the caller's kActionLimit clamp, controller.cpp:217-223) */
  float action_scale;    /* != 0 and != 1: action <- action * action_scale (after clip) */
  /* > 0: go2pi_run and go2pi_controller_step at batch <= 8 are served by a RESIDENT
     kernel (no launch per call: the request and its input rows travel as tagged
     granules in host-mapped memory); the kernel leaves after this many ms without a
     request and is relaunched by the next call. Dense (non-recurrent) policies whose
     final layer is <= 16 wide; others keep the launch path. 0 (default): one launch
     per call. Any other call on the engine first stops the resident kernel. */
  int32_t resident_ms;
  /* Two bits, for a LayerNormalization policy (no effect on any other, or on a recurrent one):
     GO2PI_LN_SMALL (1): at batch <= 8 it is served like an LN-free one: by the single-launch
     kernel and, with resident_ms > 0, by a resident kernel (go2pi_create). Without the bit:
     one launch per layer, as before this field existed. No effect above batch 8.
     GO2PI_LN_BATCHED (2): above the small-batch paths, a dense LN policy whose shape the
     4-wave pipeline serves runs on policy_mlp_ln_kernel (go2pi_create); any other keeps the
     general batched kernel. No effect on the controller tick or at batch <= 8.
     0 (default): neither; 3: both. Any value outside 0 .. 3 reads as 0. (The field fills what
     was tail padding: a zero-initialised struct of the earlier layout reads 0.) */
  int32_t ln_small;
} go2pi_opts;

void go2pi_default_opts(go2pi_opts *opts);

/* Load an ONNX policy (Gemm/MatMul+Add with Elu/Relu/Tanh/Sigmoid/LeakyRelu, optional GRU)
   and upload it to the device. `opts` may be NULL (defaults).
   Observation skip inputs (estimator-actor policies: an encoder reads the observation, the
   actor reads Concat(observation parts, encoder output)): a dense layer may read a Concat on
   the feature axis (1 or -1) of the previous layer's value (after its activation, post-LN
   or a held constant Mul / Div) and one or more observation parts, in any order. A part is
   the observation as layer 0 reads it (after its Sub / Div / Mul / Clip prologue or
   per-block front-end) or a step-1 Slice of it on the feature axis; Identity may sit
   anywhere. The Concat must feed a Gemm or MatMul. Layer 0 may itself read a Slice of the
   observation (a gather: columns it does not read are never multiplied). Several layers,
   the final one included, may have such an input. Refused with GO2PI_E_MODEL and a message
   of their own: a Concat of two computed values (two sub-networks joined), a Concat on
   another axis, a Slice with a step other than 1 or on the batch axis, a part with
   arithmetic of its own or taken from in front of the prologue, an activation /
   LayerNormalization / Clip on the concatenation, an Add of two computed values that is no
   residual connection of the form below, and any skip input in a policy with a GRU or LSTM cell. Such a policy is
   served by the general batched kernel and, at batch <= small_batch, by one launch per
   layer (replayed as a graph); by default it has no single-launch or resident kernel
   (resident_ms is accepted and go2pi_resident_kernel reports "none") and ln_small has no
   effect on it. With GO2PI_SKIP_SMALL set in the environment when the engine is created
   (to any value; it holds for the engine's life) a dense policy of the single launch's
   shape is served at batch <= small_batch by policy_latency_kernel and, with
   resident_ms > 0, by the multi-workgroup policy_resident_kernel (never by a
   single-workgroup or the wide resident kernel); a policy that also has a
   LayerNormalization needs ln_small's bit 1 as well. go2pi_controller_step* returns
   GO2PI_E_INVALID for a policy with a skip input, switch or not. go2pi_inspect_model reports each
   layer's "skip": the observation columns appended to its input, in device order.
   Residual connections (SimBa blocks, ResNet-v1 MLPs): an Add, in either operand order, of
   a layer's Gemm / MatMul (+ bias) output, in front of its LayerNormalization and activation,
   and an earlier layer's carried value (possibly through Identity): the input of that
   layer's LayerNormalization where it has one, else its output; equal widths; one carried
   value live at a time (a chain of blocks, no nesting or overlap). Refused with
   GO2PI_E_MODEL and a message that names the "residual connection": a carried value with
   more than two consumers or more than one Add, the observation as the added operand, an
   Add on the output layer, behind an activation or a LayerNormalization, or whose sum
   feeds the next Gemm with neither on it, a tap between a Gemm and its activation or from a
   LayerNormalization's output, a held constant Mul / Div on the source, and any residual
   connection beside a GRU or LSTM cell. Such a policy is served by
   policy_fused_res_kernel<8> and, at batch <= small_batch, by one launch per layer
   (replayed as a graph); opts.waves = 4 or 16 fails with GO2PI_E_INVALID for it, by default
   it has no single-launch or resident kernel (resident_ms is accepted and
   go2pi_resident_kernel reports "none"; ln_small and GO2PI_SKIP_SMALL have no effect on it),
   and go2pi_controller_step* returns GO2PI_E_INVALID, switch or not. With
   GO2PI_RESIDUAL_SMALL set in the environment when the engine is created (to any value; it
   holds for the engine's life) a policy of the single launch's shape is served at batch <=
   small_batch by policy_latency_kernel and, with resident_ms > 0, by the multi-workgroup
   policy_resident_kernel (never by a single-workgroup or the wide resident kernel); a
   policy that also has a LayerNormalization (every SimBa model) needs ln_small's bit 1 as
   well, one that also has a skip input GO2PI_SKIP_SMALL. With GO2PI_RESIDUAL_BATCHED set in
   the environment when the engine is created (to any value; it holds for the engine's life;
   an environment switch because go2pi_opts ends in ln_small) the batched launches of a
   residual policy of the 4-wave pipeline's shape run on policy_mlp_res_kernel<tiles per wave,
   head tiles>, which keeps the carried value in registers: no skip input, opts.waves = 0,
   every hidden layer's width padded to 64 the same 128, 256 or 512 (the activations may
   differ from layer to layer), an output layer of at most 32 columns (16 at 512), an
   observation no wider than the hidden layers, and no prologue (obs_mean / obs_std / clip,
   Sub / Div / Mul / Clip nodes) or action post-processing. It needs no LayerNormalization
   and no ln_small bit. Any other residual policy, and opts.waves = 8, keep
   policy_fused_res_kernel<8>; waves = 4 / 16 stay refused, batches <= small_batch, the
   resident kernel and go2pi_controller_step* are what they are without the switch, and the
   switch has no effect on a policy without residual connections. go2pi_batched_kernel
   names the kernel. go2pi_inspect_model reports each layer's
   "res": the index of the layer whose carried value it adds, or -1.
   LayerNormalization (opset 17, over the feature axis, epsilon from the attribute, Scale
   and optional B constant, only output 0 used) is accepted on any dense layer but the last,
   once per layer: right after the layer's Gemm / MatMul (+ bias), in front of its
   activation if it has one ("pre"), or right after its activation ("post"). Any other
   placement (on the observation, after the recurrent cell, on the output layer, twice on
   a layer, with a Mul / Div / Add between it and its activation), another axis or
   stash_type, a Scale / B of another length or not constant, and a consumed Mean /
   InvStdDev output fail with GO2PI_E_MODEL and a message of their own. Such a policy is
   served by the general batched kernel and, at batch <= 8, by one launch per layer. With
   opts.ln_small = 1 a dense one is served at batch <= 8 by the single-launch kernel, and
   with resident_ms > 0 by a resident kernel: policy_act1_kernel where its shape applies
   (hidden layers 64 or 128 wide), else the multi-workgroup policy_resident_kernel (never
   policy_wide_kernel or policy_resident1_kernel). Its controller tick at batch <= 8 is the
   single launch (no resident controller form), and a recurrent LN policy keeps the
   general body. The lean / pipeline batched kernels do not serve LN; with opts.ln_small's
   GO2PI_LN_BATCHED bit, batched launches of a dense LN policy run on the pipeline's LN kernel,
   policy_mlp_ln_kernel<tiles per wave, head tiles>, when every hidden layer pads to the same
   128, 256 or 512 columns with one activation, the head has at most 32 outputs (16 at 512),
   the observation is no wider than the hidden layers, and the options add no observation
   normalisation or clip and no action post-processing; go2pi_batched_kernel names it. */
int go2pi_create(const char *onnx_path, const go2pi_opts *opts, go2pi_engine **out);
int go2pi_create_from_memory(const void *onnx_bytes, size_t nbytes, const go2pi_opts *opts,
                             go2pi_engine **out);
void go2pi_destroy(go2pi_engine *e);

/* I/O metadata of graph input/output `index` (0 = the bound observation / action). */
int go2pi_num_io(const go2pi_engine *e, int32_t *n_inputs, int32_t *n_outputs);
int go2pi_io_name(const go2pi_engine *e, int32_t is_output, int32_t index, char *buf, size_t cap);
/* Writes up to `cap` dims; *rank receives the true rank. Symbolic dims read as -1. */
int go2pi_io_shape(const go2pi_engine *e, int32_t is_output, int32_t index, int64_t *dims, int32_t cap,
                   int32_t *rank);
/* Per-robot feature counts of the bound observation / action (shape[1]). */
int go2pi_io_dims(const go2pi_engine *e, int64_t *in_dim, int64_t *out_dim);

/* ---------------------------------------------------------------------------
   Buffer contract (every entry point that takes rows; tests/test_gpu_abi_confinement.py).
   Rows [0, batch) only: a call reads and writes rows [0, batch) of the buffers it is given
   and no byte outside them, so a buffer may be a sub-range of a larger allocation of the
   caller's with live data on either side. Nothing a call returns depends on what lies
   outside those rows (the kernels work in 16-row tiles; in the last tile the rows past
   `batch` are computed from zeros or from a copy of row batch - 1, never from the caller's
   memory, and are never stored).
   Inputs are never written: obs / obs_dev of the run paths, state and joy of the
   controller tick. (The tick's obs and action are in/out by design, see below.)
   The engine's own recurrent state obeys the same rule: a call on `batch` robots advances
   hidden rows [0, batch) and leaves rows [batch, max_batch) bit-identical;
   go2pi_reset_hidden(mask, batch) zeroes exactly the masked rows below `batch`.
   Alignment, per entry point:
     go2pi_run, go2pi_controller_step (host pointers)     the natural alignment of the element
         type (4 bytes for float / uint32_t, 8 for double): the rows are staged through
         engine-owned, 256-byte-aligned buffers and copied to and from the caller's.
     go2pi_run_device, go2pi_run_sequence_device          obs_dev and act_dev 4 bytes. (When
         act_dev is 16-byte aligned and out_dim is a multiple of 4 the batched kernels store
         four actions at a time, else one: the same values either way, bit for bit.)
     go2pi_controller_step_device                         action_dev, q_des_dev, kp_dev and
         kd_dev 16 bytes each (a NULL optional output is exempt): the batched tick writes a
         robot's joints four at a time with 16-byte stores (one float4, or two doubles) at
         byte offsets that are multiples of 16 from the pointer (a row is 48 or 96 bytes).
         state_dev, joy_dev, obs_dev and status_dev 4 bytes: they are read through 4-byte
         direct-to-LDS loads and written one element at a time. A pointer that breaks this
         is refused with GO2PI_E_INVALID and a message that names it, before anything is
         enqueued; no buffer is touched. A row range [r0, r1) of 16-byte-aligned [B][12]
         arrays is itself aligned, so sharding a fleet by rows needs no care. */

/* Synchronous host path: obs [batch][in_dim] -> act [batch][out_dim], host memory
   (the act() contract: reads obs at call time, overwrites act in place). */
int go2pi_run(go2pi_engine *e, const float *obs, float *act, int64_t batch);

/* Asynchronous device path: obs/act are device pointers on e's device; enqueued on
   `hip_stream` (a hipStream_t; NULL = the HIP null stream, as in HIP). No host sync.
   The caller must use the same HIP runtime instance as this library (e.g. load
   PyTorch's libamdhip64 first when sharing torch streams/tensors).
   Buffers: rows [0, batch) only, obs_dev never written, 4-byte alignment (above). */
int go2pi_run_device(go2pi_engine *e, const float *obs_dev, float *act_dev, int64_t batch, void *hip_stream);

/* Recurrent policies carry one hidden row per robot (engine-resident, HBM).
   Run `steps` ticks back to back with the hidden rows kept on-chip between ticks:
   obs_dev [steps][batch][in_dim] -> act_dev [steps][batch][out_dim]. For a
   feed-forward policy this is `steps` independent batched calls.
   Buffers: exactly steps * batch rows of each, obs_dev never written, 4-byte alignment. */
int go2pi_run_sequence_device(go2pi_engine *e, const float *obs_dev, float *act_dev, int64_t steps,
                              int64_t batch, void *hip_stream);

/* Zero the hidden state of robots whose mask byte is non-zero (mask NULL = all). */
int go2pi_reset_hidden(go2pi_engine *e, const uint8_t *mask, int64_t batch);
/* Copy hidden state rows [0,batch) to/from host (hidden_dim floats per robot). */
int go2pi_get_hidden(go2pi_engine *e, float *h, int64_t batch);
int go2pi_set_hidden(go2pi_engine *e, const float *h, int64_t batch);
int go2pi_hidden_dim(const go2pi_engine *e, int64_t *hidden_dim);

/* Wait for all work queued on the engine's own stream. */
int go2pi_sync(go2pi_engine *e);

/* Algorithmic cost per robot-step (for roofline accounting in bench.py). */
typedef struct go2pi_cost {
  double flops_per_row;    /* 2*MAC of every contraction (+ nothing for activations) */
  double weight_bytes;     /* fp32 parameter bytes (unpadded; LayerNormalization Scale and B included) */
  double io_bytes_per_row; /* obs + action (+ 2x hidden for recurrent) bytes */
  int32_t n_layers;
  int32_t has_gru;         /* recurrent cell in front of the dense layers: 0 none, 1 GRU, 2 LSTM */
} go2pi_cost;
int go2pi_get_cost(const go2pi_engine *e, go2pi_cost *cost);

/* Name of the batched kernel instantiation this engine launches for batches
   above the small-batch paths, e.g. "policy_fused_kernel<4, 8, 1>" (waves per
   workgroup, tiles per wave of the 4-wave pipeline, head tiles), as rocprofv3
   reports it. Writes a NUL-terminated string into buf (truncated to cap-1). For
   profiling tools; no compute. */
int go2pi_batched_kernel(const go2pi_engine *e, char *buf, size_t cap);

/* Name of the resident kernel that serves go2pi_run at batch <= 8 on this engine
   (opts.resident_ms > 0), then " ring=vram" when the request ring is in device
   memory the host writes through the large-BAR mapping, " ring=host" when it is in
   pinned host memory; "none" when no resident kernel serves act(). E.g.
   "policy_wide_kernel<4, 8, 12, 0> ring=vram". For tests and profiling tools; no
   compute. */
int go2pi_resident_kernel(const go2pi_engine *e, char *buf, size_t cap);

/* Name of what serves a host go2pi_run at batch <= 8 on this engine when no resident
   kernel does, following go2pi_run's selection: "policy_latency_kernel" (one launch for
   the whole policy; a LayerNormalization program's instantiation of it is the symbol
   policy_latency_ln_kernel), "gemv_layer_kernel graph" (one launch per layer replayed as a
   hipGraph; "gemv_layer_kernel" with use_graph = 0), or the batched kernel's name
   (go2pi_batched_kernel) when small_batch = -1 or the policy is recurrent. For tests and
   profiling tools; no compute. */
int go2pi_small_kernel(const go2pi_engine *e, char *buf, size_t cap);

/* Resident kernel launches this engine has made so far (one serves every request
   until it idles out or another call stops it; a kernel that aborts on a request
   shows up as a launch per call). For tests and profiling tools; no compute. */
int go2pi_resident_launches(const go2pi_engine *e, int64_t *n);

/* Parse and lower an ONNX policy WITHOUT touching a device (no compute): writes a
   JSON description (I/O names and shapes, the lowered layer program with
   per-layer weight/bias checksums) into buf. Returns the JSON length (>= 0) or an
   error code; truncates to cap-1 bytes. For loader tests and tooling. */
int go2pi_inspect_model(const char *onnx_path, char *buf, size_t cap);

/* ---------------------------------------------------------------------------
   Controller tick: the Go2 ONNXController's per-tick work around act(), fused
   into the policy launch (many robots or one):
     prologue  <- observation assembly, controller.cpp:173-212 + lowstate_cb_
                  controller.hpp:93-110 (gravity projection of the IMU quaternion,
                  q - q0, joystick velocity command, foot contacts, and the
                  kHistory-step history shift of populate_buffer, controller.hpp:45-68)
     epilogue  <- action post-processing, controller.cpp:217-223 (clamp to
                  +-kActionLimit, joystick stop button zeroes the action) and
                  240-248 (q_des = q0 + 0.25 a, kp/kd arrays for send_command)
   Needs a policy whose observation is kHistory x 49 features (kDimObs,
   controller.hpp:14; the shipped model: 98) and whose action has 12.
   Per-robot raw state row, GO2PI_CTL_STATE_DIM floats:
     [0:4]  imu_state.quaternion (w, x, y, z)     [4:7]   imu_state.gyroscope
     [7:19] joint q (Isaac order)                 [19:31] joint dq
     [31:35] foot_force (Unitree order, as in LowState)   [35] reserved
   Per-robot joystick row, GO2PI_CTL_JOY_DIM floats:
     {has_axes, axes[0], axes[1], axes[3], buttons[0]}; has_axes = 0 keeps the
     previous velocity command (the reference only updates it when axes are
     present). A NULL joystick pointer means no message for any robot (velocity
     command kept, stop button released).
   State carried between ticks (caller-owned, in place, as the reference's
   observation_ / action_ members): obs [batch][in_dim] holds the previous
   observation on entry and this tick's on return (the ObservationAction log
   row, controller.cpp:226); action [batch][12] holds the previous action on
   entry and this tick's post-processed action on return. Zero both to start.
   Outputs q_des / kp / kd [batch][12] (double, as send_command takes them) may
   be NULL. status [batch] (may be NULL): bit 0 set when a NaN entered the
   observation (the reference exit(1)s in populate_buffer's check,
   controller.hpp:57-64); the tick still completes. */
#define GO2PI_CTL_STATE_DIM 36
#define GO2PI_CTL_JOY_DIM 5
#define GO2PI_CTL_DOF 12

typedef struct go2pi_ctl_params {
  int32_t struct_size;     /* = sizeof(go2pi_ctl_params) */
  float kp;                /* kp_ (controller.hpp:119), default 28 */
  float kd;                /* kd_ (:120), default 0.5 */
  float kp_stop;           /* kp while the stop button is held (controller.cpp:246), default 5 */
  float action_limit;      /* kActionLimit (controller.hpp:17), default 1000 */
  float contact_threshold; /* foot_force >= this is a contact (controller.hpp:100-103), default 22 */
  float gravity_w[3];      /* gravity_w_ (controller.hpp:131), default (0, 0, -1) */
  double action_scale;     /* q_des = q0 + action_scale * a (controller.cpp:244), default 0.25 */
  double q0[12];           /* q0_ (controller.hpp:165), Isaac order */
} go2pi_ctl_params;

void go2pi_ctl_default_params(go2pi_ctl_params *params);
/* Set the engine's controller parameters (synchronous; defaults at create). */
int go2pi_ctl_set_params(go2pi_engine *e, const go2pi_ctl_params *params);
/* kHistory of the bound policy (in_dim / 49), or GO2PI_E_MODEL if its I/O is not
   a Go2 controller's (in_dim a multiple of 49, out_dim 12). */
int go2pi_ctl_history(const go2pi_engine *e, int32_t *history);

/* One tick for `batch` robots, host buffers (synchronous; batch <= 8 runs as
   one launch on host-mapped staging, larger batches stage through HBM). */
int go2pi_controller_step(go2pi_engine *e, const float *state, const float *joy, float *obs, float *action,
                          double *q_des, double *kp, double *kd, uint32_t *status, int64_t batch);
/* Same on device pointers, enqueued on `hip_stream`, no host sync. Buffers (the buffer
   contract above): rows [0, batch) only; state_dev and joy_dev never written; action_dev
   and the q_des_dev / kp_dev / kd_dev that are passed must be 16-byte aligned, else
   GO2PI_E_INVALID and nothing is enqueued. */
int go2pi_controller_step_device(go2pi_engine *e, const float *state_dev, const float *joy_dev, float *obs_dev,
                                 float *action_dev, double *q_des_dev, double *kp_dev, double *kd_dev,
                                 uint32_t *status_dev, int64_t batch, void *hip_stream);

/* Diagnostics: copy up to n per-workgroup clock stamps of the last batched launch
   ({s_memtime, s_memrealtime} at start and end, 4 per workgroup). Needs a
   GO2PI_DIAG_CLOCK build and GO2PI_DIAG_STAMPS set at create; returns the count. */
int go2pi_diag_stamps(go2pi_engine *e, uint64_t *out, int64_t n);

/* Thread-local message of the last failing call on this thread ("" if none). */
const char *go2pi_last_error(void);

/* Library version string. */
const char *go2pi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* GO2PI_H_ */
