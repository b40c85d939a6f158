// Device helpers shared by kernels.hip and resident.hip: activations, the
// optional observation prologue and action epilogue (go2pi_opts).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "program.hpp"

namespace go2pi {

// exp(x) - 1 for x <= 0 on the hardware exp2 (v_exp_f32, ~1 ulp): the literal
// ONNX Elu formula alpha * (exp(x) - 1). Absolute error <= ~1.2e-7 (one ulp of
// 1.0), far inside the 1e-5 contract, at ~4 VALU ops instead of libm's expm1f.
__device__ __forceinline__ float expm1_neg(float x) {
  return __builtin_amdgcn_exp2f(x * 1.4426950408889634f) - 1.f;
}

// sigmoid on v_exp_f32 + v_rcp_f32 (each ~1 ulp): ~2e-7 relative, no IEEE
// division sequence. exp2 of a large positive argument gives +inf -> rcp -> 0.
__device__ __forceinline__ float sigmoid_fast(float x) {
  return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(x * -1.4426950408889634f));
}

// ONNX Softplus ln(exp(x) + 1) in the overflow-free form max(x, 0) + ln(1 + exp(-|x|))
// on v_exp_f32 / v_log_f32 (~1 ulp each): the 1 + t rounding costs at most half an
// ulp of 1 (4e-8 absolute after the ln 2 scale); a NaN propagates through the log.
__device__ __forceinline__ float softplus_fast(float x) {
  const float t = __builtin_amdgcn_exp2f(-fabsf(x) * 1.4426950408889634f);
  return fmaxf(x, 0.f) + __builtin_amdgcn_logf(1.f + t) * 0.6931471805599453f;
}

// ONNX Clip (opset 11+): std::min(std::max(x, lo), hi) as onnxruntime computes it,
// so a NaN passes through (fminf / fmaxf would return the bound instead).
__device__ __forceinline__ float clip_nan(float x, float lo, float hi) {
  return x < lo ? lo : (x > hi ? hi : x);
}

// A dense layer's activation and its ONNX attributes (Elu / LeakyRelu alpha; Clip
// min / max; Selu alpha / gamma; HardSigmoid alpha / beta), Act in onnx_model.hpp.
struct ActP {
  int act;
  float alpha, beta;
};

// the kind of every activation after the six of r01-r03 (Clip, Selu, Softplus,
// HardSigmoid, HardSwish, Softsign) as one compile-time case: its epilogue applies
// act_fn per element (a branch on the uniform kind), which keeps the number of
// epilogue instantiations of every kernel template at seven
#define GO2PI_ACT_RT 100

__device__ __forceinline__ float act_fn(int act, float alpha, float beta, float x);

// Activation with the kind known at compile time: epilogues dispatch ONCE per
// tile group (a runtime switch per element made hipcc emit every activation's
// code, an IEEE divide and a vmcnt(0) wait for each of the 16 elements per lane:
// measured 4.4K cycles per layer epilogue).
template <int ACT>
__device__ __forceinline__ float act_t(const ActP &a, float x) {
#ifdef GO2PI_DIAG_NOEPI
  return x;
#endif
  const float alpha = a.alpha, beta = a.beta;
  if constexpr (ACT == 1) return x > 0.f ? x : alpha * expm1_neg(x);  // Elu (ONNX opset 6)
  else if constexpr (ACT == 2) return x > 0.f ? x : 0.f;              // Relu
  else if constexpr (ACT == 3) return tanhf(x);                       // Tanh
  else if constexpr (ACT == 4) return sigmoid_fast(x);                // Sigmoid
  else if constexpr (ACT == 5) return x >= 0.f ? x : alpha * x;       // LeakyRelu
  else if constexpr (ACT == 6) return clip_nan(x, alpha, beta);       // Clip (ReLU6: 0, 6)
  else if constexpr (ACT == 7) return x > 0.f ? beta * x : beta * (alpha * expm1_neg(x));  // Selu
  else if constexpr (ACT == 8) return softplus_fast(x);                                     // Softplus
  else if constexpr (ACT == 9) return clip_nan(alpha * x + beta, 0.f, 1.f);                // HardSigmoid
  else if constexpr (ACT == 10) return x * clip_nan(alpha * x + beta, 0.f, 1.f);           // HardSwish
  else if constexpr (ACT == 11) return x * __builtin_amdgcn_rcpf(1.f + fabsf(x));          // Softsign (rcp: ~1 ulp)
  else if constexpr (ACT == GO2PI_ACT_RT) return act_fn(a.act, alpha, beta, x);
  else return x;
}

__device__ __forceinline__ float act_fn(int act, float alpha, float beta, float x) {
  const ActP a{act, alpha, beta};
  switch (act) {
    case 1: return act_t<1>(a, x);
    case 2: return act_t<2>(a, x);
    case 3: return act_t<3>(a, x);
    case 4: return act_t<4>(a, x);
    case 5: return act_t<5>(a, x);
    case 6: return act_t<6>(a, x);
    case 7: return act_t<7>(a, x);
    case 8: return act_t<8>(a, x);
    case 9: return act_t<9>(a, x);
    case 10: return act_t<10>(a, x);
    case 11: return act_t<11>(a, x);
    default: return x;
  }
}

// Calls f(std::integral_constant<int, ACT>) for the runtime activation kind (the
// kinds past LeakyRelu share GO2PI_ACT_RT).
template <class F>
__device__ __forceinline__ void with_act(int act, F &&f) {
  switch (act) {
    case 0: f(std::integral_constant<int, 0>{}); break;
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 5: f(std::integral_constant<int, 5>{}); break;
    default: f(std::integral_constant<int, GO2PI_ACT_RT>{}); break;
  }
}

// Sum over the 64 lanes of a wave, the same value in every lane, on DPP moves (no LDS
// crossbar round trips: six dependent __shfl_xor steps were most of the LN pass's
// time). Within each row of 16 lanes: quad_perm [1,0,3,2] and [2,3,0,1], then row_ror:4
// and row_ror:8; lanes 0, 16, 32 and 48 then hold their row's sum, read as scalars and
// added in that order. The order of the additions depends on the lane numbers alone.
template <int CTRL>
__device__ __forceinline__ float dpp_move(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}

__device__ __forceinline__ float wave_sum(float v) {
  v += dpp_move<0xb1>(v);   // quad_perm:[1,0,3,2]
  v += dpp_move<0x4e>(v);   // quad_perm:[2,3,0,1]
  v += dpp_move<0x124>(v);  // row_ror:4
  v += dpp_move<0x128>(v);  // row_ror:8
  const int i = __builtin_bit_cast(int, v);
  const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(i, 0));
  const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(i, 16));
  const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(i, 32));
  const float r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(i, 48));
  return ((r0 + r1) + r2) + r3;
}

// A layer's LayerNormalization parameters (DevLayer), read once and passed by value.
struct LnP {
  const float *g, *b;  // [N_pad], zero padded
  int N;
  float eps;
  int act;             // a pre-LN layer's activation, applied after the normalisation
  float alpha, beta;
};

__device__ __forceinline__ LnP ln_of(const DevLayer &L) {
  return LnP{L.ln_g, L.ln_b, L.N, L.ln_eps, L.ln_act, L.ln_alpha, L.ln_beta};
}

typedef __attribute__((address_space(3))) float lds_float;

// ONNX LayerNormalization (opset 17) of LDS rows, in place, one row at a time by the
// calling wave: rows r0, r0 + rs, ... < r1 of X (LDS, stride floats apart), over columns
// [0, N): lane j owns columns j, j + 64, ...; mean, then the variance of x - mean in a
// second pass (biased, fp32), then (x - mean) * rstd * g + b and, for a pre-LN layer,
// the layer's activation. Columns [N, N_pad) are excluded by index and left as they are
// (act(0) of the dense store: finite). The order of every addition depends on the column
// index (and N) alone, so a row's result does not depend on where it sits in a tile or
// batch. The caller's waves are converged (all 64 lanes active); no barrier inside.
//
// N <= 64 * LN_U (every policy width up to 512): a lane's columns of the row live in
// registers between the three passes (one LDS read per element), and Scale / B are
// loaded once for all of the wave's rows, before the first row's statistics (their L2
// latency overlaps them). Wider layers re-read the row in each pass.
//
// A real call, not inlined: inlined into the batched body it cost the 16-wave kernel
// (128 VGPRs per lane) three spilled registers; as a call, the kernels around it keep
// the registers they had.
constexpr int LN_U = 8;

inline __device__ __noinline__ void ln_rows(float *X, int stride, int r0, int r1, int rs, LnP q, int lane) {
  lds_float *Xl = (lds_float *)X;
  const int N = q.N;
  const float fn = (float)N;
  const ActP ap{q.act, q.alpha, q.beta};
  if (N <= 64 * LN_U) {
    float g[LN_U], b[LN_U];
#pragma unroll
    for (int u = 0; u < LN_U; ++u) {
      const int k = lane + 64 * u;
      g[u] = k < N ? q.g[k] : 0.f;
      b[u] = k < N ? q.b[k] : 0.f;
    }
    for (int r = r0; r < r1; r += rs) {
      lds_float *row = Xl + r * stride;
      float x[LN_U];
#pragma unroll
      for (int u = 0; u < LN_U; ++u) x[u] = lane + 64 * u < N ? row[lane + 64 * u] : 0.f;
      float s = 0.f;
#pragma unroll
      for (int u = 0; u < LN_U; ++u) s += x[u];  // (columns past N add an exact 0)
      const float mean = wave_sum(s) / fn;
      float v = 0.f;
#pragma unroll
      for (int u = 0; u < LN_U; ++u) {
        const float d = lane + 64 * u < N ? x[u] - mean : 0.f;
        x[u] = d;
        v = fmaf(d, d, v);
      }
      const float rstd = 1.f / sqrtf(wave_sum(v) / fn + q.eps);
      with_act(q.act, [&](auto act_k) {
        constexpr int ACT = decltype(act_k)::value;
#pragma unroll
        for (int u = 0; u < LN_U; ++u)
          if (lane + 64 * u < N) row[lane + 64 * u] = act_t<ACT>(ap, fmaf(x[u] * rstd, g[u], b[u]));
      });
    }
    return;
  }
  for (int r = r0; r < r1; r += rs) {
    lds_float *row = Xl + r * stride;
    float s = 0.f;
    for (int k = lane; k < N; k += 64) s += row[k];
    const float mean = wave_sum(s) / fn;
    float v = 0.f;
    for (int k = lane; k < N; k += 64) {
      const float d = row[k] - mean;
      v = fmaf(d, d, v);
    }
    const float rstd = 1.f / sqrtf(wave_sum(v) / fn + q.eps);
    with_act(q.act, [&](auto act_k) {
      constexpr int ACT = decltype(act_k)::value;
      for (int k = lane; k < N; k += 64)
        row[k] = act_t<ACT>(ap, fmaf((row[k] - mean) * rstd, q.g[k], q.b[k]));
    });
  }
}

// ln_rows' register path for a kernel that holds the layer's Scale / B itself and has no
// registers for a call (policy_act1_kernel: its lanes carry the policy's weights): U
// columns per lane (N <= 64 U), g / b the lane's Scale and B of columns lane + 64 u (0 past
// N), inlined. The additions run in ln_rows' order (the lane's columns ascending, wave_sum,
// the variance of x - mean in a second pass, 1 / sqrt, fmaf(x * rstd, g, b), then the
// activation's own arithmetic), so a row's result is the bits ln_rows gives.
template <int U>
__device__ __forceinline__ void ln_rows_held(float *X, int stride, int r0, int r1, int rs, const float (&g)[U],
                                             const float (&b)[U], int N, float eps, ActP ap, int lane) {
  lds_float *Xl = (lds_float *)X;
  const float fn = (float)N;
  for (int r = r0; r < r1; r += rs) {
    lds_float *row = Xl + r * stride;
    float x[U];
#pragma unroll
    for (int u = 0; u < U; ++u) x[u] = lane + 64 * u < N ? row[lane + 64 * u] : 0.f;
    float s = 0.f;
#pragma unroll
    for (int u = 0; u < U; ++u) s += x[u];
    const float mean = wave_sum(s) / fn;
    float v = 0.f;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const float d = lane + 64 * u < N ? x[u] - mean : 0.f;
      x[u] = d;
      v = fmaf(d, d, v);
    }
    const float rstd = 1.f / sqrtf(wave_sum(v) / fn + eps);
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (lane + 64 * u < N) row[lane + 64 * u] = act_fn(ap.act, ap.alpha, ap.beta, fmaf(x[u] * rstd, g[u], b[u]));
  }
}

// The action epilogue (go2pi_opts and a graph's trailing Clip / scalar Mul):
// y <- scale * clip(tanh?(y), lo, hi); the clip passes a NaN through, as ONNX Clip.
// Post: its program fields read once, by value — a loop that stores the actions
// would otherwise reload them (and wait for the scalar load) per element.
struct Post {
  int tanh;
  float lo, hi, scale;
};

__device__ __forceinline__ Post post_of(const DevProgram &P) { return Post{P.post_tanh, P.clip_lo, P.clip_hi, P.scale}; }

__device__ __forceinline__ float post_fn(const Post &q, float v) {
  if (q.tanh) v = tanhf(v);
  v = clip_nan(v, q.lo, q.hi);
  return v * q.scale;
}

__device__ __forceinline__ float post_fn(const DevProgram &P, float v) { return post_fn(post_of(P), v); }

// The prologue's program fields, read once (by value): loops that store to memory
// between elements would otherwise reload them, and a reload the compiler cannot
// prove unaliased by those stores becomes a vector load (an L2 round trip per element).
struct Pro {
  const float *sub, *div, *mul;
  int sub_b, div_b, mul_b, clip;
  float lo, hi;
};

__device__ __forceinline__ Pro pro_of(const DevProgram &P) {
  return Pro{P.pre_sub, P.pre_div, P.pre_mul, P.pre_sub_bcast, P.pre_div_bcast, P.pre_mul_bcast, P.pre_clip,
             P.obs_lo, P.obs_hi};
}

__device__ __forceinline__ float prologue(const Pro &q, float v, int k) {
  if (q.sub) v -= q.sub[q.sub_b ? 0 : k];
  if (q.div) v /= q.div[q.div_b ? 0 : k];
  if (q.mul) v *= q.mul[q.mul_b ? 0 : k];
  if (q.clip) v = clip_nan(v, q.lo, q.hi);
  return v;
}

__device__ __forceinline__ float prologue(const DevProgram &P, float v, int k) { return prologue(pro_of(P), v, k); }

// One column's prologue constants, read once for a column applied to many rows
// (the identity values where an op is absent: never applied, q's flags decide).
struct ProK {
  float sub, div, mul;
};

__device__ __forceinline__ ProK pro_k(const Pro &q, int k) {
  return ProK{q.sub ? q.sub[q.sub_b ? 0 : k] : 0.f, q.div ? q.div[q.div_b ? 0 : k] : 1.f,
              q.mul ? q.mul[q.mul_b ? 0 : k] : 1.f};
}

__device__ __forceinline__ float prologue(const Pro &q, const ProK &c, float v) {
  if (q.sub) v -= c.sub;
  if (q.div) v /= c.div;
  if (q.mul) v *= c.mul;
  if (q.clip) v = clip_nan(v, q.lo, q.hi);
  return v;
}

}  // namespace go2pi
