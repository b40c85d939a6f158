// HIP kernels for gfx950 (MI355X, CDNA4): the policy forward pass that the
// reference delegates to onnxruntime's CPU EP inside ONNXActor::act()
// (onnx_inference/src/cpp/onnx_actor.cpp:47 -> Gemm/Elu chain of model.onnx).
//
// 1. policy_fused_kernel<NW>  — the batched (many-robot) path.
//    One workgroup owns a tile of 16 robots for the WHOLE policy: the
//    activations of its 16 rows stay in LDS between layers (never touch HBM),
//    every layer is a strict-fp32 MFMA contraction (v_mfma_f32_16x16x4_f32:
//    A = 16 robots x 4 k from LDS, B = 4 k x 16 outputs straight from HBM/L2 in
//    the pre-packed fragment order of program.hpp), bias enters as the
//    accumulator's initial value, the activation is fused into the epilogue,
//    and the final layer writes the action rows (with the optional
//    tanh/clip/scale epilogue) directly to global memory. A recurrent policy
//    runs its GRU cell first with the hidden rows carried in LDS across ticks.
//    At batch 4096 the grid is exactly 256 workgroups = one per CU.
//
// 2. gemv_layer_kernel        — the small-batch (1..8 robots) latency path.
//    One workgroup per 16-output tile, 8 waves split the K chunks, fp32 VALU
//    dot products on the same packed fragments + wave/LDS reductions
//    (tile_layer.hpp states the order). One launch per layer, captured into a
//    hipGraph by the engine.
//
// Numerics: fp32 storage and arithmetic throughout (the f32-input MFMA is an
// exact k-ordered fmaf chain, no TF32/xf32 on gfx950). The summation order
// differs from the CPU reference, so parity is tolerance-based (north_star:
// 1e-5 fp32 vs the CPU path), while every robot row is computed with an
// identical instruction sequence wherever it sits in the batch: sharded and
// unsharded runs are bit-identical.
#include "fused_impl.hpp"
#include "tile_layer.hpp"
#include "w4ln_layout.hpp"

namespace go2pi {

// ---------------------------------------------------------------------------
// Small-batch GEMV layer. grid = N_pad/16 workgroups (one per 16-output tile),
// the tiled layer body of tile_layer.hpp. x: [B][x_stride] (device or host-mapped memory),
// y: [B][y_stride]. Layer 0 applies the prologue; the final layer the epilogue.
constexpr int GEMV_WAVES = TILE_WAVES;

// obs: the call's observation rows [B][in_dim] (the engine's staging buffer in a captured
// graph: every replay reads the fresh rows), read by a layer with an observation skip input
// (DevLayer::skip_n): its staged row is [the previous layer's N outputs | obs columns
// skip_idx[0 .. skip_n) through the prologue], and layer 0's a gather of those columns.
// cin / cout (residual connections, DevProgram::res; the engine's carry buffers, fixed per
// engine as the ping-pong buffers are, so a replayed graph reads and writes the same rows):
// a consumer layer adds cin[b][n] after the bias and in front of the activation,
// (sum + bias) + carried; a source layer writes the value it stores to y (a pre-LN layer's
// raw pre-activation: the consumer's staging normalises y, never the carried rows) to
// cout[b][n] from the thread that writes y. Null: neither. A layer that does both gets two
// distinct buffers from the engine; each thread touches only its own (b, n) of either.
__global__ __launch_bounds__(GEMV_WAVES * 64) void gemv_layer_kernel(DevProgram P, int layer, const float *obs,
                                                                     const float *x, int x_stride, float *y,
                                                                     int y_stride, int B, const float *cin,
                                                                     float *cout, int c_stride) {
  extern __shared__ float4 lds4[];
  const DevLayer &L = P.L[layer];
  const int K_pad = L.K_pad, C = K_pad >> 4, T = L.N_pad >> 4;
  const int skip_n = L.skip_n;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int t = blockIdx.x;
  const GemvLds LY = gemv_lds(K_pad);
  float *xs = reinterpret_cast<float *>(lds4), *part = xs + LY.xs.size;  // (the regions in LY's order)
  // Weights and bias do not depend on the input: issue their loads first so
  // their latency overlaps the input staging.
  float4 wr[TILE_MAXS];
  tile_load(wr, L.w, t, T, C, wave, lane);
  const float bv = (wave == 0 && lane < 16) ? L.bias[t * 16 + lane] : 0.f;
  if (layer == 0 && skip_n) {
    stage_gather(P, obs, P.in_dim, P.skip_idx[0], skip_n, xs, K_pad, B, tid);
  } else if (layer == 0) {
    stage_obs(P, x, x_stride, xs, K_pad, B, tid);
  } else {  // the previous layer's K outputs from x, then this layer's skip columns
    const int K = P.L[layer - 1].N;
    const int *sidx = P.skip_idx[layer];
    for (int e = tid; e < B * K_pad; e += GEMV_WAVES * 64) {
      const int b = e / K_pad, k = e - b * K_pad;
      float v = 0.f;
      if (k < K) {
        v = x[(size_t)b * x_stride + k];
      } else if (k < K + skip_n) {
        // (the LN pass below normalises columns [0, K) by index and leaves these as they are)
        const int c = sidx[k - K];
        v = prologue(P, obs[(size_t)b * P.in_dim + c], c);
      }
      xs[b * K_pad + k] = v;
    }
  }
  __syncthreads();
  // The previous layer's LayerNormalization (it stored its un-normalised output: a
  // pre-LN layer its raw pre-activation): every workgroup holds the whole rows, so
  // each normalises its own copy while staging, one row per wave. No extra launch.
  if (layer > 0 && P.L[layer - 1].ln) {  // uniform over the workgroup
    ln_rows(xs, K_pad, wave, B, GEMV_WAVES, ln_of(P.L[layer - 1]), lane);
    __syncthreads();
  }
  // (chunks past the register slots, K_pad > 1024: their fragments from memory)
  const float4 *W = reinterpret_cast<const float4 *>(L.w) + (size_t)t * 64 + lane;
  tile_dot(xs, part, wr, K_pad, C, B, wave, lane, [&](int c) { return W[(size_t)c * T * 64]; });
  __syncthreads();
  // (the carry buffers are cleared when the engine is built: a column no source wrote reads 0)
  if (wave == 0 && lane < 16)
    tile_finish(part, t, lane, B, bv, ActP{L.act, L.alpha, L.beta}, layer == P.nl - 1, cin, c_stride,
                [&](int b, int n, float v, bool last) {
                  if (last) {
                    if (n < L.N) y[(size_t)b * y_stride + n] = post_fn(P, v);
                  } else {
                    y[(size_t)b * y_stride + n] = v;  // padded columns are exact zeros
                    if (cout) cout[(size_t)b * c_stride + n] = v;
                  }
                });
}

// ---------------------------------------------------------------------------
// policy_latency_kernel — the batch-1 act() path in ONE launch (B <= 4).
// One workgroup per 16-output tile of the widest layer; each layer: the
// workgroup prefetches its weight fragments into registers, gathers the layer
// input, reduces its 16 outputs over 8 waves, and publishes them as 8-byte
// {tag, value} granules (cdna_hip_programming.md Guideline 16 recipe R2: one
// aligned agent-scope relaxed store per granule; the consumer's single wave
// re-reads until every tag equals the layer's epoch — no flag, no fence, no
// counter, correct for any workgroup->XCD placement). Tags = epoch0 + layer,
// epoch0 advanced by the host every call, so granules of earlier calls never
// match. Spins are bounded: on timeout the workgroup writes `err` and stops.
constexpr int LAT_WAVES = lds::WAVES;
constexpr int LAT_MAXS = 8;  // chunk slots per wave held in registers (K_pad <= 1024)
// the wave that sums a layer's partials and publishes it: the last one, since wave 0
// alone sweeps a batch-1 layer input (its loads would complete behind its own stores)
constexpr int LAT_PW = LAT_WAVES - 1;

__device__ __forceinline__ bool sweep_layer(unsigned long long *gran, int n, unsigned tag, float *dst,
                                            unsigned *err, int lane) {
  constexpr int U = 8;  // granules per lane per batch: all loads issued before any is checked
  for (unsigned spins = 0;; ++spins) {
    bool ok = true;
    for (int base = 0; base < n; base += 64 * U) {
      unsigned long long v[U];
#pragma unroll
      for (int u = 0; u < U; ++u)  // clamped index: no branch around the loads
        v[u] = __hip_atomic_load(gran + min(base + u * 64 + lane, n - 1), __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = base + u * 64 + lane;
        if (i < n) {
          ok &= (unsigned)(v[u] >> 32) == tag;
          dst[i] = __uint_as_float((unsigned)v[u]);
        }
      }
    }
    if (__all(ok)) return true;
    if (spins > (1u << 22)) {  // ~seconds: a producer never ran (non-resident grid) -> give up
      if (lane == 0) __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      return false;
    }
    __builtin_amdgcn_s_sleep(1);
  }
}

// CTL: controller tick — layer 0 assembles the observation (every workgroup,
// redundantly: 98 features), the final layer stores through ctl_store, and
// workgroup 0 (the only one of the one-tile final layer, so every other
// workgroup's reads of the previous obs / action are done by then) writes the
// new observation and status before signalling completion.
// LNORM: the general instantiation (program.hpp program_small_general): the LayerNormalization
// pass (opts.ln_small) and a second sweep round for layer inputs of more than 4096
// granules. Every other program runs the instantiation without either.
// SKIP (with LNORM; act() only): the general instantiation of a program with observation skip
// inputs (DevLayer::skip_n; GO2PI_SKIP_SMALL). A skip layer's columns [prev.N, prev.N + skip_n)
// of the swept rows are overwritten with prologue(obs[b][idx[j]], idx[j]): the row
// gemv_layer_kernel stages. obs is pinned host memory here, so a thread's first LAT_SKIPV
// values (all of them at B * skip_n <= 512 LAT_SKIPV: any skip at batch 1) are loaded in
// front of the sweep, and only their LDS stores stand behind its barrier. A layer-0 gather
// stages its columns through the index table.
constexpr int LAT_SKIPV = 4;
// RES (with LNORM and SKIP; act() only): the instantiation of a program with residual
// connections (DevProgram::res; GO2PI_RESIDUAL_SMALL). Workgroup g owns tile g of every layer
// and a consumer has its source's width, so the carried value of column 16 g + lane, row b, is
// computed at the source layer by the publishing lane that adds it at the consumer layer: it
// stays in that lane's registers (carried[b]) and never leaves the workgroup. No granule, tag,
// sweep or barrier is added. A consumer's value is act((sum + bias) + carried), tile_finish's
// order; a source keeps the value it publishes (a pre-LN layer's raw sum: the consumer's staging
// normalises the granules, never the carried value), behind the consumer's read where a layer is
// both. carried[] starts at zero and a consumer clears what it read, so a workgroup that owns no
// tile of the source (a consumer padded wider than its source) adds 0, and one that owns no tile
// of a layer between source and consumer (a bottleneck) keeps the value across it.
template <bool CTL, bool LNORM = false, bool SKIP = false, bool RES = false>
__device__ __forceinline__ void latency_body(const DevProgram &P, const float *obs, float *act, int B,
                                             unsigned epoch0, unsigned long long *gran, int gstride, unsigned *err,
                                             unsigned *done, const DevCtl ctl) {
  extern __shared__ float4 lds4[];
  const LatencyLds LY = latency_lds(P.lds_stride, 0);  // (the regions in LY's order; its total is the launcher's)
  float *xs = reinterpret_cast<float *>(lds4), *part = xs + LY.xs.size;
  int &abort_flag = *reinterpret_cast<int *>(part + LY.part.size);
  float *okeep = part + LY.part.size + LY.flag.size;  // CTL: the regions of LatencyCtlLds
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (tid == 0) abort_flag = 0;
  const CtlLds CL = ctl_lds(okeep + latency_ctl_lds(P.in_dim).okeep.size, GO2PI_SMALL_MAXB, P.in_dim);
  CtlView cv{};
  CtlQ cq{};
  if constexpr (CTL) {
    cq = ctl_q(P, ctl);
    cv = ctl_view(ctl, CL, 0);
    if (g < (P.L[0].N_pad >> 4)) {  // layer-0 WGs
      ctl_lds_load(CL, ctl, 0, B, P.in_dim, tid, wave, lane, LAT_WAVES);
      lds_dma_wait();  // (the assembly reads the image after this workgroup's next barrier)
    }
  }
  // RES: the consumer and source layers, read once (as fused_body reads consm / srcm), and the
  // publishing lanes' carried rows
  const ResMasks rm = RES ? res_masks(P) : ResMasks{0u, 0u};
  float carried[GO2PI_SMALL_MAXB];
  if constexpr (RES) {
#pragma unroll
    for (int b = 0; b < GO2PI_SMALL_MAXB; ++b) carried[b] = 0.f;
  }
  for (int l = 0; l < P.nl; ++l) {
    const DevLayer &L = P.L[l];
    const int T = L.N_pad >> 4, C = L.K_pad >> 4, K_pad = L.K_pad;
    if (g >= T) continue;  // this workgroup owns no tile of layer l
    const float4 *W = reinterpret_cast<const float4 *>(L.w) + (size_t)g * 64 + lane;
    float4 wr[LAT_MAXS];
#pragma unroll
    for (int s = 0; s < LAT_MAXS; ++s) {
      const int c = wave + s * LAT_WAVES;
      wr[s] = c < C ? W[(size_t)c * T * 64] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const float bv = (wave == LAT_PW && lane < 16) ? L.bias[g * 16 + lane] : 0.f;
    // SKIP: this layer's skip columns, element e = tid + 512 u of [B][skip_n], in flight
    // across the sweep (sc: the observation column, for the prologue)
    const int sn = SKIP ? L.skip_n : 0, sk0 = (SKIP && l > 0) ? P.L[l - 1].N : 0;
    const int *sidx = SKIP ? P.skip_idx[l] : nullptr;
    float sv[LAT_SKIPV];
    int sc[LAT_SKIPV];
    if constexpr (SKIP) {
      if (l > 0 && sn) {  // uniform over the workgroup
#pragma unroll
        for (int u = 0; u < LAT_SKIPV; ++u) {
          const int e = tid + u * LAT_WAVES * 64;
          sv[u] = 0.f, sc[u] = 0;
          if (e < B * sn) {
            const int b = e / sn;
            sc[u] = sidx[e - b * sn];
            sv[u] = obs[(size_t)b * P.in_dim + sc[u]];
          }
        }
      }
    }
    if (l == 0) {
      const float *src = obs;
      if constexpr (CTL) {
        __syncthreads();  // the LDS image of the inputs (and the weights above) landed
        ctl_assemble_flat<false, 4>(P, CL, cq, ctl.joy != nullptr, B, okeep, P.in_dim, nullptr, tid, LAT_WAVES * 64);
        __syncthreads();
        src = okeep;
      }
      if (SKIP && sn) {  // a gather: layer 0 reads the columns sidx names, in that order
        for (int e = tid; e < B * K_pad; e += LAT_WAVES * 64) {
          const int b = e / K_pad, k = e - b * K_pad;
          float v = 0.f;
          if (k < sn) {
            const int c = sidx[k];
            v = prologue(P, src[(size_t)b * P.in_dim + c], c);
          }
          xs[e] = v;
        }
      } else {
        for (int e = tid; e < B * K_pad; e += LAT_WAVES * 64) {
          const int b = e / K_pad, k = e - b * K_pad;
          xs[e] = k < P.in_dim ? prologue(P, src[(size_t)b * P.in_dim + k], k) : 0.f;
        }
      }
    } else {
      // every wave sweeps its own 512 granules (8 per lane, all in flight), not
      // wave 0 alone in B * K_pad / 512 serial rounds
      const int n = B * K_pad, lo = wave * 512;
      unsigned long long *gl = gran + (size_t)(l - 1) * gstride;
      if (lo < n && !sweep_layer(gl + lo, min(512, n - lo), epoch0 + (unsigned)(l - 1), xs + lo, err, lane))
        abort_flag = 1;
      // rows past the eight waves' 4096 granules (K_pad > 512 at batch 5 and up; K_pad <= 1024
      // and B <= 8: at most 8192): a second round
      if constexpr (LNORM) {
        if (n > LAT_WAVES * 512) {  // uniform over the workgroup
          const int lo2 = lo + LAT_WAVES * 512;
          if (lo2 < n && !sweep_layer(gl + lo2, min(512, n - lo2), epoch0 + (unsigned)(l - 1), xs + lo2, err, lane))
            abort_flag = 1;
        }
      }
    }
    __syncthreads();
    if (abort_flag) return;
    // The previous layer's LayerNormalization, as in gemv_layer_kernel: the granules carry
    // its un-normalised output (a pre-LN layer's act is none), every consumer workgroup
    // swept the whole rows, so each normalises its own copy, one row per wave.
    // SKIP: the skip columns over what the sweep left there (the producer's zero-weight
    // tiles: act(0)), behind the barrier that ended every wave's sweep stores. ln_rows
    // touches columns k < prev.N alone, so the two passes share one barrier.
    bool filled = false;
    if constexpr (SKIP) {
      if (l > 0 && sn) {  // uniform over the workgroup
#pragma unroll
        for (int u = 0; u < LAT_SKIPV; ++u) {
          const int e = tid + u * LAT_WAVES * 64;
          if (e < B * sn) {
            const int b = e / sn;
            xs[b * K_pad + sk0 + (e - b * sn)] = prologue(P, sv[u], sc[u]);
          }
        }
        for (int e = tid + LAT_SKIPV * LAT_WAVES * 64; e < B * sn; e += LAT_WAVES * 64) {
          const int b = e / sn, j = e - b * sn, c = sidx[j];
          xs[b * K_pad + sk0 + j] = prologue(P, obs[(size_t)b * P.in_dim + c], c);
        }
        filled = true;
      }
    }
    if constexpr (LNORM) {
      if (l > 0 && P.L[l - 1].ln) {  // uniform over the workgroup
        ln_rows(xs, K_pad, wave, B, LAT_WAVES, ln_of(P.L[l - 1]), lane);
        __syncthreads();
        filled = false;
      }
    }
    if constexpr (SKIP) {
      if (filled) __syncthreads();
    }
    float p[GO2PI_SMALL_MAXB];
#pragma unroll
    for (int b = 0; b < GO2PI_SMALL_MAXB; ++b) p[b] = 0.f;
    const int koff = (lane >> 4) << 2;
#pragma unroll
    for (int s = 0; s < LAT_MAXS; ++s) {
      const int c = wave + s * LAT_WAVES;
      if (c >= C) break;
#pragma unroll
      for (int b = 0; b < GO2PI_SMALL_MAXB; ++b) {
        if (b < B) {
          const float4 a = *reinterpret_cast<const float4 *>(xs + b * K_pad + c * 16 + koff);
          p[b] = fmaf(a.x, wr[s].x, p[b]);
          p[b] = fmaf(a.y, wr[s].y, p[b]);
          p[b] = fmaf(a.z, wr[s].z, p[b]);
          p[b] = fmaf(a.w, wr[s].w, p[b]);
        }
      }
    }
#pragma unroll
    for (int b = 0; b < GO2PI_SMALL_MAXB; ++b) {
      p[b] += __shfl_xor(p[b], 16);
      p[b] += __shfl_xor(p[b], 32);
    }
    if (lane < 16) {
#pragma unroll
      for (int b = 0; b < GO2PI_SMALL_MAXB; ++b)
        if (b < B) part[(wave * GO2PI_SMALL_MAXB + b) * 16 + lane] = p[b];
    }
    lds_barrier();
    if (wave == LAT_PW && lane < 16) {
      const int n = g * 16 + lane;
      const bool last = l == P.nl - 1;
      const int la = L.act, LN = L.N;  // (read once: the stores below would make each row reload them)
      const float lal = L.alpha, lbe = L.beta;
      const Post po = post_of(P);
      if constexpr (RES) {
        // The residual instantiation's own text of the loop below (act() only), unrolled over the
        // eight rows: carried[] indexed by a run-time b would live in scratch.
        const bool cons = (rm.cons >> l) & 1u, src = (rm.src >> l) & 1u;  // uniform
#pragma unroll
        for (int b = 0; b < GO2PI_SMALL_MAXB; ++b) {
          if (b < B) {
            float s = 0.f;
            for (int w2 = 0; w2 < LAT_WAVES; ++w2) s += part[(w2 * GO2PI_SMALL_MAXB + b) * 16 + lane];
            float sb = s + bv;
            if (cons) sb += carried[b], carried[b] = 0.f;  // (sum + bias) + carried; read once
            const float v = act_fn(la, lal, lbe, sb);
            if (src) carried[b] = v;  // behind the read: a layer may be both
            if (last) {
              if (n < LN) act[(size_t)b * LN + n] = post_fn(po, v);
              if (done && b == B - 1 && g == 0) {  // the completion word, as below
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                if (lane == 0 && T == 1) __hip_atomic_store(done, epoch0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
              }
            } else {
              const unsigned long long gv = ((unsigned long long)(epoch0 + (unsigned)l) << 32) | __float_as_uint(v);
              __hip_atomic_store(gran + (size_t)l * gstride + b * L.N_pad + n, gv, __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_AGENT);
            }
          }
        }
      } else {
      for (int b = 0; b < B; ++b) {
        float s = 0.f;
        for (int w2 = 0; w2 < LAT_WAVES; ++w2) s += part[(w2 * GO2PI_SMALL_MAXB + b) * 16 + lane];
        const float v = act_fn(la, lal, lbe, s + bv);
        if (last) {
          if (n < LN) {
            if constexpr (CTL) ctl_store(cv, b, n, post_fn(po, v));
            else act[(size_t)b * LN + n] = post_fn(po, v);
          }
          if (!CTL && done && b == B - 1 && g == 0) {
            // completion word for the host's spin (instead of a stream sync): every
            // action store of this tile drained and made system-visible first
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (lane == 0 && T == 1) __hip_atomic_store(done, epoch0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          }
        } else {
          const unsigned long long gv = ((unsigned long long)(epoch0 + (unsigned)l) << 32) | __float_as_uint(v);
          __hip_atomic_store(gran + (size_t)l * gstride + b * L.N_pad + n, gv, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
        }
      }
      }  // (the loop every other instantiation runs keeps its text and indentation)
    }
    lds_barrier();  // xs / part reused by the next layer (the granule stores stay in flight)
  }
  if constexpr (CTL) {
    if (g != 0) return;
    for (int e = tid; e < B * P.in_dim; e += LAT_WAVES * 64) ctl.obs[e] = okeep[e];
    if (ctl.status && tid < B) ctl.status[tid] = CL.nanf[tid];
    // completion word: every store of this workgroup drained and made system-visible first
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (done && tid == 0) __hip_atomic_store(done, epoch0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

__global__ __launch_bounds__(LAT_WAVES * 64) void policy_latency_kernel(const DevProgram *__restrict__ Pd,
                                                                        const float *obs, float *act, int B,
                                                                        unsigned epoch0, unsigned long long *gran,
                                                                        int gstride, unsigned *err, unsigned *done) {
  // the program lives in device memory (uploaded once): a ~60-byte kernarg
  // instead of the ~700-byte DevProgram keeps the per-launch host cost down
  latency_body<false>(*Pd, obs, act, B, epoch0, gran, gstride, err, done, DevCtl{});
}

__global__ __launch_bounds__(LAT_WAVES * 64) void policy_latency_ctl_kernel(const DevProgram *__restrict__ Pd, DevCtl C,
                                                                            int B, unsigned epoch0,
                                                                            unsigned long long *gran, int gstride,
                                                                            unsigned *err, unsigned *done) {
  latency_body<true>(*Pd, nullptr, nullptr, B, epoch0, gran, gstride, err, done, C);
}

// ... and the general instantiations (the LN pass, the second sweep round)
__global__ __launch_bounds__(LAT_WAVES * 64) void policy_latency_ln_kernel(const DevProgram *__restrict__ Pd,
                                                                           const float *obs, float *act, int B,
                                                                           unsigned epoch0, unsigned long long *gran,
                                                                           int gstride, unsigned *err, unsigned *done) {
  latency_body<false, true>(*Pd, obs, act, B, epoch0, gran, gstride, err, done, DevCtl{});
}

__global__ __launch_bounds__(LAT_WAVES * 64) void policy_latency_ctl_ln_kernel(const DevProgram *__restrict__ Pd,
                                                                               DevCtl C, int B, unsigned epoch0,
                                                                               unsigned long long *gran, int gstride,
                                                                               unsigned *err, unsigned *done) {
  latency_body<true, true>(*Pd, nullptr, nullptr, B, epoch0, gran, gstride, err, done, C);
}

// ... and the general instantiation of a program with observation skip inputs
__global__ __launch_bounds__(LAT_WAVES * 64) void policy_latency_skip_kernel(const DevProgram *__restrict__ Pd,
                                                                             const float *obs, float *act, int B,
                                                                             unsigned epoch0, unsigned long long *gran,
                                                                             int gstride, unsigned *err, unsigned *done) {
  latency_body<false, true, true>(*Pd, obs, act, B, epoch0, gran, gstride, err, done, DevCtl{});
}

// ... and the instantiation of a program with residual connections (the skip code too: a
// policy may have both, and the skip paths are uniform branches on skip_n)
__global__ __launch_bounds__(LAT_WAVES * 64) void policy_latency_res_kernel(const DevProgram *__restrict__ Pd,
                                                                            const float *obs, float *act, int B,
                                                                            unsigned epoch0, unsigned long long *gran,
                                                                            int gstride, unsigned *err, unsigned *done) {
  latency_body<false, true, true, true>(*Pd, obs, act, B, epoch0, gran, gstride, err, done, DevCtl{});
}

int latency_grid(const DevProgram &p) {
  int grid = 1;
  for (int l = 0; l < p.nl; ++l) grid = std::max(grid, p.L[l].N_pad >> 4);
  return grid;
}

LatencyLds latency_lds_of(const DevProgram &p, bool ctl) {
  return latency_lds(p.lds_stride, ctl ? latency_ctl_lds(p.in_dim).total : 0);
}

int launch_latency(const DevProgram &p, const DevProgram *p_dev, const float *obs, float *act, int batch,
                   unsigned epoch0,
                   unsigned long long *gran, int gstride, unsigned *err, unsigned *done, void *stream) {
  if (batch <= 0) return 0;
  if (batch > GO2PI_SMALL_MAXB) return (int)hipErrorInvalidValue;
  const int grid = latency_grid(p);
  const size_t lds = sizeof(float) * latency_lds_of(p, false).total;
  hipLaunchKernelGGL(program_has_res(p)         ? policy_latency_res_kernel
                     : program_has_skip(p)      ? policy_latency_skip_kernel
                     : program_small_general(p) ? policy_latency_ln_kernel
                                                : policy_latency_kernel,
                     dim3(grid), dim3(LAT_WAVES * 64), lds, reinterpret_cast<hipStream_t>(stream), p_dev, obs, act, batch,
                     epoch0, gran, gstride, err, done);
  return (int)hipGetLastError();
}

int launch_latency_ctl(const DevProgram &p, const DevProgram *p_dev, const DevCtl &ctl, int batch, unsigned epoch0,
                       unsigned long long *gran, int gstride, unsigned *err, unsigned *done, void *stream) {
  if (batch <= 0) return 0;
  // (no controller form reads a skip layer's observation columns: the engine refuses the tick)
  // (nor has one a carried value)
  if (batch > GO2PI_SMALL_MAXB || p.L[p.nl - 1].N_pad != 16 || program_has_skip(p) || program_has_res(p))
    return (int)hipErrorInvalidValue;
  const int grid = latency_grid(p);
  const size_t lds = sizeof(float) * latency_lds_of(p, true).total;
  hipLaunchKernelGGL(program_small_general(p) ? policy_latency_ctl_ln_kernel : policy_latency_ctl_kernel, dim3(grid),
                     dim3(LAT_WAVES * 64), lds, reinterpret_cast<hipStream_t>(stream), p_dev, ctl, batch, epoch0, gran,
                     gstride, err, done);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------
size_t fused_lds_bytes(const DevProgram &p, int waves) {
  // activation buffers + per-wave partial-sum scratch (head fusion: up to 2 tiles)
  // + the layer hand-off flags
  // (a program with residual connections: the carried tile, in the recurrent rows' slot)
  return sizeof(float) * (size_t)(2 + p.has_gru + (program_has_res(p) ? 1 : 0)) * GO2PI_TILE_ROWS * p.lds_stride +
         sizeof(f32x4) * 64 * waves * (p.head_fuse > 1 ? p.head_fuse : 1) + sizeof(float) * GO2PI_FLAG_FLOATS +
         sizeof(float) * p.w4_bias;
}

GemvLds gemv_lds_of(const DevProgram &p, int layer) { return gemv_lds(p.L[layer].K_pad); }

// The generic body's instantiations live in kernels_gen_w{4,8,16}.hip and the 4-wave
// pipeline's in kernels_w4_t{2,4,8}.hip (one translation unit each, compiled in
// parallel): gen_*<waves> / w4_*<tiles per wave>.
template <class F>
static int with_waves(int waves, F &&f) {
  switch (waves) {
    case 4: return f(std::integral_constant<int, 4>{});
    case 16: return f(std::integral_constant<int, 16>{});
    default: return f(std::integral_constant<int, 8>{});
  }
}

template <class F>
static int with_w4(const DevProgram &p, F &&f) {
  switch (p.w4_tpw) {
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    default: return f(std::integral_constant<int, 8>{});
  }
}

// the 4-wave LayerNormalization pipeline (kernels_w4ln_t{2,4,8}.hip), DevProgram::w4ln_tpw
template <class F>
static int with_w4ln(const DevProgram &p, F &&f) {
  switch (p.w4ln_tpw) {
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    default: return f(std::integral_constant<int, 8>{});
  }
}

// a residual program on the pipeline (kernels_w4res_t{2,4,8}.hip; GO2PI_RESIDUAL_BATCHED): the LN
// pipeline's fields, policy_mlp_res_kernel
static bool w4res_program(const DevProgram &p) { return p.w4ln_tpw != 0 && program_has_res(p); }

int configure_kernels(const DevProgram &p, int waves) {
  hipError_t e = hipSuccess;
  // (an LN pipeline program: its batched kernel, and the general body too, which serves its
  // controller tick; a residual pipeline program: likewise, the general residual kernel beside it)
  if (w4res_program(p)) {
    e = (hipError_t)with_w4ln(p, [&](auto t) { return w4res_configure<decltype(t)::value>(p); });
    if (e != hipSuccess) return (int)e;
  } else if (p.w4ln_tpw) {
    e = (hipError_t)with_w4ln(p, [&](auto t) { return w4ln_configure<decltype(t)::value>(p); });
    if (e != hipSuccess) return (int)e;
  }
  if (program_has_res(p))  // (kernels_gen_res.hip; the planner gives it 8 waves)
    e = (hipError_t)res_configure(p);
  else if (waves == 4 && p.w4_tpw)
    e = (hipError_t)with_w4(p, [&](auto t) { return w4_configure<decltype(t)::value>(p); });
  else
    e = (hipError_t)with_waves(waves, [&](auto w) { return gen_configure<decltype(w)::value>(p); });
  if (e != hipSuccess) return (int)e;
  int gmax = 0;
  for (int l = 0; l < p.nl; ++l) gmax = std::max(gmax, (int)sizeof(float) * gemv_lds_of(p, l).total);
  e = hipFuncSetAttribute(reinterpret_cast<const void *>(&gemv_layer_kernel),
                          hipFuncAttributeMaxDynamicSharedMemorySize, gmax);
  return (int)e;
}

int launch_policy_fused(const DevProgram &p, const DevProgram *p_dev, int waves, const float *obs, float *act,
                        float *hidden, int batch, int steps, void *stream) {
  if (batch <= 0 || steps <= 0) return 0;
  if (w4res_program(p))
    return with_w4ln(p, [&](auto t) {
      return w4res_launch<decltype(t)::value>(p, p_dev, obs, act, batch, steps, stream);
    });
  if (program_has_res(p)) return waves == 8 ? res_launch(p, p_dev, obs, act, batch, steps, stream) : (int)hipErrorInvalidValue;
  if (p.w4ln_tpw)
    return with_w4ln(p, [&](auto t) {
      return w4ln_launch<decltype(t)::value>(p, p_dev, obs, act, batch, steps, stream);
    });
  if (waves == 4 && p.w4_tpw)
    return with_w4(p, [&](auto t) {
      return w4_launch<decltype(t)::value>(p, p_dev, obs, act, hidden, batch, steps, stream);
    });
  return with_waves(waves, [&](auto w) {
    return gen_launch<decltype(w)::value>(p, p_dev, obs, act, hidden, batch, steps, stream);
  });
}

int batched_kernel_name(const DevProgram &p, int waves, char *buf, size_t cap) {
  if (w4res_program(p)) return with_w4ln(p, [&](auto t) { return w4res_name<decltype(t)::value>(p, buf, cap); });
  if (program_has_res(p)) return res_name(p, buf, cap);
  if (p.w4ln_tpw) return with_w4ln(p, [&](auto t) { return w4ln_name<decltype(t)::value>(p, buf, cap); });
  if (waves == 4 && p.w4_tpw) return with_w4(p, [&](auto t) { return w4_name<decltype(t)::value>(p, buf, cap); });
  return with_waves(waves, [&](auto w) { return gen_name<decltype(w)::value>(p, buf, cap); });
}

const char *latency_kernel_name() { return "policy_latency_kernel"; }
const char *gemv_kernel_name() { return "gemv_layer_kernel"; }

int launch_policy_fused_ctl(const DevProgram &p, const DevProgram *p_dev, int waves, const DevCtl &ctl,
                            float *hidden, int batch, void *stream) {
  if (batch <= 0) return 0;
  const size_t lds = fused_ctl_lds_bytes(p, waves);
  if (lds > 160 * 1024) return (int)hipErrorInvalidValue;
  if (waves == 4 && p.w4_tpw)
    return with_w4(p, [&](auto t) { return w4_launch_ctl<decltype(t)::value>(p, p_dev, ctl, hidden, batch, stream); });
  return with_waves(waves, [&](auto w) {
    return gen_launch_ctl<decltype(w)::value>(p, p_dev, ctl, hidden, batch, stream);
  });
}

int launch_gemv_layer(const DevProgram &p, int layer, const float *obs, const float *x, int x_stride, float *y,
                      int y_stride, int batch, void *stream, const float *cin, float *cout, int c_stride) {
  if (batch <= 0) return 0;
  if (batch > GO2PI_SMALL_MAXB) return (int)hipErrorInvalidValue;
  // a residual layer without its carried rows, or one buffer for both directions
  if ((p.res[layer] != 0) != (cin != nullptr) || (cin && cin == cout)) return (int)hipErrorInvalidValue;
  const dim3 grid(p.L[layer].N_pad >> 4);
  hipLaunchKernelGGL(gemv_layer_kernel, grid, dim3(GEMV_WAVES * 64), sizeof(float) * gemv_lds_of(p, layer).total,
                     reinterpret_cast<hipStream_t>(stream), p, layer, obs, x, x_stride, y, y_stride, batch, cin, cout,
                     c_stride);
  return (int)hipGetLastError();
}

}  // namespace go2pi
