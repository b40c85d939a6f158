// The tiled layer body of the small-batch (1..8 rows) kernels, stated once.
//
// Three kernels run this recipe: gemv_layer_kernel (one launch per layer) and latency_body (one
// launch per call) in kernels.hip, and the layer loop of policy_resident_kernel (no launch per
// call) in resident.hip. gemv_layer_kernel calls the functions below. The other two keep
// their own text of the same steps: called from here, the same source compiled to code that
// answered a batch-1 request 0.3-0.7 us later (DESIGN section 4.2g has the measurements), and
// a launch per layer hides what those two cannot. tests/test_gpu_small_forms.py holds the
// three to the same bits, so the order below is the contract for all of them.
//
// The recipe. One workgroup owns a 16-output tile of a layer; TILE_WAVES waves split its
// k-chunks (16 input columns each): wave w owns chunks w, w + 8, ..., the first TILE_MAXS of
// them as fragments in registers (tile_load). The layer's input rows stand in LDS as
// [B][K_pad] floats (stage_obs / stage_gather for layer 0).
//
// The summation order of output n = 16 tile + j, row b (tile_dot, tile_finish):
//   1. lane (q, j) = 16 q + j of wave w runs ONE fma chain, p = 0, over its chunks c = w, w + 8,
//      ... ascending, and inside a chunk over k = 16 c + 4 q + 0, 1, 2, 3: p = fmaf(x[k], w[k], p);
//   2. the wave's four quarter sums: p += p[lane ^ 16], then p += p[lane ^ 32];
//   3. lanes 0..15 store p to part[w][b][j]; one barrier; the publishing wave's lane j sums
//      s = 0, s += part[w][b][j] for w = 0 .. 7 in that order;
//   4. v = act(s + bias), or act((s + bias) + carried) with a carried residual row.
// No step depends on B, on the row's place in the batch, or on the kernel around it.
//
// LDS pointers come in as plain float pointers and are cast to their address space inside
// (as ln_rows does): 32-bit addresses, and no register pair per fragment read.
#pragma once

#include <hip/hip_runtime.h>

#include "device_fn.hpp"
#include "program.hpp"

namespace go2pi {

constexpr int TILE_WAVES = lds::WAVES;
constexpr int TILE_MAXS = 8;   // chunk slots per wave held in registers: K_pad <= 8 * 8 * 16 = 1024

typedef float tile_f32x4_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) tile_f32x4_t lds_f32x4_t;

// Wave `wave`'s fragments of tile `tile` of a layer of T tiles and C chunks (program.hpp's
// chunk-major packing), chunk wave + 8 s in slot s; zeros past the layer's chunks.
__device__ __forceinline__ void tile_load(float4 (&wr)[TILE_MAXS], const float *w, int tile, int T, int C, int wave,
                                          int lane) {
  const float4 *W = reinterpret_cast<const float4 *>(w) + (size_t)tile * 64 + lane;
#pragma unroll
  for (int s = 0; s < TILE_MAXS; ++s) {
    const int c = wave + s * TILE_WAVES;
    wr[s] = c < C ? W[(size_t)c * T * 64] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// Steps 1 to 3 of the order above, up to the store to part (the caller's barrier follows).
// The cross-lane steps run for all eight rows (the values of rows b >= B are never stored).
// tail(c): the fragment of a chunk past the register slots (K_pad > 1024), read from memory.
// wave, lane: the caller's threadIdx.x >> 6 (made uniform) and threadIdx.x & 63 of a
//   one-dimensional workgroup of TILE_WAVES waves: the lane's LDS base below is built from
//   threadIdx.x itself and relies on that.
template <class Tail>
__device__ __forceinline__ void tile_dot(const float *xs, float *part, const float4 (&wr)[TILE_MAXS], int K_pad, int C,
                                         int B, int wave, int lane, Tail tail) {
  const lds_float *xl = (const lds_float *)xs;
  lds_float *pl = (lds_float *)part;
  float p[GO2PI_SMALL_MAXB];
#pragma unroll
  for (int b = 0; b < GO2PI_SMALL_MAXB; ++b) p[b] = 0.f;
  // the lane's columns of the wave's first chunk, from the thread index and not from `wave`
  // (uniform): as one per-lane value, a register slot's address is its row's base plus an
  // immediate 128 s floats, and the eight slot offsets need no scalar registers (the callers
  // have none to spare: 106 of 106).
  xl += ((threadIdx.x >> 6) << 4) + ((lane >> 4) << 2);
  auto chunk = [&](int c, const float4 &w) {
#pragma unroll
    for (int b = 0; b < GO2PI_SMALL_MAXB; ++b) {
      if (b < B) {
        const tile_f32x4_t a = *(const lds_f32x4_t *)(xl + b * K_pad + (c - wave) * 16);
        p[b] = fmaf(a.x, w.x, p[b]);
        p[b] = fmaf(a.y, w.y, p[b]);
        p[b] = fmaf(a.z, w.z, p[b]);
        p[b] = fmaf(a.w, w.w, p[b]);
      }
    }
  };
#pragma unroll
  for (int s = 0; s < TILE_MAXS; ++s) {
    const int c = wave + s * TILE_WAVES;
    if (c >= C) break;
    chunk(c, wr[s]);
  }
  for (int c = wave + TILE_MAXS * TILE_WAVES; c < C; c += TILE_WAVES) chunk(c, tail(c));
#pragma unroll
  for (int b = 0; b < GO2PI_SMALL_MAXB; ++b) {
    p[b] += __shfl_xor(p[b], 16);
    p[b] += __shfl_xor(p[b], 32);
  }
  if (lane < 16) {
#pragma unroll
    for (int b = 0; b < GO2PI_SMALL_MAXB; ++b)
      if (b < B) pl[(wave * GO2PI_SMALL_MAXB + b) * 16 + lane] = p[b];
  }
}

// Steps 3 (behind the caller's barrier) and 4. Called by lanes 0..15 of the publishing wave
// alone (wave 0 in the chain): the caller tests for them, so that what its store needs is
// loaded by those lanes and not by every wave between the two barriers.
// Each row's value goes to store(b, n, v, last). carried: a residual consumer's rows
// [b][c_stride] (the chain), added after the bias and in front of the activation; null: none.
template <class Store>
__device__ __forceinline__ void tile_finish(const float *part, int tile, int lane, int B, float bias, ActP ap,
                                            bool last, const float *carried, int c_stride, Store store) {
  const lds_float *pl = (const lds_float *)part;
  const int n = tile * 16 + lane;
  for (int b = 0; b < B; ++b) {
    float s = 0.f;
    for (int w = 0; w < TILE_WAVES; ++w) s += pl[(w * GO2PI_SMALL_MAXB + b) * 16 + lane];
    float sb = s + bias;
    if (carried) sb += carried[(size_t)b * c_stride + n];
    store(b, n, act_fn(ap.act, ap.alpha, ap.beta, sb), last);
  }
}

// Layer 0's input rows xs[B][K_pad] from the observation rows src[B][stride]: column k < in_dim
// through the prologue, zeros behind.
__device__ __forceinline__ void stage_obs(const DevProgram &P, const float *src, int stride, float *xs, int K_pad, int B,
                                          int tid) {
  for (int e = tid; e < B * K_pad; e += TILE_WAVES * 64) {
    const int b = e / K_pad, k = e - b * K_pad;
    xs[e] = k < P.in_dim ? prologue(P, src[(size_t)b * stride + k], k) : 0.f;
  }
}

// ... and of a layer 0 that gathers (DevLayer::skip_n on layer 0): column k < sn is
// observation column sidx[k] through that column's prologue.
__device__ __forceinline__ void stage_gather(const DevProgram &P, const float *src, int stride, const int *sidx, int sn,
                                             float *xs, int K_pad, int B, int tid) {
  for (int e = tid; e < B * K_pad; e += TILE_WAVES * 64) {
    const int b = e / K_pad, k = e - b * K_pad;
    float v = 0.f;
    if (k < sn) {
      const int c = sidx[k];
      v = prologue(P, src[(size_t)b * stride + c], c);
    }
    xs[e] = v;
  }
}

}  // namespace go2pi
