// The 4-wave pipeline for dense policies with LayerNormalization: policy_mlp_ln_kernel<TPW, HT>
// (opts.ln_small bit GO2PI_LN_BATCHED; plan.cpp decides, kernels_w4ln.inc launches), and the
// same body with residual connections, policy_mlp_res_kernel<TPW, HT> (GO2PI_RESIDUAL_BATCHED,
// kernels_w4res.inc; the RES parameter of w4ln_body and w4ln_epi, described at w4ln_body).
//
// The pipeline is w4_step's (fused_impl.hpp), built from the same parts (w4_prefill,
// w4_lds_phase, w4_chunk, w4_wait): 4 waves, one 16-robot tile per workgroup, wave w owns
// output tiles [w * TPW, (w + 1) * TPW) of every hidden layer; the register ring of weight
// fragments by buffer loads, prefetched across layers; at 4 and 8 tiles per wave the layer
// hand-off by flags with the wave's own chunks fed from registers, at 2 tiles per wave an
// epilogue + barrier + natural chunk order; the head fed from registers on four accumulator
// chains, its partial sums added in wave order. The hidden activation, the hidden-layer count
// and every layer's LN mode are read at run time, layer 0's K is padded to 64 (a multiple of
// 4 chunks), and the kernel loops over `steps` (go2pi_run_sequence_device).
//
// What is new is the epilogue of a layer with a LayerNormalization (w4ln_epi): the row
// statistics are taken from the accumulators' registers, so the row is not read back from
// LDS as the general body's separate pass (ln_tile) does.
//
// A lane holds, per own tile i, four consecutive columns of robot lane & 15: columns
// (t0 + i) * 16 + 4 * (lane >> 4) + j. A robot's row is therefore spread over 4 lane groups
// (lanes r, r + 16, r + 32, r + 48) x 4 waves. Per statistic:
//  1. the lane's partial over its 4 * TPW columns, ascending;
//  2. the four lane groups by two lane swaps (w4ln_group_sum), no LDS;
//  3. the four waves through a 64-float LDS region and one LDS-only barrier, added in wave
//     order 0..3 by every wave: every wave holds the same bits.
// The variance is that of x - mean in a second pass over the registers (as ln_rows). Columns
// >= N (the layer's true width) are excluded by index and written as act(0) or 0: finite
// values against the next layer's zero weight columns. The order of every addition depends
// on the column index, N and the wave number alone, never on the row's place in a tile or
// batch: shards and repeats are bitwise equal. The order differs from ln_rows', so the
// result is within the tolerance of the general body's, not its bits.
//
// Barriers: the LN mode of a layer is a workgroup-uniform scalar (read from the program), so
// all four waves pass the same barriers. Two statistic regions suffice for every layer: a
// wave writes `sum` before barrier 1 and reads it behind it; it writes `sum` again (the next
// LN layer) only behind barrier 2 of this layer, which no wave passes before every wave has
// arrived there, its reads of `sum` complete (lds_barrier waits lgkmcnt(0)). Likewise `var`
// is written before barrier 2, read behind it, and written again only behind the next LN
// layer's barrier 1, where every wave arrives with its reads of `var` complete.
#pragma once

#include "fused_impl.hpp"
#include "w4ln_layout.hpp"

namespace go2pi {

// Sum over the four lane groups of a row (lanes r, r + 16, r + 32, r + 48), the same value
// in all four: (v[r] + v[r + 32]) + (v[r + 16] + v[r + 48]). v_permlane32_swap exchanges rows
// 2-3 of its first operand with rows 0-1 of its second, v_permlane16_swap the odd rows of
// the first with the even rows of the second (a row: 16 lanes); with both operands the same
// value the two results are "the lower half's" and "the upper half's" in every lane.
// Builtins, not inline asm: the operands are MFMA results (the compiler places the hazard nops).
__device__ __forceinline__ float w4ln_group_sum(float v) {
  const unsigned u = __builtin_bit_cast(unsigned, v);
  const auto a = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  const float s = __builtin_bit_cast(float, (unsigned)a[0]) + __builtin_bit_cast(float, (unsigned)a[1]);
  const unsigned us = __builtin_bit_cast(unsigned, s);
  const auto b = __builtin_amdgcn_permlane16_swap(us, us, false, false);
  return __builtin_bit_cast(float, (unsigned)b[0]) + __builtin_bit_cast(float, (unsigned)b[1]);
}

// the row statistic of every robot row: this wave's group sums into its slots of `reg`
// ([16 rows][4 waves]), one LDS-only barrier (the ring's loads stay in flight), then the
// four waves' partials added in wave order
__device__ __forceinline__ float w4ln_row_sum(float part, float *reg, int wave, int lane) {
  const float s = w4ln_group_sum(part);
  if (lane < 16) reg[lane * W4LN_WAVES + wave] = s;
  lds_barrier();
  const float4 p = *reinterpret_cast<const float4 *>(reg + (lane & 15) * W4LN_WAVES);
  return ((p.x + p.y) + p.z) + p.w;
}

template <int TPW>
__device__ __forceinline__ void w4ln_act(float4 (&v)[TPW], const ActP &ap) {
  if (ap.act == 0) return;
  with_act(ap.act, [&](auto act_k) {
    constexpr int ACT = decltype(act_k)::value;
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
      v[i].x = act_t<ACT>(ap, v[i].x);
      v[i].y = act_t<ACT>(ap, v[i].y);
      v[i].z = act_t<ACT>(ap, v[i].z);
      v[i].w = act_t<ACT>(ap, v[i].w);
    }
  });
}

// A hidden layer's epilogue for the wave's TPW tiles: v = the layer's output (the next
// layer's B operand). lp: this lane's bias float4 of tile t0 of this layer in the LDS pack,
// Scale and B `gofs` and 2 * gofs floats behind it; mode: 0 act(x), 1 act(LN(x)), 2 LN(act(x));
// col0: this lane's first column of tile t0.
// RES (policy_mlp_res_kernel): the layer's residual connection, on the registers. cons: the
// layer adds the carried value, (acc + bias) + carried, in front of the activation and the LN
// (the order of dense_store, tile_finish and the small-batch forms); src: it then keeps what
// its dense store would write before any LN pass, the raw sum of a pre-LN layer (mode 1: no
// activation yet) and the activated value of mode 0 and mode 2. A layer that is both reads
// before it overwrites. carried: the lane's TPW values. Without RES nothing of this is compiled.
template <int TPW, bool RES = false>
__device__ __forceinline__ void w4ln_epi(float4 (&v)[TPW], const f32x4 (&acc)[TPW], const float *lp, int gofs, int mode,
                                         float eps, int N, const ActP &ap, int col0, float *rsum, float *rvar,
                                         int wave, int lane, [[maybe_unused]] float4 *carried = nullptr,
                                         [[maybe_unused]] bool cons = false, [[maybe_unused]] bool src = false) {
#pragma unroll
  for (int i = 0; i < TPW; ++i) {
    const float4 bv = *reinterpret_cast<const float4 *>(lp + i * 16);
    v[i] = make_float4(acc[i][0] + bv.x, acc[i][1] + bv.y, acc[i][2] + bv.z, acc[i][3] + bv.w);
  }
  if constexpr (RES) {
    if (cons) {
#pragma unroll
      for (int i = 0; i < TPW; ++i)
        v[i] = make_float4(v[i].x + carried[i].x, v[i].y + carried[i].y, v[i].z + carried[i].z, v[i].w + carried[i].w);
    }
  }
  if (mode != 1) w4ln_act<TPW>(v, ap);
  if constexpr (RES) {
    if (src) {
#pragma unroll
      for (int i = 0; i < TPW; ++i) carried[i] = v[i];
    }
  }
  if (mode == 0) return;
  const float fn = (float)N;
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < TPW; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) s += col0 + i * 16 + j < N ? f4c(v[i], j) : 0.f;
  const float mean = w4ln_row_sum(s, rsum, wave, lane) / fn;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < TPW; ++i) {
    float d[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      d[j] = col0 + i * 16 + j < N ? f4c(v[i], j) - mean : 0.f;
      q = fmaf(d[j], d[j], q);
    }
    v[i] = make_float4(d[0], d[1], d[2], d[3]);
  }
  const float rstd = 1.f / sqrtf(w4ln_row_sum(q, rvar, wave, lane) / fn + eps);
#pragma unroll
  for (int i = 0; i < TPW; ++i) {
    const float4 g = *reinterpret_cast<const float4 *>(lp + gofs + i * 16);
    const float4 b = *reinterpret_cast<const float4 *>(lp + 2 * gofs + i * 16);
    const int c = col0 + i * 16;
    // (a column past N: 0, whatever rstd is)
    v[i].x = c + 0 < N ? fmaf(v[i].x * rstd, g.x, b.x) : 0.f;
    v[i].y = c + 1 < N ? fmaf(v[i].y * rstd, g.y, b.y) : 0.f;
    v[i].z = c + 2 < N ? fmaf(v[i].z * rstd, g.z, b.z) : 0.f;
    v[i].w = c + 3 < N ? fmaf(v[i].w * rstd, g.w, b.w) : 0.f;
  }
  if (mode == 1) w4ln_act<TPW>(v, ap);
}

// The residual kernel's state (w4ln_body, RES): the two layer masks and the lane's carried value.
template <int TPW, bool RES>
struct W4ResState {};
template <int TPW>
struct W4ResState<TPW, true> {
  unsigned consm, srcm;
  float4 carried[TPW];
};

// dims = in_dim | c0 << 12 | hidden layers << 20 (c0: layer 0's k-chunks, a multiple of 4).
// pack: DevProgram::bpack of an LN pipeline program (program.hpp w4ln_tpw).
//
// RES (policy_mlp_res_kernel<TPW, HT>, GO2PI_RESIDUAL_BATCHED): residual connections
// (DevProgram::res). Wave w owns the same tiles of every hidden layer and all hidden layers
// have one padded width, so a lane holds the same (robot, column) elements in v[] at every
// hidden layer's epilogue, and a consumer has the width of its source (loader rule): the
// carried value stays in the lane's registers (carried[TPW]) from the source's epilogue to
// the consumer's, with no LDS tile, no barrier and no traffic. P.res[] is read once into two
// scalar masks; carried[] is zero at the start of every step. The hidden layers need not
// share an activation (SimBa: none / Relu / none), so each layer's is read from P.L[l] (a
// pre-LN layer's from its ln_act), never from the hot block's hid_act; a layer without LN runs
// mode 0 against zero Scale / B in the pack. The loader refuses an Add on the output layer:
// the head is the LN kernel's.
// Pad columns (>= N) under RES: their weight rows and biases are zero, so such a column holds
// act(0), or act(0 + carried) where the carried pad is itself such a value: a finite sum of
// act(0) constants of the layers before, the same in every row. It is excluded from every LN by
// index (and written 0 behind one), and it meets only zero weight columns in the next layer
// and the head (a consumer's N is its source's N, and every layer's K is its predecessor's N).
// The order of every addition still depends on the column, N and the wave alone.
template <int TPW, int HT, bool RES = false>
__device__ __forceinline__ void w4ln_body(const DevProgram &P, const float *__restrict__ obs, float *__restrict__ act,
                                          const float *l0w, const float *pack, int B, int steps, unsigned dims,
                                          unsigned *yield) {
  constexpr int NW = W4LN_WAVES;
  constexpr int RD = GO2PI_W4_RD(TPW);
  constexpr int CH = NW * TPW;    // k-chunks of every layer after the first = output tiles of a hidden layer
  constexpr int W = 16 * CH;      // the hidden layers' padded width
  constexpr int CSB = CH * 1024;  // bytes per k-chunk of a layer's fragments
  constexpr bool HO = TPW >= 4;   // the register hand-off (w4_step)
  constexpr W4LnLds LY = w4ln_lds(TPW, HT, 0);  // (the pack is the last region: no offset depends on nh)
  constexpr int S = LY.stride;
  static_assert(TPW == 2 || TPW == 4 || TPW == 8, "tiles per wave");
  static_assert(HT == 1 || (HT == 2 && TPW < 8), "head tiles");
  extern __shared__ float4 lds4[];
  float *lds = reinterpret_cast<float *>(lds4);
  // tell idle resident kernels on this device to give their CUs back (resident.hip)
  if (blockIdx.x == 0 && threadIdx.x == 0 && gridDim.x > GO2PI_YIELD_MIN_GRID)
    __hip_atomic_fetch_add(yield, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int in_dim = (int)(dims & 0xFFFu), c0 = (int)((dims >> 12) & 0xFFu), nh = (int)((dims >> 20) & 0xFFu);
  float *bufA = lds + LY.xa.off, *bufB = lds + LY.xb.off;
  f32x4 *scratch = reinterpret_cast<f32x4 *>(lds + LY.scratch.off);
  int *flags = reinterpret_cast<int *>(lds + LY.flags.off);
  float *rsum = lds + LY.sum.off, *rvar = lds + LY.var.off, *lpack = lds + LY.pack.off;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int row0 = blockIdx.x * GO2PI_TILE_ROWS;
  const int nch = (16 * c0 + 63) >> 6;  // 64-column chunks of the observation tile
  const int t0 = wave * TPW;
  const int kb1 = HO ? t0 : 0;  // first k-chunk of every layer after the first
  const int gofs = nh * W;      // floats from a layer's bias to its Scale, and from Scale to B, in the pack
  const int col0 = t0 * 16 + ((lane >> 4) << 2);
  int vo[TPW];  // per-lane byte offset of each own tile's fragment in chunk 0 (every layer)
#pragma unroll
  for (int i = 0; i < TPW; ++i) vo[i] = ((t0 + i) * 64 + lane) * 16;
  auto layer_w = [&](int l) { return l0w + (size_t)(c0 + (l - 1) * CH) * CH * 256; };  // (w4_layer_w)
  int ep = 0;  // flag epochs published so far (the same in every wave)
  // (RES) consm bit l: hidden layer l adds the carried value; srcm bit l: its value is one.
  // Read here, once (as fused_body reads them): the per-layer tests are scalar arithmetic
  // (and the carried value itself; without RES the struct is empty)
  [[maybe_unused]] W4ResState<TPW, RES> rs;
  if constexpr (RES) {
    unsigned consm = 0, srcm = 0;
#pragma unroll
    for (int l = 0; l < GO2PI_MAX_LAYERS; ++l) {
      const unsigned r = l < nh ? (unsigned)P.res[l] : 0u;  // j + 1, 0: none
      consm |= (r != 0u ? 1u : 0u) << l;
      srcm |= r ? 1u << (r - 1) : 0u;
    }
    rs.consm = __builtin_amdgcn_readfirstlane(consm);
    rs.srcm = __builtin_amdgcn_readfirstlane(srcm);
  }
  // (RES) the epilogue's activation of hidden layer PL: the layer's own, a pre-LN layer's from its ln_act
  [[maybe_unused]] auto layer_act = [](const DevLayer &PL, int mode) {
    const bool pre = mode == 1;
    return ActP{__builtin_amdgcn_readfirstlane(pre ? PL.ln_act : PL.act), pre ? PL.ln_alpha : PL.alpha,
                pre ? PL.ln_beta : PL.beta};
  };
  for (int step = 0; step < steps; ++step) {
    // wave w stages rows w, w + NW, ... in whole 64-column chunks by direct-to-LDS loads;
    // padding lanes read an element of the same row (times a zero weight column), rows past
    // B the last row
    const float *ob = obs + (size_t)step * B * in_dim;
#pragma unroll
    for (int i = 0; i < GO2PI_TILE_ROWS / NW; ++i) {
      const int r = wave + NW * i, row = min(row0 + r, B - 1);
      const float *rp = ob + (size_t)row * in_dim;
      for (int c = 0; c < nch; ++c)
        __builtin_amdgcn_global_load_lds((gvoid_t *)(rp + min(c * 64 + lane, in_dim - 1)),
                                         (lvoid_t *)(bufA + r * S + c * 64), 4, 0, 0);
    }
    if (step == 0 && tid < NW) flags[tid] = 0;
    // biases, Scale and B of every hidden layer into LDS once, in flight with the observation tile
    if (step == 0) glds_copy(lpack, pack, 3 * gofs, wave, lane, NW);
    float4 f[4][TPW];
    asm volatile("" ::: "memory");  // the DMA loads stay ahead of the ring's first loads
    w4_prefill<TPW, 0, NW>(l0w, f, wave, lane);
    asm volatile("" ::: "memory");
    // the program's fields, behind the first loads (their round trip overlaps those)
    const float *hwp = P.head_w, *hbp = P.head_bias;
    unsigned *err = P.err_hot;
    const int head_n = P.head_n, head_act = P.head_act;
    const float head_alpha = P.head_alpha, head_beta = P.head_beta;
    // (RES: not used, and so not read: every epilogue takes its layer's own, layer_act)
    [[maybe_unused]] const ActP ap{P.hid_act, P.hid_alpha, P.hid_beta};
    if constexpr (RES) {
#pragma unroll
      for (int i = 0; i < TPW; ++i) rs.carried[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // layer 0's input rows and the pack are in LDS (this wave's direct-to-LDS loads, older
    // than the ring's RD * TPW loads, which stay in flight)
    wg_barrier_vm<RD * TPW>();
    // the head's fragments and bias by buffer loads (vmcnt alone), in front of the last LDS phase
    float4 hw[HT][TPW], hbv;
    auto load_head = [&] {
      hbv = WStream(hbp).ld(((wave < HT ? wave : 0) * 16 + ((lane >> 4) << 2)) * 4, 0);
      const WStream wh(hwp);
#pragma unroll
      for (int h = 0; h < HT; ++h)
#pragma unroll
        for (int i = 0; i < TPW; ++i) hw[h][i] = wh.ld((((t0 + i) * HT + h) * 64 + lane) * 16, 0);
    };
    if (nh == 1) load_head();
    // layer 0: the observation tile, natural chunk order; the tail fetches layer 1's first chunks
    f32x4 acc[TPW];
#pragma unroll
    for (int i = 0; i < TPW; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    {
      const WStream ws(l0w);
      if (nh > 1) {
        const WStream wn(layer_w(1));
        w4_lds_phase<TPW, RD, 0, 4, true>(bufA, S, lane, c0, 0, 0, ws, CSB, wn, CSB, kb1, CH, vo, acc, f);
      } else {
        w4_lds_phase<TPW, RD, 0, 4, false>(bufA, S, lane, c0, 0, 0, ws, CSB, ws, 0, 0, 1, vo, acc, f);
      }
    }
    float *Y = bufB;  // where the previous layer's activations go
    const float *lp0 = lpack + col0;
    for (int l = 1; l < nh; ++l) {
      const bool more = l + 1 < nh;
      const WStream ws(layer_w(l)), wn(layer_w(more ? l + 1 : l));
      const DevLayer &PL = P.L[l - 1];
      const int mode = __builtin_amdgcn_readfirstlane(PL.ln), N = __builtin_amdgcn_readfirstlane(PL.N);
      const float eps = PL.ln_eps;
      f32x4 accn[TPW];
#pragma unroll
      for (int i = 0; i < TPW; ++i) accn[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      float *yrow = Y + (lane & 15) * S + col0;
      // layer l - 1's epilogue for all the wave's tiles, to registers and to LDS
      float4 v[TPW];
      if constexpr (RES)
        w4ln_epi<TPW, true>(v, acc, lp0 + (l - 1) * W, gofs, mode, eps, N, layer_act(PL, mode), col0, rsum, rvar, wave,
                            lane, rs.carried, (rs.consm >> (l - 1)) & 1u, (rs.srcm >> (l - 1)) & 1u);
      else
        w4ln_epi<TPW>(v, acc, lp0 + (l - 1) * W, gofs, mode, eps, N, ap, col0, rsum, rvar, wave, lane);
#pragma unroll
      for (int i = 0; i < TPW; ++i) *reinterpret_cast<float4 *>(yrow + i * 16) = v[i];
      if constexpr (HO) {
        // own phase: layer l's MFMAs over the wave's own chunks with the B operand from
        // registers; the tiles are published behind the first chunk (their stores have
        // landed by then), then the other waves' flags are awaited
        auto publish = [&] {
          ++ep;
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's tile stores are in LDS
          if (lane == 0) __hip_atomic_store(flags + wave, ep, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        };
        [&]<int... I>(std::integer_sequence<int, I...>) {
          ((w4_chunk<TPW, (I & 3), RD, true, true>(accn, f, v[I], ws, vo, ((t0 + I + RD) & (CH - 1)) * CSB),
            I == 0 ? publish() : void()),
           ...);
        }(std::make_integer_sequence<int, TPW>{});
        w4_wait<NW>(flags, wave, ep, lane, err);
      } else {
        lds_barrier();  // every wave's tiles are in LDS; the ring's loads stay in flight
      }
      // LDS phase: the other waves' chunks, rotated order from t0 + TPW (2 tiles per wave: every chunk)
      constexpr int K0 = HO ? TPW : 0;
      constexpr int NT = (CH - K0) % 4 ? (CH - K0) % 4 : 4;
      if (more) {
        w4_lds_phase<TPW, RD, (K0 & 3), NT, true>(Y, S, lane, CH, kb1, K0, ws, CSB, wn, CSB, kb1, CH, vo, accn, f);
      } else {
        load_head();
        w4_lds_phase<TPW, RD, (K0 & 3), NT, false>(Y, S, lane, CH, kb1, K0, ws, CSB, wn, CSB, 0, 1, vo, accn, f);
      }
#pragma unroll
      for (int i = 0; i < TPW; ++i) acc[i] = accn[i];
      Y = Y == bufA ? bufB : bufA;
    }
    // the last hidden layer's epilogue feeds the head from registers (no LDS copy): four
    // accumulator chains per head tile, one per k-step of a chunk, summed (c0 + c1) + (c2 + c3)
    {
      const DevLayer &PL = P.L[nh - 1];
      const int mode = __builtin_amdgcn_readfirstlane(PL.ln), N = __builtin_amdgcn_readfirstlane(PL.N);
      const float eps = PL.ln_eps;
      float4 v[TPW];
      if constexpr (RES)
        w4ln_epi<TPW, true>(v, acc, lp0 + (nh - 1) * W, gofs, mode, eps, N, layer_act(PL, mode), col0, rsum, rvar, wave,
                            lane, rs.carried, (rs.consm >> (nh - 1)) & 1u, (rs.srcm >> (nh - 1)) & 1u);
      else
        w4ln_epi<TPW>(v, acc, lp0 + (nh - 1) * W, gofs, mode, eps, N, ap, col0, rsum, rvar, wave, lane);
      f32x4 hacc[HT][4];
#pragma unroll
      for (int h = 0; h < HT; ++h)
#pragma unroll
        for (int c = 0; c < 4; ++c) hacc[h][c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < TPW; ++i)
#pragma unroll
        for (int h = 0; h < HT; ++h)
#pragma unroll
          for (int j = 0; j < 4; ++j) hacc[h][j] = mfma4(f4c(hw[h][i], j), f4c(v[i], j), hacc[h][j]);
#pragma unroll
      for (int h = 0; h < HT; ++h)
        scratch[(h * NW + wave) * 64 + lane] = (hacc[h][0] + hacc[h][1]) + (hacc[h][2] + hacc[h][3]);
    }
    __syncthreads();
    if (wave < HT) {  // head tile `wave`: the four waves' partials in wave order, bias, final store
      f32x4 hs = scratch[(wave * NW) * 64 + lane];
#pragma unroll
      for (int w = 1; w < NW; ++w) hs += scratch[(wave * NW + w) * 64 + lane];
      const int row = row0 + (lane & 15), n0 = wave * 16 + ((lane >> 4) << 2);
      float4 o4 = make_float4(hs[0] + hbv.x, hs[1] + hbv.y, hs[2] + hbv.z, hs[3] + hbv.w);
      if (head_act != 0) {  // (the exported policies' heads have none)
        o4.x = act_fn(head_act, head_alpha, head_beta, o4.x);
        o4.y = act_fn(head_act, head_alpha, head_beta, o4.y);
        o4.z = act_fn(head_act, head_alpha, head_beta, o4.z);
        o4.w = act_fn(head_act, head_alpha, head_beta, o4.w);
      }
      if (row < B) {
        float *o = act + ((size_t)step * B + row) * head_n;
        if ((head_n & 3) == 0 && ((uintptr_t)act & 15) == 0) {  // (12 actions: one 16-byte store per lane)
          if (n0 < head_n) *reinterpret_cast<float4 *>(o + n0) = o4;
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (n0 + r < head_n) o[n0 + r] = f4c(o4, r);
        }
      }
    }
  }
}

// Argument order = preload order (the unit is built with -amdgpu-kernarg-preload-count=16;
// these are 13 dwords), as policy_mlp_seq_kernel's.
template <int TPW, int HT>
__global__ __launch_bounds__(256) void policy_mlp_ln_kernel(const float *__restrict__ obs, float *__restrict__ act,
                                                            const float *__restrict__ l0w,
                                                            const float *__restrict__ pack,
                                                            const DevProgram *__restrict__ Pd, int B, int steps,
                                                            unsigned dims, unsigned *yield) {
  w4ln_body<TPW, HT>(*Pd, obs, act, l0w, pack, B, steps, dims, yield);
}

// The same pipeline with residual connections (w4ln_body's RES; GO2PI_RESIDUAL_BATCHED,
// kernels_w4res.inc launches): a residual program with or without LayerNormalization.
template <int TPW, int HT>
__global__ __launch_bounds__(256) void policy_mlp_res_kernel(const float *__restrict__ obs, float *__restrict__ act,
                                                             const float *__restrict__ l0w,
                                                             const float *__restrict__ pack,
                                                             const DevProgram *__restrict__ Pd, int B, int steps,
                                                             unsigned dims, unsigned *yield) {
  w4ln_body<TPW, HT, true>(*Pd, obs, act, l0w, pack, B, steps, dims, yield);
}

}  // namespace go2pi
