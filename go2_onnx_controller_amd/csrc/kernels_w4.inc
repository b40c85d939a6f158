// The 4-wave pipeline's instantiations for GO2PI_W4_TPW tiles per wave (one
// translation unit each: kernels_w4_t{2,4,8}.hip, compiled in parallel) and their
// host launchers. Per program: the head width (1 or 2 tiles; 8 tiles per wave:
// 1), the lean body (PL: w4_plain_body, program.hpp w4_plain) or the general one,
// and layer 0's k-chunk count mod 4 (C0M, program.hpp w4_c0m).
#include "fused_impl.hpp"

namespace go2pi {
namespace {

constexpr int TPW = GO2PI_W4_TPW;

template <int HT, bool PL, int C0M, int RNN, int ACTC = -1, int NHC = 0>
struct Shape {};

// (HT, PL, C0M, RNN) of program p: head tiles, lean body, layer-0 chunks mod 4,
// recurrent cell (0 none / GRU, 1 LSTM)
template <class F>
int with_shape(const DevProgram &p, F &&f) {
  constexpr int H2 = TPW < 8 ? 2 : 1;
  const bool h2 = TPW < 8 && p.head_fuse == 2, c3 = p.w4_c0m == 3, pl = p.w4_plain != 0;
  const bool lstm = p.has_gru && p.gru.cell == 1;
  auto rest = [&]<int HT>(std::integral_constant<int, HT>) {
    if (pl && p.w4_actc == 1 && p.w4_nhc == 3)
      return c3 ? f(Shape<HT, true, 3, 0, 1, 3>{}) : f(Shape<HT, true, 0, 0, 1, 3>{});
    if (pl && p.w4_actc == 1) return c3 ? f(Shape<HT, true, 3, 0, 1>{}) : f(Shape<HT, true, 0, 0, 1>{});
    if (pl) return c3 ? f(Shape<HT, true, 3, 0>{}) : f(Shape<HT, true, 0, 0>{});
    // (a recurrent policy's layer 0 is H wide: C0M = 0)
    if (lstm) return p.w4_nhc == 3 ? f(Shape<HT, false, 0, 1, 1, 3>{}) : f(Shape<HT, false, 0, 1>{});
    // the general body with the lean body's compile-time Elu and layer count (GRU policies)
    if (p.w4_actc == 1 && p.w4_nhc == 3) return c3 ? f(Shape<HT, false, 3, 0, 1, 3>{}) : f(Shape<HT, false, 0, 0, 1, 3>{});
    return c3 ? f(Shape<HT, false, 3, 0>{}) : f(Shape<HT, false, 0, 0>{});
  };
  return h2 ? rest(std::integral_constant<int, H2>{}) : rest(std::integral_constant<int, 1>{});
}

template <int HT, bool PL, int C0M, int RNN, int ACTC, int NHC>
const void *batched_kernel() {
  if constexpr (PL) return reinterpret_cast<const void *>(&policy_mlp_kernel<TPW, HT, C0M, ACTC, NHC>);
  else return reinterpret_cast<const void *>(&policy_fused_kernel<4, TPW, HT, C0M, RNN, ACTC, NHC>);
}

// The lean recurrent tick's instantiation for program p (DevProgram::w4_gru_lean), or
// null: the GRU tick (policy_gru_kernel) or the LSTM one (policy_lstm_kernel, r06), hidden
// tiles per wave GT = H / 64 (2 or 4), the hidden rows no wider than the dense ones.
// gt (optional): the instantiation's GT.
template <int HT>
const void *gru_lean_kernel(const DevProgram &p, int *gt = nullptr) {
  if (!p.w4_gru_lean) return nullptr;
  const bool lstm = p.gru.cell == 1;
  if (gt) *gt = p.gru.H == 128 ? 2 : 4;
  if (p.gru.H == 128)
    return lstm ? reinterpret_cast<const void *>(&policy_lstm_kernel<TPW, HT, 2>)
                : reinterpret_cast<const void *>(&policy_gru_kernel<TPW, HT, 2>);
  if constexpr (TPW >= 4) {
    if (p.gru.H == 256)
      return lstm ? reinterpret_cast<const void *>(&policy_lstm_kernel<TPW, HT, 4>)
                  : reinterpret_cast<const void *>(&policy_gru_kernel<TPW, HT, 4>);
  }
  return nullptr;
}

}  // namespace

template <>
int w4_configure<TPW>(const DevProgram &p) {
  return with_shape(p, [&]<int HT, bool PL, int C0M, int RNN, int ACTC, int NHC>(Shape<HT, PL, C0M, RNN, ACTC, NHC>) {
    hipError_t e = hipFuncSetAttribute(batched_kernel<HT, PL, C0M, RNN, ACTC, NHC>(), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)fused_lds_bytes(p, 4));
    if (e != hipSuccess) return (int)e;
    if constexpr (PL) {  // the lean kernel's looped form (w4_launch)
      e = hipFuncSetAttribute(reinterpret_cast<const void *>(&policy_mlp_seq_kernel<TPW, HT, C0M, ACTC, NHC>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)fused_lds_bytes(p, 4));
      if (e != hipSuccess) return (int)e;
    }
    if constexpr (!PL && C0M == 0 && ACTC == 1 && NHC == 3) {  // (RNN: the GRU or the LSTM tick)
      if (const void *k = gru_lean_kernel<HT>(p)) {
        e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fused_lds_bytes(p, 4));
        if (e != hipSuccess) return (int)e;
      }
    }
    const size_t ctl = fused_ctl_lds_bytes(p, 4);
    if (ctl > 160 * 1024) return 0;  // controller tick unavailable for this width (launch fails loudly)
    if constexpr (PL && ACTC == 1 && NHC == 3) {
      e = hipFuncSetAttribute(reinterpret_cast<const void *>(&policy_mlp_ctl_kernel<TPW, HT, C0M>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)ctl);
      if (e != hipSuccess) return (int)e;
    }
    return (int)hipFuncSetAttribute(reinterpret_cast<const void *>(&policy_fused_ctl_kernel<4, TPW, HT, C0M, RNN>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)ctl);
  });
}

template <>
int w4_launch<TPW>(const DevProgram &p, const DevProgram *p_dev, const float *obs, float *act, float *hidden,
                   int batch, int steps, void *stream) {
  const dim3 grid((batch + GO2PI_TILE_ROWS - 1) / GO2PI_TILE_ROWS);
  const size_t lds = fused_lds_bytes(p, 4);
  return with_shape(p, [&]<int HT, bool PL, int C0M, int RNN, int ACTC, int NHC>(Shape<HT, PL, C0M, RNN, ACTC, NHC>) {
    if constexpr (PL) {
      // dims bit 31: the launch bumps the yield counter (the one-tick form reads it here
      // instead of the grid size)
      const unsigned dims = (unsigned)p.in_dim | (unsigned)p.c0 << 12 | (unsigned)(p.nl - 1) << 20 |
                            (grid.x > GO2PI_YIELD_MIN_GRID ? 1u << 31 : 0u);
      // one tick of a policy with an identity head (every exported one): the one-tick
      // form; a device-side sequence or a head with an activation: the looped form
      if (steps == 1 && p.head_act == 0)
        hipLaunchKernelGGL((policy_mlp_kernel<TPW, HT, C0M, ACTC, NHC>), grid, dim3(256), lds,
                           reinterpret_cast<hipStream_t>(stream), obs, act, p.l0_w, p.bpack, p_dev, batch, steps, dims,
                           p.yield);
      else
        hipLaunchKernelGGL((policy_mlp_seq_kernel<TPW, HT, C0M, ACTC, NHC>), grid, dim3(256), lds,
                           reinterpret_cast<hipStream_t>(stream), obs, act, p.l0_w, p.bpack, p_dev, batch, steps, dims,
                           p.yield);
    } else {
      if constexpr (C0M == 0 && ACTC == 1 && NHC == 3) {
        if (const void *k = gru_lean_kernel<HT>(p); k && batch < (1 << 20)) {  // the lean GRU / LSTM tick (w4_gru_body)
          const unsigned shape = (unsigned)batch | (unsigned)p.in_dim << 20;
          const float *gw = p.gru.w, *l0 = p.l0_w, *bp = p.bpack, *bzr = p.gru.bzr, *bh = p.gru.bh;
          unsigned *y = p.yield;
          int st = steps;
          void *args[] = {&obs, &act, &hidden, &gw, &l0, &bp, const_cast<unsigned *>(&shape), &bzr, &bh,
                          const_cast<const DevProgram **>(&p_dev), &st, &y};
          return (int)hipLaunchKernel(k, grid, dim3(256), args, lds, reinterpret_cast<hipStream_t>(stream));
        }
      }
      hipLaunchKernelGGL((policy_fused_kernel<4, TPW, HT, C0M, RNN, ACTC, NHC>), grid, dim3(256), lds,
                         reinterpret_cast<hipStream_t>(stream), p_dev, obs, act, hidden, batch, steps);
    }
    return (int)hipGetLastError();
  });
}

// What w4_launch runs for one tick (steps = 1) of fewer than 2^20 rows, from the Shape it
// launches: the same branches, a name where it has a launch.
template <>
int w4_name<TPW>(const DevProgram &p, char *buf, size_t cap) {
  return with_shape(p, [&]<int HT, bool PL, int C0M, int RNN, int ACTC, int NHC>(Shape<HT, PL, C0M, RNN, ACTC, NHC>) {
    if constexpr (PL) {
      // <tiles per wave, head tiles, layer-0 chunks mod 4, act, hidden layers, waves per workgroup (4)>
      return std::snprintf(buf, cap, "%s<%d, %d, %d, %d, %d, 4>",
                           p.head_act == 0 ? "policy_mlp_kernel" : "policy_mlp_seq_kernel", TPW, HT, C0M, ACTC, NHC);
    } else {
      if constexpr (C0M == 0 && ACTC == 1 && NHC == 3) {
        int gt = 0;
        if (gru_lean_kernel<HT>(p, &gt))  // <tiles per wave, head tiles, hidden tiles per wave>
          return std::snprintf(buf, cap, "%s<%d, %d, %d>", p.gru.cell == 1 ? "policy_lstm_kernel" : "policy_gru_kernel",
                               TPW, HT, gt);
      }
      return std::snprintf(buf, cap, "policy_fused_kernel<4, %d, %d, %d, %d, %d, %d>", TPW, HT, C0M, RNN, ACTC, NHC);
    }
  });
}

template <>
int w4_launch_ctl<TPW>(const DevProgram &p, const DevProgram *p_dev, const DevCtl &ctl, float *hidden, int batch,
                       void *stream) {
  const dim3 grid((batch + GO2PI_TILE_ROWS - 1) / GO2PI_TILE_ROWS);
  const size_t lds = fused_ctl_lds_bytes(p, 4);
  return with_shape(p, [&]<int HT, bool PL, int C0M, int RNN, int ACTC, int NHC>(Shape<HT, PL, C0M, RNN, ACTC, NHC>) {
    if constexpr (PL && ACTC == 1 && NHC == 3) {
      // the lean controller tick (w4_ctl_body); p.ctl_general (GO2PI_CTL_GENERAL=1 at create): the general body
      if (!p.ctl_general && batch < (1 << 20) && p.in_dim < (1 << 12)) {
        const unsigned shape = (unsigned)batch | (unsigned)p.in_dim << 20;
        hipLaunchKernelGGL((policy_mlp_ctl_kernel<TPW, HT, C0M>), grid, dim3(256), lds,
                           reinterpret_cast<hipStream_t>(stream), ctl.state, ctl.joy, ctl.obs, ctl.action, ctl.prm,
                           p.l0_w, shape, p.bpack, p_dev, p.yield, p.c0, ctl);
        return (int)hipGetLastError();
      }
    }
    hipLaunchKernelGGL((policy_fused_ctl_kernel<4, TPW, HT, C0M, RNN>), grid, dim3(256), lds,
                       reinterpret_cast<hipStream_t>(stream), p_dev, ctl, hidden, batch);
    return (int)hipGetLastError();
  });
}

}  // namespace go2pi
