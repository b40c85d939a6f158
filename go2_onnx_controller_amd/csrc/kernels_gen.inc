// The generic batched body's instantiations for GO2PI_GEN_NW waves per workgroup
// (one translation unit each: kernels_gen_w{4,8,16}.hip, compiled in parallel)
// and their host launchers: policies the 4-wave pipeline does not cover
// (non-uniform widths, narrow recurrent cells), with or without the controller tick.
// RNN: the recurrent cell (0 none / GRU, 1 LSTM), from the program.
#include "fused_impl.hpp"

namespace go2pi {
namespace {

constexpr int NW = GO2PI_GEN_NW;

template <class F>
int with_rnn(const DevProgram &p, F &&f) {
  return (p.has_gru && p.gru.cell == 1) ? f(std::integral_constant<int, 1>{}) : f(std::integral_constant<int, 0>{});
}

}  // namespace

template <>
int gen_configure<NW>(const DevProgram &p) {
  return with_rnn(p, [&]<int RNN>(std::integral_constant<int, RNN>) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&policy_fused_kernel<NW, 0, 0, 0, RNN>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)fused_lds_bytes(p, NW));
    if (e != hipSuccess) return (int)e;
    const size_t ctl = fused_ctl_lds_bytes(p, NW);
    if (ctl > 160 * 1024) return 0;  // controller tick unavailable for this width (launch fails loudly)
    return (int)hipFuncSetAttribute(reinterpret_cast<const void *>(&policy_fused_ctl_kernel<NW, 0, 0, 0, RNN>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)ctl);
  });
}

template <>
int gen_launch<NW>(const DevProgram &p, const DevProgram *p_dev, const float *obs, float *act, float *hidden,
                   int batch, int steps, void *stream) {
  const dim3 grid((batch + GO2PI_TILE_ROWS - 1) / GO2PI_TILE_ROWS);
  const size_t lds = fused_lds_bytes(p, NW);
  return with_rnn(p, [&]<int RNN>(std::integral_constant<int, RNN>) {
    hipLaunchKernelGGL((policy_fused_kernel<NW, 0, 0, 0, RNN>), grid, dim3(NW * 64), lds,
                       reinterpret_cast<hipStream_t>(stream), p_dev, obs, act, hidden, batch, steps);
    return (int)hipGetLastError();
  });
}

template <>
int gen_name<NW>(const DevProgram &p, char *buf, size_t cap) {  // (what gen_launch runs)
  return with_rnn(p, [&]<int RNN>(std::integral_constant<int, RNN>) {
    return std::snprintf(buf, cap, "policy_fused_kernel<%d, 0, 0, 0, %d, -1, 0>", NW, RNN);
  });
}

template <>
int gen_launch_ctl<NW>(const DevProgram &p, const DevProgram *p_dev, const DevCtl &ctl, float *hidden, int batch,
                       void *stream) {
  const dim3 grid((batch + GO2PI_TILE_ROWS - 1) / GO2PI_TILE_ROWS);
  const size_t lds = fused_ctl_lds_bytes(p, NW);
  return with_rnn(p, [&]<int RNN>(std::integral_constant<int, RNN>) {
    hipLaunchKernelGGL((policy_fused_ctl_kernel<NW, 0, 0, 0, RNN>), grid, dim3(NW * 64), lds,
                       reinterpret_cast<hipStream_t>(stream), p_dev, ctl, hidden, batch);
    return (int)hipGetLastError();
  });
}

}  // namespace go2pi
