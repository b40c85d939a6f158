// The generic batched body with a carried tile (fused_impl.hpp fused_body RES,
// policy_fused_res_kernel): policies with residual connections (DevProgram::res). A
// translation unit of its own, so kernels_gen_w{4,8,16}.hip compile to what they were. Only
// the 8-wave instantiation is built (a general-body unit takes minutes to compile); the
// planner refuses an explicit waves = 4 or 16 for such a program (plan.cpp plan_program).
#include "fused_impl.hpp"

namespace go2pi {

namespace {
constexpr int NW = 8;
}

int res_configure(const DevProgram &p) {
  return (int)hipFuncSetAttribute(reinterpret_cast<const void *>(&policy_fused_res_kernel<NW>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)fused_lds_bytes(p, NW));
}

int res_launch(const DevProgram &p, const DevProgram *p_dev, const float *obs, float *act, int batch, int steps,
               void *stream) {
  if (p.has_gru || p.head_fuse) return (int)hipErrorInvalidValue;  // (never planned for such a program)
  const dim3 grid((batch + GO2PI_TILE_ROWS - 1) / GO2PI_TILE_ROWS);
  hipLaunchKernelGGL(policy_fused_res_kernel<NW>, grid, dim3(NW * 64), fused_lds_bytes(p, NW),
                     reinterpret_cast<hipStream_t>(stream), p_dev, obs, act, batch, steps);
  return (int)hipGetLastError();
}

int res_name(const DevProgram &, char *buf, size_t cap) {  // (what res_launch runs)
  return std::snprintf(buf, cap, "policy_fused_res_kernel<%d>", NW);
}

}  // namespace go2pi
