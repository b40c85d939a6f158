// The 4-wave pipeline's residual instantiations (policy_mlp_res_kernel, w4ln_impl.hpp RES) for
// GO2PI_W4_TPW tiles per wave (one translation unit each: kernels_w4res_t{2,4,8}.hip, units of
// their own so that every other unit compiles as it did) and their host launchers. Per
// program: the head width (1 or 2 tiles; 8 tiles per wave: 1). The LDS layout, the pack and
// the arguments are the LN pipeline's (w4ln_layout.hpp, program.hpp w4ln_tpw).
#include "w4ln_impl.hpp"

namespace go2pi {
namespace {

constexpr int TPW = GO2PI_W4_TPW;

template <class F>
int with_head(const DevProgram &p, F &&f) {
  if constexpr (TPW < 8) {
    if (p.L[p.nl - 1].N_pad == 32) return f(std::integral_constant<int, 2>{});
  }
  return f(std::integral_constant<int, 1>{});
}

}  // namespace

template <>
int w4res_configure<TPW>(const DevProgram &p) {
  return with_head(p, [&](auto ht) {
    return (int)hipFuncSetAttribute(reinterpret_cast<const void *>(&policy_mlp_res_kernel<TPW, decltype(ht)::value>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)w4ln_lds_bytes(p));
  });
}

template <>
int w4res_launch<TPW>(const DevProgram &p, const DevProgram *p_dev, const float *obs, float *act, int batch, int steps,
                      void *stream) {
  const dim3 grid((batch + GO2PI_TILE_ROWS - 1) / GO2PI_TILE_ROWS);
  const size_t lds = w4ln_lds_bytes(p);
  // (the planner selects the kernel only for in_dim < 4096 and a layer 0 of a multiple of 4 chunks)
  const unsigned dims = (unsigned)p.in_dim | (unsigned)p.c0 << 12 | (unsigned)(p.nl - 1) << 20;
  return with_head(p, [&](auto ht) {
    hipLaunchKernelGGL((policy_mlp_res_kernel<TPW, decltype(ht)::value>), grid, dim3(256), lds,
                       reinterpret_cast<hipStream_t>(stream), obs, act, p.l0_w, p.bpack, p_dev, batch, steps, dims,
                       p.yield);
    return (int)hipGetLastError();
  });
}

template <>
int w4res_name<TPW>(const DevProgram &p, char *buf, size_t cap) {
  return with_head(p, [&](auto ht) {  // <tiles per wave, head tiles>
    return std::snprintf(buf, cap, "policy_mlp_res_kernel<%d, %d>", TPW, (int)decltype(ht)::value);
  });
}

}  // namespace go2pi
