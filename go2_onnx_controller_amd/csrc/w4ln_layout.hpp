// The dynamic-LDS layout of the 4-wave LayerNormalization pipeline (w4ln_impl.hpp
// policy_mlp_ln_kernel<TPW, HT>), in the manner of lds_layout.hpp: one struct and one
// constexpr function, read by the kernel (the offsets), by its launcher (the size of the
// allocation) and by the planner (plan.cpp: a policy whose layout passes 160 KiB keeps the
// general body). Plain C++. Offsets and sizes in floats.
#pragma once

#include <cstddef>

#include "program.hpp"

namespace go2pi {

constexpr int W4LN_WAVES = 4;
constexpr int W4LN_MAX_LDS_BYTES = 160 * 1024;

struct W4LnLds {
  lds::Span xa, xb;    // [16][64 tpw + 4] the two activation buffers (layer l reads one, writes the other)
  lds::Span scratch;   // [ht][4 waves][64 lanes] float4: the head's partial sums
  lds::Span flags;     // [64] the per-wave layer hand-off words
  lds::Span sum, var;  // [16 rows][4 waves] each: the waves' partial row statistics (mean pass, variance pass)
  lds::Span pack;      // [3][nh][64 tpw] biases | Scale | B of the nh hidden layers, one direct-to-LDS stream
  int stride;          // floats per activation row
  int total;
};

// tpw: tiles per wave (2 / 4 / 8), ht: head tiles (1 / 2), nh: hidden layers. The pack is
// the last region, so every other offset is a constant of the instantiation.
constexpr W4LnLds w4ln_lds(int tpw, int ht, int nh) {
  W4LnLds L{};
  L.stride = 64 * tpw + 4;  // +16 B per row: rows start on different LDS banks (= DevProgram::lds_stride)
  L.xa = {0, lds::TILE * L.stride};
  L.xb = lds::after(L.xa, lds::TILE * L.stride);
  L.scratch = lds::after(L.xb, ht * W4LN_WAVES * 64 * 4);
  L.flags = lds::after(L.scratch, 64);
  L.sum = lds::after(L.flags, lds::TILE * W4LN_WAVES);
  L.var = lds::after(L.sum, lds::TILE * W4LN_WAVES);
  L.pack = lds::after(L.var, 3 * nh * 64 * tpw);  // (a multiple of 64: glds_copy's whole waves)
  L.total = L.pack.end();
  return L;
}

constexpr bool w4ln_lds_ok(int tpw, int ht, int nh) {
  const W4LnLds L = w4ln_lds(tpw, ht, nh);
  // in order, none overlapping, and every region that holds float4 values or takes a
  // direct-to-LDS load starts on 16 bytes
  return L.xa.off == 0 && L.xb.off == L.xa.end() && L.scratch.off == L.xb.end() && L.flags.off == L.scratch.end() &&
         L.sum.off == L.flags.end() && L.var.off == L.sum.end() && L.pack.off == L.var.end() &&
         L.xa.size > 0 && L.xb.size > 0 && L.scratch.size > 0 && L.sum.size > 0 && L.var.size > 0 &&
         L.stride % 4 == 0 && L.xb.off % 4 == 0 && L.scratch.off % 4 == 0 && L.sum.off % 4 == 0 &&
         L.var.off % 4 == 0 && L.pack.off % 4 == 0;
}
static_assert(w4ln_lds_ok(2, 1, 1) && w4ln_lds_ok(2, 2, 7) && w4ln_lds_ok(4, 1, 3) && w4ln_lds_ok(4, 2, 7) &&
                  w4ln_lds_ok(8, 1, 7),
              "regions of the LN pipeline's LDS overlap or are misaligned");
// the workload's shape (48 -> 512^3 -> 12) fits with room to spare
static_assert(sizeof(float) * w4ln_lds(8, 1, 3).total <= W4LN_MAX_LDS_BYTES, "ln_512_pre must fit");

// bytes of dynamic LDS of an LN pipeline program's launch (program.hpp w4ln_tpw)
inline size_t w4ln_lds_bytes(const DevProgram &p) {
  return sizeof(float) * (size_t)w4ln_lds(p.w4ln_tpw, p.L[p.nl - 1].N_pad / 16, p.nl - 1).total;
}

// The host side, one translation unit per tiles per wave (kernels_w4ln_t{2,4,8}.hip).
template <int TPW>
int w4ln_configure(const DevProgram &p);
template <int TPW>
int w4ln_launch(const DevProgram &p, const DevProgram *p_dev, const float *obs, float *act, int batch, int steps,
                void *stream);
template <int TPW>
int w4ln_name(const DevProgram &p, char *buf, size_t cap);  // w4ln_launch's kernel (batched_kernel_name)

// The pipeline's residual kernel (policy_mlp_res_kernel; a program with w4ln_tpw != 0 and
// residual connections, GO2PI_RESIDUAL_BATCHED): the layout, the pack and the launch arguments
// above; one translation unit per tiles per wave (kernels_w4res_t{2,4,8}.hip).
template <int TPW>
int w4res_configure(const DevProgram &p);
template <int TPW>
int w4res_launch(const DevProgram &p, const DevProgram *p_dev, const float *obs, float *act, int batch, int steps,
                 void *stream);
template <int TPW>
int w4res_name(const DevProgram &p, char *buf, size_t cap);

}  // namespace go2pi
