// The dynamic-LDS layout of every small-batch and resident kernel, one struct and one
// function each: the kernel takes its struct once and steps through the regions in the
// struct's order by their sizes (policy_wide_kernel, whose layout is a compile-time
// constant, by their offsets; DESIGN §4.2f says why the others step), its launcher sizes
// the allocation as sizeof(float) * total, and tests/test_cpu_lds_layout.py checks every
// layout through tests/cpp/plan_probe.cpp without a GPU. Plain C++ (no HIP header, no
// host / device macro): constexpr functions, callable from device code as they stand.
// All offsets and sizes in floats. A region starts where the previous one ends (after),
// so every size term is written once; a region in front of one that holds double or
// float4 values, or is the target of a direct-to-LDS load, is padded to 16 bytes (pad4)
// where its size is not a multiple of that by construction. A region a form does not
// have keeps its place with size 0. The batched pipeline's layout (fused_lds_bytes,
// fused_impl.hpp) is not here.
#pragma once

namespace go2pi {

namespace lds {
// (program.hpp asserts these equal its GO2PI_* constants, the kernels their wave counts)
constexpr int MAXB = 8;    // GO2PI_SMALL_MAXB: rows of a small-batch request
constexpr int WAVES = 8;   // waves that split a layer's k-chunks (GEMV_WAVES, LAT_WAVES, RES_WAVES)
constexpr int TILE = 16;   // GO2PI_TILE_ROWS
constexpr int CTL_STATE = 36, CTL_JOY = 5, CTL_DOF = 12;  // GO2PI_CTL_*_DIM, GO2PI_CTL_DOF
constexpr int CTL_RAW = CTL_STATE + CTL_JOY + CTL_DOF;    // GO2PI_CTL_RAW

struct Span {
  int off, size;
  constexpr int end() const { return off + size; }
};
constexpr Span after(Span prev, int size) { return Span{prev.end(), size}; }
constexpr int pad4(int x) { return (x + 3) / 4 * 4; }
constexpr int c64(int x) { return (x + 63) & ~63; }  // room for a direct-to-LDS copy (glds_copy: whole waves)
}  // namespace lds

// The LDS image of one tile's controller inputs (ctl_fn.hpp CtlLds), rows r < R.
// obs false: the caller places the previous observation rows (the batched kernel, in its
// layer-0 output buffer: at a 16-step history they are 50 KB per tile).
struct CtlImage {
  lds::Span q0;    // 12 doubles, copied by one direct-to-LDS instruction (64 lanes x 4 B)
  lds::Span st;    // [R][36] raw state rows
  lds::Span jy;    // [R][5] joystick rows
  lds::Span act;   // [R][12] previous action rows
  lds::Span obs;   // [R][in_dim] previous observation rows
  lds::Span nanf;  // [16] per-row NaN flags
  int total;
};
constexpr CtlImage ctl_image(int R, int in_dim, bool obs = true) {
  CtlImage L{};
  L.q0 = {0, 64};
  L.st = lds::after(L.q0, lds::c64(R * lds::CTL_STATE));
  L.jy = lds::after(L.st, lds::c64(R * lds::CTL_JOY));
  L.act = lds::after(L.jy, lds::c64(R * lds::CTL_DOF));
  L.obs = lds::after(L.act, obs ? lds::c64(R * in_dim) : 0);
  L.nanf = lds::after(L.obs, lds::TILE);
  L.total = L.nanf.end();
  return L;
}
constexpr int ctl_lds_floats(int R, int in_dim, bool obs = true) { return ctl_image(R, in_dim, obs).total; }

// gemv_layer_kernel (kernels.hip), one layer of K_pad inputs
struct GemvLds {
  lds::Span xs;    // [8][K_pad] the layer's input rows
  lds::Span part;  // [waves][8][16] partial sums
  int total;
};
constexpr GemvLds gemv_lds(int K_pad) {
  GemvLds L{};
  L.xs = {0, lds::MAXB * K_pad};
  L.part = lds::after(L.xs, lds::WAVES * lds::MAXB * 16);
  L.total = L.part.end();
  return L;
}

// The controller form's regions of latency_body (LatencyLds ctl)
struct LatencyCtlLds {
  lds::Span okeep;  // [8][in_dim] the new raw observation rows
  lds::Span image;  // the LDS image of the inputs
  lds::Span slack;  // reserved since the form was written, never addressed
  int total;
};
constexpr LatencyCtlLds latency_ctl_lds(int in_dim) {
  LatencyCtlLds L{};
  L.okeep = {0, lds::MAXB * in_dim};
  L.image = lds::after(L.okeep, ctl_lds_floats(lds::MAXB, in_dim));
  L.slack = lds::after(L.image, lds::MAXB);
  L.total = L.slack.end();
  return L;
}

// latency_body (kernels.hip: policy_latency_kernel and its controller / general forms).
// ctl: the floats of the controller form's LatencyCtlLds, 0 for act().
struct LatencyLds {
  lds::Span xs;    // [8][lds_stride] layer input
  lds::Span part;  // [waves][8][16] partial sums
  lds::Span flag;  // [0] the abort flag
  lds::Span ctl;   // the controller form's regions
  int total;
};
constexpr LatencyLds latency_lds(int lds_stride, int ctl) {
  LatencyLds L{};
  L.xs = {0, lds::MAXB * lds_stride};
  L.part = lds::after(L.xs, lds::WAVES * lds::MAXB * 16);
  L.flag = lds::after(L.part, 4);
  L.ctl = lds::after(L.flag, ctl);
  L.total = L.ctl.end();
  return L;
}

// policy_resident1_kernel (resident.hip)
struct R1Lds {
  lds::Span x0;      // [8][S] layer 0's input rows (zero past in_dim)
  lds::Span xa, xb;  // [8][S] each: hidden layers' rows (ping-pong)
  lds::Span st;      // [0] leave, [1] epoch, [2] batch, [3] word
  lds::Span obsv;    // [8][in_dim] the request's observation
  lds::Span image;   // ctl: the LDS image of the tick's inputs
  lds::Span craw;    // ctl: [8][GO2PI_CTL_RAW + in_dim] request rows
  int total;
};
constexpr R1Lds r1_lds(int S, int in_dim, bool ctl) {
  R1Lds L{};
  L.x0 = {0, lds::MAXB * S};
  L.xa = lds::after(L.x0, lds::MAXB * S);
  L.xb = lds::after(L.xa, lds::MAXB * S);
  L.st = lds::after(L.xb, 4);
  L.obsv = lds::after(L.st, lds::pad4(lds::MAXB * in_dim));
  L.image = lds::after(L.obsv, ctl ? ctl_lds_floats(lds::MAXB, in_dim) : 0);
  L.craw = lds::after(L.image, ctl ? lds::MAXB * (lds::CTL_RAW + in_dim) : 0);
  L.total = L.craw.end();
  return L;
}

// policy_act1_kernel keeps layer 0's and the head's weights in LDS, not registers
// (re-read per request): in the controller form, where they spilled beside the assembly's
// registers, and for a LayerNormalization program of four 128-wide layers, where the LN
// pass's registers beside all the weights spilled 7 to 33 registers to scratch.
constexpr bool act1_weights_in_lds(bool ctl, bool ln, int h, int nl) { return ctl || (ln && h == 128 && nl == 4); }

// policy_act1_kernel<NL, H, F0, ..., CTL, LN> (resident.hip)
struct Act1Lds {
  int h, nl, f0;     // the template arguments it was made for
  lds::Span x0;      // [8][S] layer 0's input rows (zero past in_dim)
  lds::Span xa, xb;  // [8][S] each: wide layers' rows (ping-pong)
  lds::Span st;      // [0] leave, [1] epoch, [2] batch, [3] word
  lds::Span image;   // ctl: the LDS image of the tick's inputs (q0 once, the request's rows per request)
  lds::Span w0l;     // weights in LDS: layer 0's, lane-major [f][j][compute lane] float4 (a wave's read: 1 KiB contiguous)
  lds::Span wol;     // weights in LDS: the head's, lane-major [f][head lane] float4, 256 lanes
  lds::Span obsn;    // ctl: [8][in_dim] the request's new observation rows
  int total;
};
constexpr Act1Lds act1_lds(int S, int in_dim, int h, int nl, int f0, bool ctl, bool ln) {
  const bool wl = act1_weights_in_lds(ctl, ln, h, nl);
  Act1Lds L{};
  L.h = h, L.nl = nl, L.f0 = f0;
  L.x0 = {0, lds::MAXB * S};
  L.xa = lds::after(L.x0, lds::MAXB * S);
  L.xb = lds::after(L.xa, lds::MAXB * S);
  L.st = lds::after(L.xb, 4);
  L.image = lds::after(L.st, ctl ? ctl_lds_floats(lds::MAXB, in_dim) : 0);
  L.w0l = lds::after(L.image, wl ? f0 * h * 16 * 4 : 0);  // f0 float4s for each of an output's 16 k-slice lanes
  L.wol = lds::after(L.w0l, wl ? h / 64 * 256 * 4 : 0);
  L.obsn = lds::after(L.wol, ctl ? lds::MAXB * in_dim : 0);
  L.total = L.obsn.end();
  return L;
}

// policy_resident_kernel's local layer 0: every workgroup computes all of layer 0 itself,
// its 512 threads as ks k-slices of N_pad outputs, nf fragment floats (nf / 4 chunks) per
// thread; the launcher runs it where nf is 8, 12 or 16 (a slice's chunks past layer 0's
// own are zero fragments on zero columns).
struct Local0 {
  int ks, nf;
};
constexpr Local0 local0_geometry(int K_pad, int N_pad) {
  constexpr int NT = lds::WAVES * 64;
  const int ks = (N_pad > 0 && NT % N_pad == 0) ? NT / N_pad : 0;
  return Local0{ks, ks > 0 ? 4 * (((K_pad >> 4) + ks - 1) / ks) : 0};
}
// floats per prologued input row: nf / 4 chunks for each of the ks slices (>= K_pad)
constexpr int local0_row(int nf, int ks) { return (nf / 4) * ks * 16; }

// The recurrent cell's regions of policy_resident_kernel<0, false, RNN> (MultiLds cell)
struct CellLds {
  lds::Span hx;     // [8][I_pad + H] the cell's input rows [x | h]
  lds::Span hpart;  // [waves][4][8][16] partial sums (z, r, n_x, n_h)
  lds::Span le;     // [8] row epochs
  lds::Span lb;     // [8] the granule buffer holding each row's h
  lds::Span hown;   // [8][16] this workgroup's units' latest h'
  lds::Span cown;   // [8][16] LSTM: its units' cell state (laid out for a GRU too)
  // the cell's outputs of the request in flight, copied to hown / cown only once this
  // workgroup has finished the request: a request abandoned mid-layers (a sweep met a
  // LEAVE tag) then leaves the committed state, which the leave path writes back, as it was
  lds::Span hst, cst;  // [8][16] each
  int total;
};
constexpr CellLds cell_lds(int I_pad, int H) {
  const int row = lds::MAXB * 16;
  CellLds L{};
  L.hx = {0, lds::MAXB * (I_pad + H)};
  L.hpart = lds::after(L.hx, lds::WAVES * 4 * row);
  L.le = lds::after(L.hpart, lds::MAXB);
  L.lb = lds::after(L.le, lds::MAXB);
  L.hown = lds::after(L.lb, row);
  L.cown = lds::after(L.hown, row);
  L.hst = lds::after(L.cown, row);
  L.cst = lds::after(L.hst, row);
  L.total = L.cst.end();
  return L;
}

// policy_resident_kernel<NF, CTL, RNN, ..> (resident.hip). nf: NF (0: layer 0 tiled);
// cell: the floats of the recurrent form's CellLds, 0 without a cell (the controller's
// and the cell's regions start at the same place: the forms are exclusive).
struct MultiLds {
  int nf;           // the template argument it was made for
  lds::Span xs;     // [8][lds_stride] layer input
  lds::Span part;   // [waves][8][16] partial sums
  lds::Span st;     // [0] leave, [1] epoch, [2] batch
  lds::Span obsv;   // [8][in_dim] the request's observation
  lds::Span x0;     // [8][local0_row] local layer 0's prologued input rows (layer 0 tiled: [8][K_pad], unused)
  lds::Span p0;     // [ks][8][N_pad] local layer 0's partials where ks > 1 slices
  lds::Span image;  // ctl: the LDS image of the tick's inputs
  lds::Span craw;   // ctl: [8][GO2PI_CTL_RAW + in_dim] request rows
  lds::Span cell;   // rnn: the cell's regions (CellLds)
  int total;
};
constexpr MultiLds multi_lds(int lds_stride, int in_dim, int K_pad, int N_pad, int nf, bool ctl, int cell) {
  // (in the kernel's own arithmetic, for a padded layer width N_pad >= 16: the slices of a
  // local layer 0, which has nf > 0 only where N_pad divides 512, and the slices past one)
  constexpr int NT = lds::WAVES * 64;
  const int x0row = nf > 0 ? local0_row(nf, NT / N_pad) : K_pad;
  const int ks1 = (NT % N_pad == 0 && N_pad < NT) ? NT / N_pad : 0;
  MultiLds L{};
  L.nf = nf;
  L.xs = {0, lds::MAXB * lds_stride};
  L.part = lds::after(L.xs, lds::WAVES * lds::MAXB * 16);
  L.st = lds::after(L.part, 4);
  L.obsv = lds::after(L.st, lds::MAXB * in_dim);
  L.x0 = lds::after(L.obsv, lds::MAXB * x0row);
  L.p0 = lds::after(L.x0, lds::pad4(ks1 * lds::MAXB * N_pad));
  L.image = lds::after(L.p0, ctl ? ctl_lds_floats(lds::MAXB, in_dim) : 0);
  L.craw = lds::after(L.image, ctl ? lds::MAXB * (lds::CTL_RAW + in_dim) : 0);
  L.cell = lds::after(L.craw, cell);
  L.total = L.cell.end();
  return L;
}

// policy_wide_kernel<NL, CW, F0, PRO> (resident_wide.hip): H = 64 CW
struct WideLds {
  lds::Span x0;  // [8][4 F0] the observation rows (prologued, zero-padded)
  lds::Span h0;  // [8][H] layer 0's outputs
  lds::Span hh;  // [8][H] a sliced layer's outputs of every workgroup (swept)
  lds::Span ho;  // [8][16] this workgroup's outputs of a sliced layer
  lds::Span pp;  // [8][16 columns][16 head outputs] its head products
  lds::Span st;  // [0] leave [1] epoch [2] batch [3] fail
  int total;
};
constexpr WideLds wide_lds(int cw, int f0) {
  WideLds L{};
  L.x0 = {0, lds::MAXB * 4 * f0};
  L.h0 = lds::after(L.x0, lds::MAXB * 64 * cw);
  L.hh = lds::after(L.h0, lds::MAXB * 64 * cw);
  L.ho = lds::after(L.hh, lds::MAXB * 16);
  L.pp = lds::after(L.ho, lds::MAXB * 256);
  L.st = lds::after(L.pp, 4);
  L.total = L.st.end();
  return L;
}

}  // namespace go2pi
