// The engine's planner (plan.hpp): model + options + switches -> the program's scalars, the
// host buffers behind its pointers, and which kernel serves what. No HIP in here.
#include "plan.hpp"
#include "w4ln_layout.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

namespace go2pi {
namespace {

inline int ceil16(int x) { return (x + 15) & ~15; }
inline int ceil64(int x) { return (x + 63) & ~63; }

// K is padded to a multiple of 64 (4 chunks: the kernel's unroll); a hidden layer's
// N to its consumer's K_pad (64), the final layer's N to 16 (one MFMA tile).
// next_k: the consumer's K where it has a skip input (its K_pad = ceil64(N + skip_n) can pass
// ceil64(N): the extra tiles are zero weights and biases, and the consumer's skip columns
// overwrite part of what their store leaves), else 0.
void pack_dense(const Dense &d, bool last, std::vector<float> &w, std::vector<float> &b, int &K_pad, int &N_pad,
                int kq = 64, int next_k = 0) {
  K_pad = kq == 16 ? ceil16(d.K) : ceil64(d.K);
  N_pad = last ? ceil16(d.N) : ceil64(std::max(d.N, next_k));
  const int T = N_pad / 16, C = K_pad / 16;
  w.assign((size_t)T * C * 64 * 4, 0.f);
  for (int t = 0; t < T; ++t)
    for (int c = 0; c < C; ++c)
      for (int lane = 0; lane < 64; ++lane)
        for (int j = 0; j < 4; ++j) {
          const int n = 16 * t + (lane & 15), k = 16 * c + 4 * (lane >> 4) + j;
          w[(((size_t)c * T + t) * 64 + lane) * 4 + j] = (n < d.N && k < d.K) ? d.W[(size_t)n * d.K + k] : 0.f;
        }
  b.assign(N_pad, 0.f);
  std::copy(d.b.begin(), d.b.end(), b.begin());
}

// Recurrent-cell fragments: [Cx + Ch][Ht][gate][lane] float4 over the concatenated
// [x (I_pad) | h (H)] axis; x chunks carry W, h chunks carry R. G = 3 gates (GRU:
// z, r, h) or 4 (LSTM: i, o, f, c), in ONNX row order. The x columns k >= I are zeros; the
// lean recurrent tick's observation staging reads its padding lanes' zeros from them
// (fused_impl.hpp w4_gru_body; tests/test_cpu_plan.py pins this layout).
void pack_gru(const Gru &g, std::vector<float> &w, int &I_pad) {
  I_pad = ceil64(g.I);  // whole 4-chunk groups of x (the pipelined cell's ring runs on them)
  const int H = g.H, Ht = H / 16, Cx = I_pad / 16, Ch = H / 16, Cc = Cx + Ch, G = g.G;
  w.assign((size_t)Ht * Cc * G * 64 * 4, 0.f);
  for (int t = 0; t < Ht; ++t)
    for (int c = 0; c < Cc; ++c)
      for (int gate = 0; gate < G; ++gate)
        for (int lane = 0; lane < 64; ++lane)
          for (int j = 0; j < 4; ++j) {
            const int unit = 16 * t + (lane & 15);
            const int row = gate * H + unit;
            float v = 0.f;
            if (c < Cx) {
              const int k = 16 * c + 4 * (lane >> 4) + j;
              if (k < g.I) v = g.W[(size_t)row * g.I + k];
            } else {
              const int k = 16 * (c - Cx) + 4 * (lane >> 4) + j;
              v = g.R[(size_t)row * H + k];
            }
            w[((((size_t)c * Ht + t) * G + gate) * 64 + lane) * 4 + j] = v;
          }
}

// The pipeline's shape test (w4_eligible below; the LN pipeline, plan_program): the tiles per
// wave (2, 4 or 8) of a policy whose dense layers it serves, else 0. uniform_act = false: the
// hidden layers need not share an activation (the residual pipeline reads each layer's own).
int w4_shape_tpw(const Model &m, bool uniform_act = true) {
  const int nl = (int)m.layers.size();
  if (nl < 2) return 0;
  const int tpw = ceil64(m.layers[0].N) / 64, t_last = ceil16(m.layers[nl - 1].N) / 16;
  if (!(tpw == 2 || tpw == 4 || tpw == 8) || t_last > (tpw == 8 ? 1 : 2)) return 0;
  for (int l = 0; l + 1 < nl; ++l)
    if (ceil64(m.layers[l].N) != 64 * tpw ||
        (uniform_act && (m.layers[l].act != m.layers[0].act || m.layers[l].alpha != m.layers[0].alpha ||
                         m.layers[l].beta != m.layers[0].beta)))
      return 0;
  return tpw;
}

// The 4-wave uniform-MLP pipeline (fused_impl.hpp w4_step) applies to a policy
// whose hidden layers are all 64 * TPW wide (TPW = 2, 4 or 8) with one
// activation, and whose final layer is at most 2 tiles wide (1 at TPW = 8); a GRU
// in front needs H % 64 == 0. It is the default (waves = 0) wherever it applies:
// measured faster than the generic 8-wave body.
// ln: a LayerNormalization on any layer: served by the general batched body and the GEMV
// chain only (no pipeline / lean kernel, latency kernel or resident form); with
// opts.ln_small = 1 a dense one also by the latency kernel and, of the resident forms,
// policy_act1_kernel's act() form or the multi-workgroup kernel.
bool w4_eligible(const Model &m, const go2pi_opts &o, const Switches &sw, bool ln) {
  const int nl = (int)m.layers.size();
  // an observation skip input: the general body and the GEMV chain only
  // ... and a residual connection: the general body's residual instantiation and the chain
  for (const auto &d : m.layers)
    if (!d.skip.empty() || d.res >= 0) return false;
  if (!(o.waves == 0 || o.waves == 4) || nl < 2) return false;
  if (m.has_gru && m.gru.H % 64) return false;
  if (m.has_gru && m.gru.cell == 0 && m.gru.lbr == 0) return false;  // the two-pass cell: generic body only
  if (sw.no_head_fuse || sw.no_w4) return false;  // A/B diagnostics only
  // LayerNormalization: the general body (fused_impl.hpp ln_tile), or, with opts.ln_small's
  // GO2PI_LN_BATCHED bit, the pipeline's LN kernel beside it (plan_program, w4ln_tpw)
  if (ln) return false;
  return w4_shape_tpw(m) != 0;
}

// opts.ln_small as its two bits (GO2PI_LN_SMALL | GO2PI_LN_BATCHED); any value outside 0..3
// reads as 0: the field fills the earlier layout's tail padding, which may hold anything
int ln_bits(const go2pi_opts &o) { return o.ln_small >= 0 && o.ln_small <= 3 ? o.ln_small : 0; }

// no action post-processing (tanh / clip / scale): the head's plain store
bool post_plain(const DevProgram &p) {
  return !p.post_tanh && std::isinf(p.clip_lo) && p.clip_lo < 0 && std::isinf(p.clip_hi) && p.clip_hi > 0 &&
         p.scale == 1.f;
}

}  // namespace

void check_model(const Model &m) {
  if ((int)m.layers.size() > GO2PI_MAX_LAYERS)
    throw ApiError("policy has more than " + std::to_string(GO2PI_MAX_LAYERS) + " dense layers", GO2PI_E_MODEL);
  if (m.has_gru) {
    // lbr = 0 (Keras reset_after=False) runs the generic body's two-pass cell
    // (fused_impl.hpp gru0_cell), one tile group per wave: H <= 256
    if (m.gru.cell == 0 && m.gru.lbr == 0 && m.gru.H > 256)
      throw ApiError("GRU linear_before_reset=0 with hidden size > 256 is not supported", GO2PI_E_MODEL);
    if (m.gru.H % 16) throw ApiError("recurrent hidden size must be a multiple of 16", GO2PI_E_MODEL);
  }
}

void fill_hot_block(DevProgram &p) {
  if (!p.w4_tpw && !p.w4ln_tpw) return;
  const auto &H = p.L[p.nl - 1];
  p.l0_w = p.L[0].w;
  p.head_w = H.w;
  p.head_bias = H.bias;
  p.bpack = p.w4_bpack;
  p.zero_hot = p.zero;
  p.err_hot = p.err;
  p.nbias = p.w4_bias;
  p.head_n = H.N;
  p.c0 = p.L[0].K_pad / 16;
  p.in_dim_hot = p.in_dim;
  p.hid_act = p.L[0].act;
  p.hid_alpha = p.L[0].alpha;
  p.hid_beta = p.L[0].beta;
  p.head_act = H.act;
  p.head_alpha = H.alpha;
  p.head_beta = H.beta;
  p.post_plain = post_plain(p) ? 1 : 0;
  if (p.w4ln_tpw) {
    // the LN pipeline (program.hpp w4ln_tpw): the model's hidden activation (the planner moved
    // a pre-LN layer's to its ln_act), and the pack's floats; bpack is set by build()
    const DevLayer &L0 = p.L[0];
    p.hid_act = L0.ln == 1 ? L0.ln_act : L0.act;
    p.hid_alpha = L0.ln == 1 ? L0.ln_alpha : L0.alpha;
    p.hid_beta = L0.ln == 1 ? L0.ln_beta : L0.beta;
    p.nbias = 3 * (p.nl - 1) * 64 * p.w4ln_tpw;
  }
}

Plan plan_program(const Model &m, const go2pi_opts &o, const Switches &sw) {
  Plan pl;
  HostBuffers &buf = pl.buf;
  // 8 waves per 16-robot workgroup (2 per SIMD) measured fastest with the
  // interleaved schedule (kernels.hip, dense_acc note): 104K vs 106K cycles at 16
  pl.waves = (o.waves == 4 || o.waves == 16) ? o.waves : 8;
  pl.small_batch = o.small_batch == 0 ? GO2PI_SMALL_MAXB : std::min<int>(o.small_batch, GO2PI_SMALL_MAXB);

  DevProgram &p = pl.prog;
  std::memset(&p, 0, sizeof(p));
  p.nl = (int)m.layers.size();
  p.in_dim = m.in_dim;
  p.out_dim = m.out_dim;
  double flops = 0, wbytes = 0;
  for (int l = 0; l < p.nl; ++l) {
    const auto &d = m.layers[l];
    auto &L = p.L[l];
    L.N = d.N;
    L.skip_n = (int)d.skip.size();
    buf.skip[l] = d.skip;
    p.res[l] = d.res + 1;
    if (d.res >= 0) flops += d.N;  // the carried value's add
    L.act = d.act;
    L.alpha = d.alpha;
    L.beta = d.beta;
    if (d.ln) {
      L.ln = d.ln;
      L.ln_eps = d.ln_eps;
      if (d.ln == 1) {
        // a pre-LN layer's dense store writes the raw pre-activation and the LN pass
        // applies the layer's activation
        L.ln_act = L.act;
        L.ln_alpha = L.alpha;
        L.ln_beta = L.beta;
        L.act = ACT_NONE;
        L.alpha = L.beta = 0.f;
      }
      wbytes += 4.0 * 2.0 * d.N;
    }
    flops += 2.0 * d.K * d.N;
    wbytes += 4.0 * ((double)d.K * d.N + d.N);
  }
  pl.has_ln = program_has_ln(p);
  // An observation skip input on any layer: the program runs on the general batched body and
  // the GEMV chain alone: no pipeline (w4_eligible), LN pipeline, single launch or resident
  // form below, and no controller tick (the engine refuses it). With GO2PI_SKIP_SMALL
  // (Switches::skip_small) the single launch serves it at batch <= 8 and, of the resident
  // forms, the multi-workgroup kernel's act() (plan_resident), under the shape conditions of
  // any dense program.
  pl.has_skip = program_has_skip(p);
  // A residual connection on any layer: policy_fused_res_kernel<8> (the general body with a
  // carried tile, kernels_gen_res.hip) for batched launches and the GEMV chain at batch <=
  // small_batch; nothing else. Only the 8-wave instantiation is built (a general-body unit
  // takes minutes to compile), so an explicit waves = 4 or 16 is refused, and the
  // GO2PI_LN_BATCHED, ln_small and GO2PI_SKIP_SMALL bits have no effect on such a program.
  // With GO2PI_RESIDUAL_BATCHED (Switches::residual_batched) a program of the pipeline's shape
  // runs its batched launches on policy_mlp_res_kernel (below, w4ln_tpw); waves = 4 / 16 stay
  // refused, and every other launch of the engine runs what it runs without the switch.
  // With GO2PI_RESIDUAL_SMALL (Switches::residual_small) the single launch serves it at batch
  // <= 8 and, of the resident forms, the multi-workgroup kernel's act() with a tiled layer 0
  // (plan_resident; resident.hip multi_nf), under the shape conditions of any dense program;
  // an LN + residual program needs the GO2PI_LN_SMALL bit beside it, a skip + residual
  // program GO2PI_SKIP_SMALL.
  pl.has_res = program_has_res(p);
  if (pl.has_res && (o.waves == 4 || o.waves == 16))
    throw ApiError("a policy with residual connections runs on the 8-wave batched kernel only: waves = " +
                   std::to_string(o.waves) + " is not available for it (use 0 or 8)", GO2PI_E_INVALID);
  // The 4-wave pipeline (decided below) takes a layer 0 of 3 (mod 4) k-chunks:
  // a 48- or 98-wide observation is padded to 16 columns, not 64 (25 % / 12.5 %
  // fewer layer-0 MFMAs and fragment bytes). Other kernels take any chunk count.
  const bool w4_shape = w4_eligible(m, o, sw, pl.has_ln);
  const int k0q = (w4_shape && !m.has_gru && (ceil16(m.layers[0].K) / 16) % 4 == 3 && !sw.k0_pad64)
                      ? 16 : 64;  // (the switch: A/B diagnostics only)
  // every dense layer's fragments back to back in one arena (the pipeline finds
  // layer l from the base: fused_impl.hpp w4_layer_w)
  int maxw = 0;
  buf.off.resize(p.nl);
  for (int l = 0; l < p.nl; ++l) {
    const auto &d = m.layers[l];
    auto &L = p.L[l];
    std::vector<float> w;
    const int next_k = (l + 1 < p.nl && !m.layers[l + 1].skip.empty()) ? m.layers[l + 1].K : 0;
    pack_dense(d, l == p.nl - 1, w, buf.bias[l], L.K_pad, L.N_pad, l == 0 ? k0q : 64, next_k);
    buf.off[l] = buf.arena.size();
    buf.arena.insert(buf.arena.end(), w.begin(), w.end());
    if (d.ln) {  // scale and bias padded to N_pad with zeros
      buf.ln_g[l].assign(L.N_pad, 0.f);
      buf.ln_b[l].assign(L.N_pad, 0.f);
      std::copy(d.ln_g.begin(), d.ln_g.end(), buf.ln_g[l].begin());
      std::copy(d.ln_b.begin(), d.ln_b.end(), buf.ln_b[l].begin());
    }
    maxw = std::max({maxw, L.K_pad, L.N_pad});
  }
  if (m.has_gru) {
    pack_gru(m.gru, buf.gru_w, p.gru.I_pad);
    const int H = m.gru.H, G = m.gru.G;
    auto &bzr = buf.gru_bzr, &bh = buf.gru_bh;
    bzr.assign(2 * H, 0.f);
    bh.assign(2 * H, 0.f);
    if (m.gru.cell == 1) {  // LSTM: every gate's two biases summed (i, o, f, c)
      bzr.resize(4 * H);
      for (int j = 0; j < 4 * H; ++j) bzr[j] = m.gru.Wb[j] + m.gru.Rb[j];
    } else {
      for (int j = 0; j < H; ++j) {
        bzr[j] = m.gru.Wb[j] + m.gru.Rb[j];
        bzr[H + j] = m.gru.Wb[H + j] + m.gru.Rb[H + j];
        bh[j] = m.gru.Wb[2 * H + j];
        bh[H + j] = m.gru.Rb[2 * H + j];
      }
    }
    p.has_gru = 1;
    p.gru.I = m.gru.I;
    p.gru.H = H;
    p.gru.lbr = m.gru.lbr;
    p.gru.cell = m.gru.cell;
    p.gru.sw = m.gru.cell == 1 ? 2 * H : H;
    p.in_pad = p.gru.I_pad;
    maxw = std::max({maxw, p.gru.I_pad, H});
    flops += 2.0 * G * H * ((double)m.gru.I + H);
    wbytes += 4.0 * ((double)G * H * (m.gru.I + H) + 2.0 * G * H);
  } else {
    p.in_pad = p.L[0].K_pad;
  }
  pl.tmp_stride = maxw;
  p.lds_stride = maxw + 4;  // +16 B per row: rows start on different LDS banks
  // Every LDS column a layer reads is written first (hidden N_pad == next K_pad,
  // the observation stage writes [0, in_pad)), except after a GRU whose H is not
  // a multiple of 64: then the columns [H, ceil64(H)) must be cleared once.
  p.zero_fill = (m.has_gru && m.gru.H % 64) ? 1 : 0;
  // head fusion: a narrow final layer (<= 2 tiles) whose predecessor runs one tile
  // group set per wave (T >= waves) is folded into the predecessor's epilogue
  if (p.nl >= 2 && !sw.no_head_fuse) {  // (the switch: A/B diagnostics only)
    const int t_last = p.L[p.nl - 1].N_pad / 16, t_prev = p.L[p.nl - 2].N_pad / 16;
    // (not behind a LayerNormalization: dense_layer_head feeds the head from un-normalised registers)
    // (nor a head with a skip input: its observation columns are not in those registers)
    // (nor a program with residual connections: switched off for it, so that the layer in front
    // of the head, which may carry a sum, runs the one dense store every other layer runs)
    if (t_last <= 2 && t_prev >= pl.waves && !p.L[p.nl - 2].ln && !p.L[p.nl - 1].skip_n && !pl.has_res)
      p.head_fuse = t_last;
  }
  // 4-wave uniform-MLP pipeline (kernels.hip, w4_step): a fused head, and
  // every hidden layer exactly one group of 2, 4 or 8 tiles per wave. It is the
  // default (waves = 0) wherever it applies: measured faster than the generic
  // 8-wave body; otherwise waves = 0 means 8.
  // (a GRU policy runs its cell first and hands h' to the pipeline as layer 0's input)
  if (w4_shape) {
    const int tpw = p.L[0].N_pad / 64;
    pl.waves = 4;
    p.head_fuse = p.L[p.nl - 1].N_pad / 16;
    p.w4_tpw = tpw;
    p.w4_bias = (p.nl - 1) * 64 * tpw;
    for (int l = 0; l + 1 < p.nl; ++l) buf.bpack.insert(buf.bpack.end(), buf.bias[l].begin(), buf.bias[l].end());
  }

  // prologue: model-defined (Sub/Div/Mul/Clip nodes) and/or opts-defined normalisation
  buf.pre_sub = m.pre_sub;
  buf.pre_div = m.pre_div;
  buf.pre_mul = m.pre_mul;
  if (o.obs_mean) {
    if (!buf.pre_sub.empty())
      throw ApiError("model already normalises its input; obs_mean not allowed", GO2PI_E_INVALID);
    buf.pre_sub.assign(o.obs_mean, o.obs_mean + m.in_dim);
  }
  if (o.obs_std) {
    if (!buf.pre_div.empty())
      throw ApiError("model already normalises its input; obs_std not allowed", GO2PI_E_INVALID);
    buf.pre_div.assign(o.obs_std, o.obs_std + m.in_dim);
  }
  if (!buf.pre_mul.empty() && (o.obs_mean || o.obs_std))
    throw ApiError("model already scales its input; obs_mean / obs_std not allowed", GO2PI_E_INVALID);
  p.pre_sub_bcast = buf.pre_sub.size() == 1;
  p.pre_div_bcast = buf.pre_div.size() == 1;
  p.pre_mul_bcast = buf.pre_mul.size() == 1;
  p.obs_lo = m.pre_lo;
  p.obs_hi = m.pre_hi;
  if (o.obs_clip > 0.f) {
    p.obs_lo = std::max(p.obs_lo, -o.obs_clip);
    p.obs_hi = std::min(p.obs_hi, o.obs_clip);
  }
  p.pre_clip = (std::isfinite(p.obs_lo) || std::isfinite(p.obs_hi)) ? 1 : 0;
  // action epilogue: the graph's trailing Clip / scalar Mul (post_fn: clip, then
  // scale), then the options'. The options apply after the graph, which post_fn's
  // fixed order tanh -> clip -> scale can only express when the graph adds no scale
  // (and, for tanh, no clip either).
  const bool m_clip = std::isfinite(m.clip_lo) || std::isfinite(m.clip_hi);
  if (o.action_tanh && (m_clip || m.post_scale != 1.f))
    throw ApiError("action_tanh on a graph that clips or scales its output is not supported", GO2PI_E_INVALID);
  if (o.action_clip > 0.f && m.post_scale != 1.f)
    throw ApiError("action_clip on a graph that scales its output is not supported", GO2PI_E_INVALID);
  p.post_tanh = o.action_tanh ? 1 : 0;
  p.clip_lo = m.clip_lo;
  p.clip_hi = m.clip_hi;
  if (o.action_clip > 0.f) {
    p.clip_lo = std::max(p.clip_lo, -o.action_clip);
    p.clip_hi = std::min(p.clip_hi, o.action_clip);
  }
  p.scale = m.post_scale * ((o.action_scale != 0.f) ? o.action_scale : 1.f);

  const size_t lds = fused_lds_bytes(p, pl.waves);
  if (lds > 160 * 1024)
    throw ApiError("layer width " + std::to_string(maxw) + " needs " + std::to_string(lds) +
                   " B of LDS per tile (> 160 KiB)" +
                   (pl.has_res ? ": a policy with residual connections holds a third activation buffer, the carried tile"
                               : ""),
                   GO2PI_E_MODEL);

  // a layer past the first with more than 512 input columns: at batch 5 and up its input
  // rows pass the 4096 granules one sweep round takes. The single launch and the
  // resident act() form sweep a second round (their general instantiations,
  // program.hpp program_small_general); the resident controller and recurrent forms do not
  int kmax1 = 0;
  for (int l = 1; l < p.nl; ++l) kmax1 = std::max(kmax1, p.L[l].K_pad);
  pl.one_round = kmax1 <= 512;
  // single-launch small-batch path: dense programs whose layers fit the kernel's
  // register slots (K_pad <= 1024) and whose widest layer fits one resident grid
  pl.latency_shape = std::max(kmax1, p.L[0].K_pad) <= 1024 && latency_grid(p) <= 256 && pl.small_batch > 0 &&
                     !sw.small_chain;  // (the switch: diagnostics, force the GEMV chain)
  // (a LayerNormalization policy: only with opts.ln_small's GO2PI_LN_SMALL bit, ln_bits;
  // latency_body normalises the swept rows as gemv_layer_kernel does)
  // (a policy with observation skip inputs: only with GO2PI_SKIP_SMALL)
  // (a policy with residual connections: only with GO2PI_RESIDUAL_SMALL)
  pl.latency_ok = !m.has_gru && pl.latency_shape && (!pl.has_ln || (ln_bits(o) & GO2PI_LN_SMALL)) &&
                  (!pl.has_skip || sw.skip_small) && (!pl.has_res || sw.residual_small);
  // the resident kernel's GRU / LSTM form (resident.hip, RNN): the cell tiled in front
  // of the dense layers, h' carried between requests as granules (an LSTM's c in the
  // owning workgroups' LDS)
  pl.res_rnn = m.has_gru && ((m.gru.cell == 0 && m.gru.lbr == 1) || m.gru.cell == 1) && m.gru.H % 64 == 0 &&
               p.gru.I_pad + m.gru.H <= 512 && (m.gru.H >> 4) <= 256 && pl.latency_shape && o.resident_ms > 0 &&
               !pl.has_ln && pl.one_round && !pl.has_skip && !pl.has_res;
  pl.done_ok = (pl.latency_ok || pl.res_rnn) && p.L[p.nl - 1].N_pad == 16;
  // controller tick: a policy with kHistory x 49 observations and 12 actions
  if (m.in_dim > 0 && m.in_dim % GO2PI_CTL_STEP_DIM == 0 && m.in_dim <= 16 * GO2PI_CTL_STEP_DIM &&
      m.out_dim == GO2PI_CTL_DOF)
    pl.ctl_hist = m.in_dim / GO2PI_CTL_STEP_DIM;

  // The pipeline's LN kernel (w4ln_impl.hpp policy_mlp_ln_kernel) for batched launches, with
  // opts.ln_small's GO2PI_LN_BATCHED bit: a dense LN policy of the pipeline's shape and the
  // lean kernel's conditions (no prologue constants or clip, no action post-processing, an
  // observation no wider than the hidden layers). The program stays the general body's in
  // every other respect, so the controller tick, the GEMV chain, the single launch and the
  // resident forms run what they run without the bit. Anything else keeps the general body.
  // The pipeline's residual kernel (policy_mlp_res_kernel, the same body with the carried value
  // in registers) with GO2PI_RESIDUAL_BATCHED: a residual program, with or without an LN and
  // whatever opts.ln_small says, under the same conditions, except that its hidden layers need
  // not share an activation. It takes the LN pipeline's fields (w4ln_tpw, the pack: zero Scale
  // / B for a layer without LN); w4ln_tpw != 0 && program_has_res(p) identifies the form.
  // Anything else (a skip input, 64-wide or non-uniform hidden layers, waves = 8, a prologue)
  // keeps policy_fused_res_kernel<8>.
  const bool ln_pipe = (ln_bits(o) & GO2PI_LN_BATCHED) && pl.has_ln && !pl.has_res;
  const bool res_pipe = sw.residual_batched && pl.has_res;
  if ((ln_pipe || res_pipe) && !pl.has_skip && !m.has_gru && o.waves == 0 && !sw.no_w4 && !sw.no_head_fuse) {
    const int tpw = w4_shape_tpw(m, !res_pipe), nh = p.nl - 1;
    const bool bare = buf.pre_sub.empty() && buf.pre_div.empty() && buf.pre_mul.empty() && !p.pre_clip &&
                      post_plain(p) && p.lds_stride == 64 * tpw + 4;
    if (tpw && bare && p.in_dim < 4096 && p.L[0].K_pad / 16 < 256 && (p.L[0].K_pad / 16) % 4 == 0 &&
        sizeof(float) * (size_t)w4ln_lds(tpw, p.L[nh].N_pad / 16, nh).total <= (size_t)W4LN_MAX_LDS_BYTES) {
      p.w4ln_tpw = tpw;
      const size_t W = 64 * (size_t)tpw;
      buf.lnpack.assign(3 * nh * W, 0.f);
      for (int l = 0; l < nh; ++l) {
        std::copy(buf.bias[l].begin(), buf.bias[l].end(), buf.lnpack.begin() + l * W);
        std::copy(buf.ln_g[l].begin(), buf.ln_g[l].end(), buf.lnpack.begin() + (nh + l) * W);
        std::copy(buf.ln_b[l].begin(), buf.ln_b[l].end(), buf.lnpack.begin() + (2 * nh + l) * W);
      }
    }
  }
  // the pipeline's hot block (program.hpp): what it reads, in one scalar burst
  fill_hot_block(p);
  if (p.w4_tpw) {
    p.w4_c0m = p.c0 % 4;
    // no prologue arithmetic, an LDS row no wider than the hidden layers
    const bool bare = buf.pre_sub.empty() && buf.pre_div.empty() && buf.pre_mul.empty() && !p.pre_clip &&
                      p.post_plain && p.lds_stride == 64 * p.w4_tpw + 4;
    // the lean kernel: no prologue / epilogue arithmetic, no recurrent cell
    p.w4_plain = !p.has_gru && bare && !sw.no_plain;
    // the lean kernel's compile-time activation: Elu (the exported rsl_rl / Isaac policies'), else runtime
    // (1 = Elu with alpha 1, the ONNX default; any other alpha takes the runtime form)
    p.w4_actc = (p.hid_act == 1 && p.hid_alpha == 1.f && !sw.lean_rt_act) ? 1 : -1;  // (the switch: A/B only)
    // ... and its hidden-layer count (3: the usual policy depth): the layer loop fully
    // unrolled, so no ring-register copies (and no vmcnt(0)) at the layer boundaries.
    // The general body (recurrent policies) takes both only together.
    p.w4_nhc = (p.w4_actc == 1 && p.nl - 1 == 3 && !sw.lean_rt_nh) ? 3 : 0;  // (the switch: A/B only)
    if (!p.w4_plain && p.w4_nhc == 0) p.w4_actc = -1;
    // the lean recurrent tick (policy_gru_kernel, r05; policy_lstm_kernel, r06): a GRU cell
    // (lbr = 1) or an LSTM cell in front of a dense chain the lean kernel would serve
    // (GO2PI_GRU_GENERAL=1 keeps the general body for both cells, A/B)
    p.w4_gru_lean = (p.has_gru && ((p.gru.cell == 0 && p.gru.lbr == 1) || p.gru.cell == 1) &&
                     (p.gru.H == 128 || p.gru.H == 256) && p.gru.H <= 64 * p.w4_tpw && bare && p.w4_actc == 1 &&
                     p.w4_nhc == 3 && p.c0 == p.gru.H / 16 && p.gru.I_pad == (p.in_dim + 63) / 64 * 64 &&
                     p.in_dim < 4096 && !p.zero_fill && !sw.gru_general) ? 1 : 0;
  }
  // the controller tick's general body instead of the lean tick kernel (A/B diagnostics,
  // tests/test_gpu_controller.py::test_controller_tick_bodies)
  p.ctl_general = sw.ctl_general ? 1 : 0;

  pl.cost.flops_per_row = flops;
  pl.cost.weight_bytes = wbytes;
  pl.cost.io_bytes_per_row = 4.0 * (m.in_dim + m.out_dim) + (m.has_gru ? 8.0 * p.gru.sw : 0.0);
  pl.cost.n_layers = p.nl;
  pl.cost.has_gru = p.has_gru ? (p.gru.cell == 1 ? 2 : 1) : 0;  // 1 GRU, 2 LSTM (go2pi.h)
  return pl;
}

// The resident kernel of each kind of request (program.hpp ResForm), decided here and
// nowhere else. Every policy with a resident path has the multi-workgroup kernel; a
// dense one takes a better form where one applies (GO2PI_RES_MULTI=1: never, A/B and
// the multi-workgroup form's tests):
//  - one workgroup, where the weights fit one CU's registers (no inter-workgroup hop per
//    layer): policy_act1_kernel wherever its shape applies (GO2PI_RES_R1W=1: never), else
//    r04's policy_resident1_kernel where that fits;
//  - act() of a wide policy (every hidden layer 256 or 512 wide: BASELINE configs[1]'s
//    48 -> 512^3 -> 12): policy_wide_kernel, when every workgroup can poll the request
//    ring in device memory (large BAR); else workgroup 0 of the multi-workgroup kernel
//    alone polls the host and mirrors the request.
// A LayerNormalization policy (opts.ln_small): of these, policy_act1_kernel's act() form
// only, and no resident controller form (its tick at batch <= 8: policy_latency_ctl_kernel).
// The controller form serves dense policies whose layer inputs fit one sweep round.
// A policy with observation skip inputs (GO2PI_SKIP_SMALL): the multi-workgroup kernel's
// act() and nothing else: the single-workgroup and wide forms keep a layer's input in
// registers or in layouts with no room for the skip columns, and the tick is refused.
// A policy with residual connections (GO2PI_RESIDUAL_SMALL): the same, for the carried value:
// only the multi-workgroup kernel's publishing lanes hold one across layers.
ResForms plan_resident(const Plan &pl, const Switches &sw, bool resident_ok, bool ring_in_vram) {
  ResForms r;
  if (!resident_ok) return r;
  const DevProgram &p = pl.prog;
  if (pl.has_skip || pl.has_res) {
    r.act = ResForm::Multi;
    return r;
  }
  const bool ln = pl.has_ln;
  const bool better = !p.has_gru && !sw.res_multi;
  const bool act1 = better && !sw.res_r1w && resident_act1_fits(p);
  r.act = ResForm::Multi;
  if (act1) r.act = ResForm::Act1;
  else if (better && !ln && resident_r1_fits(p, false)) r.act = ResForm::R1;
  else if (better && !ln && ring_in_vram && wide_shape(p).nl > 0) r.act = ResForm::Wide;
  if (!p.has_gru && !ln && pl.one_round) {
    r.ctl = ResForm::Multi;
    if (act1) r.ctl = ResForm::Act1;
    else if (better && resident_r1_fits(p, true)) r.ctl = ResForm::R1;
  }
  return r;
}

// (go2pi_run's selection at batch <= GO2PI_SMALL_MAXB: use_latency, use_graph, use_chain)
void small_kernel_name(const DevProgram &p, int waves, int small_batch, bool latency_ok, bool use_graph, char *buf,
                       size_t cap) {
  if (latency_ok)
    std::snprintf(buf, cap, "%s", latency_kernel_name());
  else if (!p.has_gru && small_batch > 0)  // (use_chain(1))
    std::snprintf(buf, cap, "%s%s", gemv_kernel_name(), use_graph ? " graph" : "");
  else
    batched_kernel_name(p, waves, buf, cap);
}

}  // namespace go2pi
