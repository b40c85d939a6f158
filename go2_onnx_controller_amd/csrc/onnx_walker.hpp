// The ONNX loader's walker: the main chain from graph input 0 to output 0, one node at a time,
// lowered into Model's program. Internal to onnx_model.cpp.
//
// step() picks the next node (next_node) and dispatches it to one handler per operator. The
// dispatch tests its cases in a fixed order, and that order is the refusal priority: a malformed
// graph gets the message of the first case it matches (an Add between a LayerNormalization and
// its activation is refused as that before it is looked at as a bias).
#pragma once

#include "onnx_front_end.hpp"

namespace go2pi {
namespace {

int act_of(const std::string &op) {
  static const std::pair<const char *, int> kActs[] = {
      {"Elu", ACT_ELU}, {"Relu", ACT_RELU}, {"Tanh", ACT_TANH}, {"Sigmoid", ACT_SIGMOID}, {"LeakyRelu", ACT_LEAKY},
      {"Selu", ACT_SELU}, {"Softplus", ACT_SOFTPLUS}, {"HardSigmoid", ACT_HARDSIGMOID}, {"HardSwish", ACT_HARDSWISH},
      {"Softsign", ACT_SOFTSIGN}};
  for (auto &a : kActs)
    if (op == a.first) return a.second;
  return -1;
}

// The node's attributes with the ONNX defaults (opset 6+ for Elu / LeakyRelu /
// Selu / HardSigmoid, opset 14 HardSwish: alpha = 1/6, beta = 0.5 fixed).
void act_attrs(const Node &nd, int act, float &alpha, float &beta) {
  alpha = beta = 0.f;
  switch (act) {
    case ACT_ELU: alpha = nd.fattr("alpha", 1.f); break;
    case ACT_LEAKY: alpha = nd.fattr("alpha", 0.01f); break;
    case ACT_SELU:
      alpha = nd.fattr("alpha", 1.67326319217681884765625f);
      beta = nd.fattr("gamma", 1.05070102214813232421875f);
      break;
    case ACT_HARDSIGMOID:
      alpha = nd.fattr("alpha", 0.2f);
      beta = nd.fattr("beta", 0.5f);
      break;
    case ACT_HARDSWISH:
      alpha = 1.f / 6.f;
      beta = 0.5f;
      break;
    default: break;
  }
}

struct Walker {
  const GraphView &gv;
  Model &m;
  const std::string &final_out;  // graph output 0

  // ---- the walk's state, and what each member means between two steps
  // cur: the running value, the one the next node consumes. Every value on the chain has one
  // unused consumer, except x0 (skip Concats read it too) and a residual connection's tap.
  std::string cur;
  // used[k]: node k is lowered (by the front-end, a step, or resolve_part) and is no successor.
  std::vector<bool> used;
  // x0: the value layer 0 reads (the observation after its prologue / front-end), named in front
  // of any Identity; x0_width its columns. Empty until the first Gemm / MatMul, or the Slice in
  // front of it, is met; skip parts resolve against it (onnx_model.hpp Dense::skip).
  std::string x0;
  int64_t x0_width = 0;
  // l0_sliced: layer 0 reads the columns l0_cols of x0 through a Slice (a gather: a column it
  // does not read is never multiplied, so a non-finite value there cannot reach it). Set by
  // that Slice; until layer 0 exists only a Gemm / MatMul (or Identity) may follow.
  bool l0_sliced = false;
  Cols l0_cols;
  // pend.on: true only between a skip Concat and its Gemm / MatMul (only Identity may stand
  // between), which takes the column order from it and clears it.
  struct {
    bool on = false;
    int nrun = 0;                 // the running value's width
    std::vector<int> perm, skip;  // device column j <- ONNX column perm[j]; x0 column of device column nrun + j
  } pend;
  // tap.on: a residual connection is open (onnx_model.hpp Dense::res): `name` (in front of any
  // Identity) holds layer `layer`'s carried value and an Add behind a later Gemm / MatMul
  // closes it. At most one tap is live.
  struct {
    bool on = false;
    std::string name;
    int layer = -1;
  } tap;
  // last_has_act: the last layer's activation (or the recurrent cell) is behind cur; false only
  // from a Gemm / MatMul to its activation. True in front of the first layer.
  bool last_has_act = true;
  // pending_bias_ok: true only between a Gemm / MatMul and anything but a constant Add or a
  // folded Mul / Div: a constant Add is that layer's bias.
  bool pending_bias_ok = false;
  // col_scale: a constant Mul / Div behind the last layer's activation, held for the next
  // Gemm / MatMul's input columns (begin_layer) or the output scale (finish). Empty: none.
  std::vector<float> col_scale;
  // post_clip: a Clip stands behind the last layer's activation; only the graph's end, a scalar
  // Mul / Div or another such Clip may follow.
  bool post_clip = false;
  size_t rnn_node = SIZE_MAX;  // the recurrent cell's node

  Walker(const GraphView &g, Model &model)
      : gv(g), m(model), final_out(g.outputs[0].name), cur(g.obs()), used(g.nodes.size(), false) {}

  void run() {
    front_end(m, gv, used, cur);
    while (cur != final_out) step();
    finish();
  }

  bool at_input() const { return m.layers.empty() && !m.has_gru; }  // still in front of the first layer
  const std::string &other_input(const Node &nd) const {
    if (nd.in.size() < 2) fail(nd.op + " needs two inputs");
    return nd.in[0] == cur ? nd.in[1] : nd.in[0];
  }

  // The successor of cur: its one unused consumer; of several, the main chain beside a residual
  // connection's tap, or beside the observation's skip branches.
  size_t next_node() {
    auto it = gv.consumers.find(cur);
    size_t idx = SIZE_MAX, n_unused = 0;
    if (it != gv.consumers.end())
      for (size_t k : it->second)
        if (!used[k]) {
          if (idx == SIZE_MAX) idx = k;
          ++n_unused;
        }
    bool tapped = false;
    if (n_unused > 1 && !at_input())
      for (size_t k : it->second) tapped |= !used[k] && gv.add_ward(k);
    if (tapped) {
      idx = open_tap(it->second);
    } else if (n_unused > 1) {
      // the observation with skip branches: the main chain is the consumer that does not
      // lead, through Slice / Identity alone, to a Concat (nor to a residual Add, which is
      // refused where the chain reaches it)
      for (size_t k : it->second)
        if (!used[k] && !gv.node_to_concat(k)) { idx = k; break; }
      if (at_input())
        for (size_t k : it->second)
          if (!used[k] && !gv.node_to_concat(k) && !gv.obs_to_add(k)) { idx = k; break; }
    }
    if (idx == SIZE_MAX) fail("dangling value '" + cur + "' does not reach output '" + final_out + "'");
    return idx;
  }

  // A residual connection's tap: cur has two consumers, the main chain and the closing Add
  // (through Identity). Remembers the tensor and returns the main chain's node.
  size_t open_tap(const std::vector<size_t> &consumers) {
    size_t n_add = 0, n_main = 0, main = SIZE_MAX;
    for (size_t k : consumers) {
      if (used[k]) continue;
      if (gv.add_ward(k)) ++n_add;
      else if (n_main++ == 0) main = k;
    }
    if (m.has_gru) fail("a residual connection in a policy with a GRU or LSTM cell is unsupported");
    if (n_add > 1) fail("the tap '" + cur + "' of a residual connection is consumed by more than one Add");
    if (n_main != 1 || consumers.size() > 2)
      fail("a value with more than two consumers ('" + cur + "') cannot be the tap of a residual connection");
    if (tap.on)
      fail("nested or overlapping residual connections are unsupported: '" + cur + "' is tapped while the one from "
           "layer " + std::to_string(tap.layer) + " is open");
    const std::string mop = gv.real_op(main);
    const bool mact = act_of(mop) >= 0 || mop == "Clip";
    if (m.layers.back().ln)
      fail("a residual connection tapped from a LayerNormalization's output (or behind it) is unsupported: the "
           "carried value of a layer with a LayerNormalization is that LayerNormalization's input");
    if (post_clip || !col_scale.empty() || (last_has_act && (mop == "Mul" || mop == "Div")))
      fail("a residual connection from a layer with a constant Mul / Div (or Clip) behind its activation is "
           "unsupported");
    if (!last_has_act && mact)
      fail("a residual connection tapped between a Gemm / MatMul and its activation is unsupported (tap the "
           "activation's output, or the input of a LayerNormalization)");
    if (mop != "LayerNormalization" && mop != "Gemm" && mop != "MatMul" && mop != "Concat")
      fail("the tap of a residual connection must feed a LayerNormalization, the next Gemm / MatMul or a skip "
           "Concat, not '" + mop + "'");
    tap = {true, gv.canon(cur), (int)m.layers.size() - 1};
    return main;
  }

  void step() {
    const size_t idx = next_node();
    used[idx] = true;
    const Node &nd = gv.nodes[idx];
    const std::string &op = nd.op;
    const bool linear = op == "Gemm" || op == "MatMul";
    if (pend.on && !linear && op != "Identity")
      fail("a skip Concat must feed a Gemm or MatMul: '" + op + "' applied to the concatenation is unsupported");
    if (l0_sliced && at_input() && !linear && op != "Identity")
      fail("a Slice of the observation in front of the first layer must feed a Gemm or MatMul, not '" + op + "'");

    if (op == "Gemm") on_gemm(nd);
    else if (op == "MatMul") on_matmul(nd);
    else if (op == "LayerNormalization") on_layernorm(nd);
    else if (gv.real_add(idx)) on_residual_add(nd);
    else if (!m.layers.empty() && m.layers.back().ln == 1 && !last_has_act &&
             (op == "Add" || op == "Mul" || op == "Div" || op == "Sub"))
      fail(op + " between a LayerNormalization and its activation is unsupported");
    else if (op == "Add" && gv.is_init(other_input(nd))) on_bias_add(nd);
    else if (op == "Add" && nd.in.size() >= 2)
      fail("Add of two computed values (a residual connection) is unsupported (node '" + nd.name + "')");
    else if (op == "Slice") on_slice(nd);
    else if (op == "Concat") on_skip_concat(nd);
    else if (at_input() && (op == "Mul" || ((op == "Sub" || op == "Div") && nd.in[0] == cur)) && gv.is_init(other_input(nd)))
      on_prologue_arith(nd);
    else if ((op == "Mul" || (op == "Div" && nd.in[0] == cur)) && gv.is_init(other_input(nd))) on_scale(nd);
    else if (op == "Clip") on_clip(nd);
    else if (act_of(op) >= 0) on_activation(nd);
    else if (op == "Identity" || op == "Flatten") {}  // pass-through on [B, F]
    else if (op == "Unsqueeze") on_unsqueeze(nd);
    else if (op == "GRU" || op == "LSTM") return on_rnn(nd, idx);  // (sets cur itself: the cell has two outputs)
    else if (op == "Squeeze") { if (!m.has_gru) fail("Squeeze is only supported after a GRU or LSTM"); }
    else fail("unsupported operator '" + op + "' (node '" + nd.name + "')");
    if (nd.out.empty()) fail("node without output");
    cur = nd.out[0];
  }

  // must feed the recurrent cell: X [1, B, I]
  void on_unsqueeze(const Node &nd) {
    auto ci = gv.consumers.find(nd.out.at(0));
    if (ci == gv.consumers.end() || ci->second.size() != 1 ||
        (gv.nodes[ci->second[0]].op != "GRU" && gv.nodes[ci->second[0]].op != "LSTM"))
      fail("Unsqueeze is only supported in front of a GRU or LSTM");
  }

  // W [N][K] of a Gemm / MatMul's constant operand B (transposed: B is [N][K] already), times alpha
  static Dense dense_of(const Tensor &B, bool transposed, float alpha) {
    Dense d;
    d.N = int(transposed ? B.dims[0] : B.dims[1]);
    d.K = int(transposed ? B.dims[1] : B.dims[0]);
    d.W.resize(size_t(d.N) * d.K);
    for (int i = 0; i < d.N; ++i)
      for (int k = 0; k < d.K; ++k) {
        float w = transposed ? B.f[size_t(i) * d.K + k] : B.f[size_t(k) * d.N + i];
        d.W[size_t(i) * d.K + k] = alpha == 1.f ? w : alpha * w;
      }
    d.b.assign(d.N, 0.f);
    return d;
  }

  // a new linear layer: no trailing op may sit between it and the previous one,
  // except a held column scale, folded into its weights here
  void begin_layer(Dense d, const std::string &op) {
    if (post_clip) fail(op + ": a Clip after an activation is only supported at the end of the graph");
    // (I + W) z: no exported architecture writes it, and the sum would be a layer output
    // with no epilogue of its own
    if (!m.layers.empty() && m.layers.back().res >= 0 && !last_has_act && !m.layers.back().ln)
      fail(op + ": the sum of a residual connection feeds it with neither an activation nor a LayerNormalization "
           "on the sum (Gemm -> Add -> Gemm), which is unsupported");
    int nrun = d.K;  // the columns that read the previous layer's outputs
    if (pend.on) {
      // the skip Concat in front: W's columns into device order (running value first, then
      // the observation parts in Concat order)
      if (d.K != (int)pend.perm.size())
        fail(op + ": K = " + std::to_string(d.K) + " does not match its skip Concat's " +
             std::to_string(pend.perm.size()) + " columns");
      std::vector<float> W(d.W.size());
      for (int i = 0; i < d.N; ++i)
        for (int k = 0; k < d.K; ++k) W[size_t(i) * d.K + k] = d.W[size_t(i) * d.K + pend.perm[k]];
      d.W = std::move(W);
      d.skip = std::move(pend.skip);
      nrun = pend.nrun;
      pend = {};
    } else if (at_input()) {
      if (l0_sliced) {  // layer 0 reads a Slice of x0: a gather
        if (d.K != l0_cols.e - l0_cols.b)
          fail(op + ": K = " + std::to_string(d.K) + " does not match the Slice of the observation it reads");
        for (int64_t c = l0_cols.b; c < l0_cols.e; ++c) d.skip.push_back((int)c);
      } else {
        x0 = gv.canon(cur);
        x0_width = d.K;
      }
    }
    if (!col_scale.empty()) {
      // (a held scale applies to the running value's columns, not to the observation parts)
      if ((int)col_scale.size() != 1 && (int)col_scale.size() != nrun) fail(op + ": the Mul before it must broadcast over K");
      for (int i = 0; i < d.N; ++i)
        for (int k = 0; k < nrun; ++k) d.W[size_t(i) * d.K + k] *= col_scale[col_scale.size() == 1 ? 0 : k];
      col_scale.clear();
    }
    m.layers.push_back(std::move(d));
    last_has_act = false;
    pending_bias_ok = true;
  }

  void on_gemm(const Node &nd) {
    if (nd.in[0] != cur) fail("Gemm: activation must be input A");
    if (nd.iattr("transA", 0)) fail("Gemm transA=1 unsupported");
    const Tensor &B = gv.init(nd.in.at(1));
    if (B.dims.size() != 2) fail("Gemm: B must be 2-D");
    const float beta = nd.fattr("beta", 1.f);
    Dense d = dense_of(B, nd.iattr("transB", 0) != 0, nd.fattr("alpha", 1.f));
    if (nd.in.size() > 2 && !nd.in[2].empty()) {
      d.b = broadcast(gv.init(nd.in[2]), d.N, "Gemm: bias must broadcast over N");
      for (float &c : d.b) c = beta == 1.f ? c : beta * c;
    }
    begin_layer(std::move(d), "Gemm");
  }

  void on_matmul(const Node &nd) {
    if (nd.in[0] != cur) fail("MatMul: activation must be the left operand");
    const Tensor &B = gv.init(nd.in.at(1));
    if (B.dims.size() != 2) fail("MatMul: weight must be 2-D");
    begin_layer(dense_of(B, false, 1.f), "MatMul");
  }

  // opset 17, over the feature axis of the [batch, N] value: right after a layer's
  // Gemm / bias ("pre": the activation, if any, follows it) or right after its
  // activation ("post"). Anything else is refused, never approximated.
  void on_layernorm(const Node &nd) {
    if (nd.in.size() < 2 || nd.in[0] != cur) fail("LayerNormalization: the activation must be input X");
    if (at_input()) fail("LayerNormalization before the first layer is unsupported");
    if (m.layers.empty()) fail("LayerNormalization right after the recurrent cell is unsupported");
    Dense &d = m.layers.back();
    if (d.ln) fail("a second LayerNormalization on the same layer is unsupported");
    if (post_clip) fail("LayerNormalization after a Clip that follows an activation is unsupported");
    if (!col_scale.empty()) fail("a Mul or Div between an activation and its LayerNormalization is unsupported");
    const int64_t axis = nd.iattr("axis", -1);
    if (axis != -1 && axis != 1) fail("LayerNormalization: axis must be the feature axis (-1 or 1)");
    if (nd.iattr("stash_type", 1) != 1) fail("LayerNormalization: stash_type other than 1 is unsupported");
    for (size_t k = 1; k < nd.out.size(); ++k) {
      if (nd.out[k].empty()) continue;
      bool is_out = false;
      for (auto &o : m.outputs) is_out |= o.name == nd.out[k];
      if (is_out || gv.consumers.count(nd.out[k]))
        fail("LayerNormalization: the Mean / InvStdDev outputs must not be consumed");
    }
    auto param = [&](const std::string &name, const char *what) {
      auto pi = gv.inits.find(name);
      if (pi == gv.inits.end()) fail(std::string("LayerNormalization: ") + what + " must be a constant");
      if (pi->second.dtype != 1) fail(std::string("LayerNormalization: ") + what + " must be a FLOAT tensor");
      if (pi->second.numel() != d.N || (int64_t)pi->second.f.size() != d.N)
        fail(std::string("LayerNormalization: ") + what + " must have the layer's " + std::to_string(d.N) + " elements");
      return pi->second.f;
    };
    d.ln_g = param(nd.in[1], "Scale");
    if (nd.in.size() > 2 && !nd.in[2].empty()) d.ln_b = param(nd.in[2], "B");
    else d.ln_b.assign(d.N, 0.f);
    d.ln_eps = nd.fattr("epsilon", 1e-5f);
    d.ln = last_has_act ? 2 : 1;
    pending_bias_ok = false;
  }

  // a residual connection's closing Add: lowered directly behind a layer's Gemm / MatMul
  // (+ bias), against the live tap (Dense::res)
  void on_residual_add(const Node &nd) {
    if (gv.obs_derived(other_input(nd)))
      fail("the observation (or a Slice of it) as the added operand of a residual connection is unsupported (node '" +
           nd.name + "')");
    if (!tap.on || gv.canon(other_input(nd)) != tap.name)
      fail("Add of two computed values (a residual connection) is unsupported (node '" + nd.name + "')");
    if (m.has_gru) fail("a residual connection in a policy with a GRU or LSTM cell is unsupported");
    Dense &d = m.layers.back();
    const int l = (int)m.layers.size() - 1;
    if (last_has_act || d.ln || l <= tap.layer || d.res >= 0)
      fail("a residual connection added behind a layer's activation or LayerNormalization (x + act(Wx), x + LN(..)) "
           "is unsupported: the Add is lowered only directly behind the Gemm / MatMul (node '" + nd.name + "')");
    if (m.layers[tap.layer].N != d.N)
      fail("a residual connection adds the " + std::to_string(m.layers[tap.layer].N) + " features of layer " +
           std::to_string(tap.layer) + " to the " + std::to_string(d.N) + " of layer " + std::to_string(l));
    d.res = tap.layer;
    tap.on = false;
    pending_bias_ok = false;
  }

  void on_bias_add(const Node &nd) {
    const Tensor &C = gv.init(other_input(nd));
    if (m.layers.empty() || last_has_act || !pending_bias_ok) fail("Add: only a bias right after Gemm/MatMul is supported");
    Dense &d = m.layers.back();
    const std::vector<float> c = broadcast(C, d.N, "Add: bias must broadcast over N");
    for (int i = 0; i < d.N; ++i) d.b[i] += c[i];
  }

  // layer 0 reads a Slice of the observation (an encoder that reads part of it)
  void on_slice(const Node &nd) {
    if (!at_input() || nd.in.at(0) != cur)
      fail("Slice is only supported on the observation (a front-end block, a skip part or layer 0's input)");
    const auto &shape = m.inputs[0].shape;
    if (shape.size() != 2 || shape[1] <= 0 || shape[1] > INT32_MAX / 2)
      fail("Slice on the observation needs a static [batch, features] input shape");
    x0 = gv.canon(cur);
    x0_width = shape[1];
    l0_cols = gv.slice_cols(nd, x0_width);
    l0_sliced = true;
  }

  // A skip Concat's input that is not the running value: the columns of x0 it holds. It is
  // x0 itself or a Slice of it (Slices of Slices compose), Identity anywhere.
  Cols resolve_part(const std::string &name) {
    std::vector<size_t> slices;  // outermost first
    std::string v = name;
    for (int hop = 0;; ++hop) {
      if (v == x0) break;
      if (hop >= 64) fail("Concat input '" + name + "' is too deep a chain");
      auto pi = gv.producers.find(v);
      if (pi == gv.producers.end()) {
        if (v == gv.obs()) fail(kPartArith);
        fail("Concat input '" + v + "' is neither the running value nor a part of the observation");
      }
      const Node &pn = gv.nodes[pi->second];
      if (pn.in.empty()) fail("Concat input '" + v + "' is neither the running value nor a part of the observation");
      if (pn.op == "Slice") slices.push_back(pi->second);
      else if (pn.op != "Identity") {
        if (gv.obs_derived(v)) fail(kPartArith);
        fail("a Concat of two running values (two sub-networks joined) is unsupported (input '" + v + "' comes from '" +
             pn.op + "')");
      }
      used[pi->second] = true;
      v = pn.in[0];
    }
    Cols c{0, x0_width};
    for (size_t i = slices.size(); i-- > 0;) {
      const Cols r = gv.slice_cols(gv.nodes[slices[i]], c.e - c.b);
      c = Cols{c.b + r.b, c.b + r.e};
    }
    return c;
  }

  // a skip Concat: the running value and one or more parts of x0, on the feature axis
  void on_skip_concat(const Node &nd) {
    if (m.has_gru) fail("a skip Concat in a policy with a GRU or LSTM cell is unsupported");
    if (at_input())
      fail("a Concat of observation parts alone in front of the first layer is a front-end, not a skip input "
           "(node '" + nd.name + "')");
    const int64_t axis = nd.iattr("axis", 1);
    if (axis != 1 && axis != -1)
      fail("a skip Concat must be on the feature axis (1 or -1), not axis " + std::to_string(axis));
    if (post_clip) fail("Concat: a Clip after an activation is only supported at the end of the graph");
    const int prevN = m.layers.back().N;
    int64_t at = 0, run_at = -1;
    std::vector<std::pair<int64_t, Cols>> parts;  // ONNX column offset, x0 columns
    for (auto &name : nd.in) {
      if (name == cur) {
        if (run_at >= 0) fail("a skip Concat takes the running value twice");
        run_at = at;
        at += prevN;
      } else {
        const Cols c = resolve_part(name);
        parts.emplace_back(at, c);
        at += c.e - c.b;
      }
    }
    if (parts.empty() || run_at < 0) fail("a skip Concat needs the running value and at least one observation part");
    if (at > INT32_MAX / 2) fail("a skip Concat is too wide");
    pend.on = true;
    pend.nrun = prevN;
    for (int j = 0; j < prevN; ++j) pend.perm.push_back((int)run_at + j);
    for (auto &pc : parts)
      for (int64_t c = pc.second.b; c < pc.second.e; ++c) {
        pend.perm.push_back((int)(pc.first + (c - pc.second.b)));
        pend.skip.push_back((int)c);
      }
  }

  // observation normalisation, evaluated as written: (x - sub) / div * mul
  void on_prologue_arith(const Node &nd) {
    const std::string &op = nd.op;
    if (op != "Mul") gv.init(other_input(nd));  // (a constant that is no FLOAT tensor: a Sub / Div's first refusal, a Mul's last)
    std::vector<float> &dst = op == "Sub" ? m.pre_sub : op == "Div" ? m.pre_div : m.pre_mul;
    if (!dst.empty()) fail("only one " + op + " in the prologue is supported");
    if (op == "Sub" && (!m.pre_div.empty() || !m.pre_mul.empty())) fail("prologue must be Sub, then Div / Mul");
    if (!m.pre_mul.empty() || std::isfinite(m.pre_lo) || std::isfinite(m.pre_hi))
      fail("prologue must be Sub, Div, Mul, then Clip");
    dst = gv.init(other_input(nd)).f;
  }

  // a constant scale between or after the layers (its reciprocal for a Div)
  void on_scale(const Node &nd) {
    const Tensor &C = gv.init(other_input(nd));
    if (m.has_gru && m.layers.empty()) fail(nd.op + " right after the recurrent cell is unsupported");
    if (post_clip && C.numel() != 1) fail("a per-feature " + nd.op + " after the output Clip is unsupported");
    Dense &d = m.layers.back();
    if (!last_has_act && d.res >= 0)
      fail("a constant " + nd.op + " between the Add of a residual connection and the activation is unsupported");
    std::vector<float> sc = broadcast(C, d.N, nd.op + " must broadcast over " + std::to_string(d.N) + " features");
    for (auto &v : sc) v = nd.op == "Div" ? 1.f / v : v;
    if (!last_has_act) {
      // straight after Gemm (+ bias): scale the layer's rows and bias
      for (int i = 0; i < d.N; ++i) {
        for (int k = 0; k < d.K; ++k) d.W[size_t(i) * d.K + k] *= sc[i];
        d.b[i] *= sc[i];
      }
    } else {
      // after an activation: held for the next layer's input columns (or the output)
      if (C.numel() == 1) sc.resize(1);
      if (col_scale.empty()) col_scale = sc;
      else if (col_scale.size() == 1 && sc.size() == 1) col_scale[0] *= sc[0];
      else fail("two vector Mul / Div in a row are unsupported");
    }
  }

  void on_clip(const Node &nd) {
    float lo, hi;
    gv.clip_bounds(nd, nullptr, lo, hi);
    if (at_input()) {
      // clip of the observation (after any normalisation)
      m.pre_lo = std::max(m.pre_lo, lo);
      m.pre_hi = std::min(m.pre_hi, hi);
    } else if (m.has_gru && m.layers.empty()) {
      fail("Clip right after the recurrent cell is unsupported");
    } else if (!last_has_act) {
      // the layer's activation (ReLU6 = Clip(0, 6)), applied in its epilogue
      Dense &d = m.layers.back();
      d.act = ACT_CLIP;
      d.alpha = lo;
      d.beta = hi;
      last_has_act = true;
      pending_bias_ok = false;
    } else {
      // after an activation: only as the output clip (the action epilogue)
      if (!col_scale.empty()) fail("Clip after a Mul that follows an activation is unsupported");
      m.clip_lo = std::max(m.clip_lo, lo);
      m.clip_hi = std::min(m.clip_hi, hi);
      post_clip = true;
    }
  }

  void on_activation(const Node &nd) {
    if (m.layers.empty()) fail(nd.op + " before any linear layer");
    if (last_has_act) fail("two activations in a row are unsupported");
    Dense &d = m.layers.back();
    d.act = act_of(nd.op);
    act_attrs(nd, d.act, d.alpha, d.beta);
    last_has_act = true;
    pending_bias_ok = false;
  }

  // ONNX GRU (opset 14: gates z, r, h) or LSTM (opset 14: gates i, o, f, c), one
  // forward direction, default activations, as torch.onnx.export writes nn.GRU / nn.LSTM
  void on_rnn(const Node &nd, size_t idx) {
    const bool lstm = nd.op == "LSTM";
    const std::string op = nd.op;
    if (m.has_gru) fail("only one recurrent layer is supported");
    if (!m.layers.empty()) fail(op + " must be the first layer of the policy");
    if (nd.iattr("layout", 0) != 0) fail(op + " layout=1 unsupported");
    const Tensor &W = gv.init(nd.in.at(1));
    const Tensor &R = gv.init(nd.in.at(2));
    Gru &g = m.gru;
    g.cell = lstm ? 1 : 0;
    g.G = lstm ? 4 : 3;
    if (W.dims.size() != 3 || W.dims[0] != 1)
      fail(op + ": W must be [1, " + std::to_string(g.G) + "H, I] (one direction)");
    g.H = int(R.dims.at(2));
    g.I = int(W.dims[2]);
    if (R.dims.size() != 3 || R.dims[0] != 1 || g.H <= 0 || g.I <= 0) fail(op + ": R must be [1, G*H, H], H > 0");
    if (W.dims[1] != g.G * g.H || R.dims[1] != g.G * g.H) fail(op + ": gate dims mismatch");
    g.lbr = lstm ? 0 : int(nd.iattr("linear_before_reset", 0));
    g.W = W.f;
    g.R = R.f;
    g.Wb.assign((size_t)g.G * g.H, 0.f);
    g.Rb.assign((size_t)g.G * g.H, 0.f);
    if (nd.in.size() > 3 && !nd.in[3].empty()) {
      const Tensor &B = gv.init(nd.in[3]);
      if (B.numel() != (int64_t)2 * g.G * g.H) fail(op + ": B must be [1, " + std::to_string(2 * g.G) + "H]");
      std::copy(B.f.begin(), B.f.begin() + (long)g.G * g.H, g.Wb.begin());
      std::copy(B.f.begin() + (long)g.G * g.H, B.f.end(), g.Rb.begin());
    }
    if (nd.in.size() > 4 && !nd.in[4].empty()) fail(op + ": sequence_lens unsupported");
    if (nd.attrs.count("activations")) fail(op + ": custom activations unsupported");
    if (nd.attrs.count("clip")) fail(op + ": cell clip unsupported");
    if (lstm && nd.iattr("input_forget", 0) != 0) fail("LSTM: input_forget=1 unsupported");
    if (lstm && nd.in.size() > 7 && !nd.in[7].empty()) fail("LSTM: peepholes (input P) unsupported");
    m.has_gru = true;
    rnn_node = idx;
    // follow Y_h (output 1) if consumed, else Y (output 0)
    if (nd.out.size() > 1 && !nd.out[1].empty() && gv.consumers.count(nd.out[1])) cur = nd.out[1];
    else cur = nd.out.at(0);
    last_has_act = true;
    pending_bias_ok = false;
  }

  // The recurrent state I/O listed as (h, c) after the observation / action, whatever
  // the graph's order: traced by name to the cell's initial_h / initial_c (inputs 5,
  // 6) through Unsqueeze / Identity / Reshape, and Y_h / Y_c (outputs 1, 2) through
  // Squeeze / Identity / Reshape. Other extra graph inputs / outputs keep their order.
  void order_state_io() {
    const Node &cell = gv.nodes[rnn_node];
    auto is_pass = [](const std::string &op, bool in) {
      return op == "Identity" || op == "Reshape" || op == (in ? "Unsqueeze" : "Squeeze");
    };
    auto find_io = [](std::vector<IoInfo> &v, const std::string &name) -> long {
      for (size_t i = 1; i < v.size(); ++i)
        if (v[i].name == name) return (long)i;
      return -1;
    };
    // the graph input behind the cell's input k (in: backwards through each value's producer), or the
    // graph output behind its output k (forwards through the last pass-through consumer); -1: none
    auto trace = [&](bool in, size_t k) -> long {
      const std::vector<std::string> &names = in ? cell.in : cell.out;
      if (names.size() <= k || names[k].empty()) return -1;
      std::string v = names[k];
      for (int hop = 0; hop < 8; ++hop) {
        const long i = find_io(in ? m.inputs : m.outputs, v);
        if (i >= 0) return i;
        const Node *nx = nullptr;
        auto pi = gv.producers.find(v);
        auto ci = gv.consumers.find(v);
        if (in && pi != gv.producers.end() && is_pass(gv.nodes[pi->second].op, true)) nx = &gv.nodes[pi->second];
        if (!in && ci != gv.consumers.end())
          for (size_t c : ci->second)
            if (is_pass(gv.nodes[c].op, false)) nx = &gv.nodes[c];
        if (!nx || (in ? nx->in : nx->out).empty()) return -1;
        v = (in ? nx->in : nx->out)[0];
      }
      return -1;
    };
    auto reorder = [](std::vector<IoInfo> &v, long h, long c) {
      std::vector<IoInfo> r{v[0]};
      if (h > 0) r.push_back(v[h]);
      if (c > 0) r.push_back(v[c]);
      for (long i = 1; i < (long)v.size(); ++i)
        if (i != h && i != c) r.push_back(v[i]);
      v = std::move(r);
    };
    const bool lstm = m.gru.cell == 1;
    const long hi = trace(true, 5), ci = lstm ? trace(true, 6) : -1, ho = trace(false, 1), co = lstm ? trace(false, 2) : -1;
    //  the state I/O is (h) or (h, c) positionally after the observation /
    // action (actor.py maps them so): an LSTM exposes both or neither, and h and c are
    // distinct graph values
    if (lstm && ((hi >= 0) != (ci >= 0) || (ho >= 0) != (co >= 0)))
      fail("LSTM: initial_h / initial_c (and Y_h / Y_c) must both be graph I/O, or neither");
    if ((hi >= 0 && hi == ci) || (ho >= 0 && ho == co)) fail(std::string(lstm ? "LSTM" : "GRU") + ": h and c trace to the same graph I/O");
    reorder(m.inputs, hi, ci);
    reorder(m.outputs, ho, co);
  }

  // the graph's end: nothing may be left open, and the layers' dims must chain
  void finish() {
    if (pend.on) fail("a skip Concat must feed a Gemm or MatMul: it is the graph's output");
    if (m.layers.empty()) fail("policy has no linear layer");
    if (m.layers.back().ln) fail("LayerNormalization on the output layer is unsupported");
    if (m.layers.back().res >= 0) fail("a residual connection on the output layer is unsupported");
    if (tap.on) fail("the tap of a residual connection from layer " + std::to_string(tap.layer) + " is never added");
    if (rnn_node != SIZE_MAX) order_state_io();
    if (!col_scale.empty()) {
      if (col_scale.size() != 1) fail("a per-feature Mul after the final activation is unsupported");
      m.post_scale = col_scale[0];
    }
    m.in_dim = m.has_gru ? m.gru.I : l0_sliced ? (int)x0_width : m.layers[0].K;
    if (m.has_gru && m.layers[0].K != m.gru.H) fail("recurrent hidden size does not match the first dense layer");
    for (size_t l = 1; l < m.layers.size(); ++l)
      if (m.layers[l].K != m.layers[l - 1].N + (int)m.layers[l].skip.size())
        fail("layer " + std::to_string(l) + " input dim mismatch");
    for (auto &d : m.layers) {
      if (m.has_gru && !d.skip.empty()) fail("a skip input in a policy with a GRU or LSTM cell is unsupported");
      for (int c : d.skip)
        if (c < 0 || c >= m.in_dim) fail("a skip input reads a column outside the observation");
    }
    m.out_dim = m.layers.back().N;
    if (!m.pre_sub.empty() && int(m.pre_sub.size()) != m.in_dim && m.pre_sub.size() != 1) fail("prologue Sub size");
    if (!m.pre_div.empty() && int(m.pre_div.size()) != m.in_dim && m.pre_div.size() != 1) fail("prologue Div size");
    if (!m.pre_mul.empty() && int(m.pre_mul.size()) != m.in_dim && m.pre_mul.size() != 1) fail("prologue Mul size");
    // check declared feature dims against the program (reference reads shape.at(1), onnx_actor.cpp:32,35)
    const auto &is = m.inputs[0].shape, &os = m.outputs[0].shape;
    if (is.size() >= 2 && is[1] > 0 && is[1] != m.in_dim) fail("input feature dim disagrees with weights");
    if (os.size() >= 2 && os[1] > 0 && os[1] != m.out_dim) fail("output feature dim disagrees with weights");
  }
};

}  // namespace
}  // namespace go2pi
