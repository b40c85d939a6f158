// The ONNX loader's graph queries: every question the front-end and the walker ask of a Graph
// (what a value is computed from, where it leads, a constant's value), each written once.
// Internal to onnx_model.cpp. Every search has a hop or depth cap, so a cyclic file ends.
#pragma once

#include <algorithm>
#include <cmath>

#include "onnx_proto.hpp"

namespace go2pi {
namespace {

// C, a scalar or n elements, as n floats; msg: the refusal of any other size
std::vector<float> broadcast(const Tensor &C, int64_t n, const std::string &msg) {
  if (C.numel() != 1 && C.numel() != n) fail(msg);
  std::vector<float> v((size_t)n);
  for (int64_t j = 0; j < n; ++j) v[(size_t)j] = C.numel() == 1 ? C.f.at(0) : C.f.at((size_t)j);
  return v;
}

struct Cols { int64_t b = 0, e = 0; };  // columns [b, e)

// A Graph with its queries.
struct GraphView : Graph {
  const std::string &obs() const { return inputs[0].name; }  // the observation: graph input 0

  // ---- constants
  bool is_init(const std::string &name) const { return inits.count(name) > 0; }
  const Tensor &init(const std::string &name) const {
    auto it = inits.find(name);
    if (it == inits.end()) fail("'" + name + "' is not an initializer (dynamic weights unsupported)");
    if (it->second.dtype != 1) fail("'" + name + "' is not a FLOAT tensor");
    return it->second;
  }
  // a FLOAT scalar constant; msg: the one refusal of anything else, or null for a message by cause
  float scalar_of(const std::string &name, const char *msg) const {
    auto it = inits.find(name);
    if (msg && (it == inits.end() || it->second.dtype != 1 || it->second.numel() != 1 || it->second.f.empty())) fail(msg);
    const Tensor &t = init(name);
    if (t.f.empty()) fail("'" + name + "' is empty");
    if (t.numel() != 1) fail("'" + name + "' must be a scalar");
    return t.f[0];
  }
  // a Clip's interval: min / max are attributes in opset 6, optional scalar inputs from opset 11
  void clip_bounds(const Node &nd, const char *msg, float &lo, float &hi) const {
    lo = nd.fattr("min", -INFINITY);
    hi = nd.fattr("max", INFINITY);
    if (nd.in.size() > 1 && !nd.in[1].empty()) lo = scalar_of(nd.in[1], msg);
    if (nd.in.size() > 2 && !nd.in[2].empty()) hi = scalar_of(nd.in[2], msg);
  }
  // An int64 vector input of a node (Slice starts / ends / axes / steps), or empty.
  std::vector<int64_t> ints_of(const Node &nd, size_t k) const {
    if (nd.in.size() <= k || nd.in[k].empty()) return {};
    auto it = inits.find(nd.in[k]);
    if (it == inits.end() || it->second.dtype != 7) fail(nd.op + ": input " + std::to_string(k) + " must be an INT64 constant");
    return it->second.i;
  }
  // The columns [b, e) a Slice takes of a [batch, F] value: opset 10+ inputs or opset 1-9
  // attributes, negative and out-of-range bounds clamped as ONNX defines. A step other than
  // 1, the batch axis, and an empty result are refused.
  Cols slice_cols(const Node &sl, int64_t F) const {
    std::vector<int64_t> st, en, ax, sp;
    if (sl.in.size() > 1) {
      st = ints_of(sl, 1);
      en = ints_of(sl, 2);
      ax = ints_of(sl, 3);
      sp = ints_of(sl, 4);
    } else {  // opset 1-9: attributes
      auto a = sl.attrs.find("starts"), b = sl.attrs.find("ends"), c = sl.attrs.find("axes");
      if (a == sl.attrs.end() || b == sl.attrs.end()) fail("Slice without starts / ends");
      st = a->second.ints;
      en = b->second.ints;
      if (c != sl.attrs.end()) ax = c->second.ints;
    }
    if (ax.empty())
      for (size_t i = 0; i < st.size(); ++i) ax.push_back((int64_t)i);
    if (st.size() != en.size() || ax.size() != st.size() || (!sp.empty() && sp.size() != st.size()))
      fail("Slice: starts / ends / axes / steps lengths differ");
    Cols bl{0, F};
    for (size_t i = 0; i < st.size(); ++i) {
      const int64_t a = ax[i] < 0 ? ax[i] + 2 : ax[i];
      if (!sp.empty() && sp[i] != 1) fail("Slice with a step other than 1 is unsupported");
      auto clampi = [&](int64_t v, int64_t dim) { return std::max<int64_t>(0, std::min(v < 0 ? v + dim : v, dim)); };
      if (a == 0) {
        if (clampi(st[i], INT64_MAX) != 0 || en[i] < INT32_MAX) fail("Slice on the batch axis is unsupported");
      } else if (a == 1) {
        bl.b = clampi(st[i], F);
        bl.e = clampi(en[i], F);
      } else {
        fail("Slice axis out of range for a [batch, features] observation");
      }
    }
    if (bl.e <= bl.b) fail("empty Slice of the observation");
    return bl;
  }

  // ---- backwards from a value
  // v's name in front of any Identity
  std::string canon(std::string v) const {
    for (int hop = 0; hop < 64; ++hop) {
      auto pi = producers.find(v);
      if (pi == producers.end() || nodes[pi->second].op != "Identity" || nodes[pi->second].in.empty()) break;
      v = nodes[pi->second].in[0];
    }
    return v;
  }
  // v is computed from the observation alone: obs through Slice / Identity and
  // Sub / Div / Mul / Clip by constants (a front-end block, a prologue value, a skip part)
  bool obs_derived(std::string v) const {
    for (int hop = 0; hop < 64; ++hop) {
      if (v == obs()) return true;
      auto p = producers.find(v);
      if (p == producers.end()) return false;
      const Node &nd = nodes[p->second];
      if (nd.in.empty()) return false;
      if (nd.op == "Slice" || nd.op == "Identity" || nd.op == "Clip") {
        v = nd.in[0];
      } else if (nd.op == "Sub" || nd.op == "Div" || nd.op == "Mul") {
        if (nd.in.size() < 2) return false;
        const bool c0 = is_init(nd.in[0]), c1 = is_init(nd.in[1]);
        if (c0 == c1) return false;
        v = c0 ? nd.in[1] : nd.in[0];
      } else {
        return false;
      }
    }
    return false;
  }

  // ---- forwards from a value or a node
  // the one consumer of a front-end value
  size_t only_consumer(const std::string &v) const {
    auto it = consumers.find(v);
    if (it == consumers.end() || it->second.size() != 1) fail("front-end value '" + v + "' must have exactly one consumer");
    return it->second[0];
  }
  // the first operator behind node k that is no Identity
  std::string real_op(size_t k) const {
    for (int hop = 0; hop < 64 && nodes[k].op == "Identity" && !nodes[k].out.empty(); ++hop) {
      auto ci = consumers.find(nodes[k].out[0]);
      if (ci == consumers.end() || ci->second.size() != 1) break;
      k = ci->second[0];
    }
    return nodes[k].op;
  }
  // v, through Slice / Identity alone, reaches a Concat
  bool to_concat(const std::string &v, int depth = 0) const {
    auto it = consumers.find(v);
    if (it == consumers.end() || depth > 16) return false;
    for (size_t c : it->second)
      if (node_to_concat(c, depth)) return true;
    return false;
  }
  bool node_to_concat(size_t c, int depth = 0) const {
    const Node &nd = nodes[c];
    if (nd.op == "Concat") return true;
    return (nd.op == "Slice" || nd.op == "Identity") && !nd.out.empty() && to_concat(nd.out[0], depth + 1);
  }
  // node k is an Add of two computed values: a residual connection's closing Add
  bool real_add(size_t k) const {
    const Node &a = nodes[k];
    return a.op == "Add" && a.in.size() >= 2 && !is_init(a.in[0]) && !is_init(a.in[1]);
  }
  // node k is such an Add, or an Identity whose every consumer leads to one
  bool add_ward(size_t k, int depth = 0) const {
    if (real_add(k)) return true;
    const Node &a = nodes[k];
    if (a.op != "Identity" || a.out.empty() || depth > 16) return false;
    auto ci = consumers.find(a.out[0]);
    if (ci == consumers.end() || ci->second.empty()) return false;
    for (size_t c : ci->second)
      if (!add_ward(c, depth + 1)) return false;
    return true;
  }
  // node k is such an Add, or leads to one through Slice / Identity alone (the observation as
  // the added operand of a residual connection: refused). depth counts the nodes passed.
  bool obs_to_add(size_t k, int depth = 0) const {
    if (real_add(k)) return true;
    const Node &a = nodes[k];
    if ((a.op != "Identity" && a.op != "Slice") || a.out.empty() || depth > 16) return false;
    auto ci = consumers.find(a.out[0]);
    if (ci == consumers.end()) return false;
    for (size_t c : ci->second)
      if (obs_to_add(c, depth + 1)) return true;
    return false;
  }
  // ... the same from a value. The search this replaces counted the values passed from 0 and
  // stopped behind the 17th, which is where the count of nodes from 1 stops: for
  // T(v, d) = d <= 16 && any consumer c: add(c) || (pass(c) && T(out(c), d + 1)) and
  // A(k, d) = add(k) || (pass(k) && d <= 16 && any consumer c of out(k): A(c, d + 1)),
  // T(v, d) = d <= 16 && any consumer c: A(c, d + 1), by induction downwards from d = 17.
  bool to_res_add(const std::string &v) const {
    auto it = consumers.find(v);
    if (it == consumers.end()) return false;
    for (size_t c : it->second)
      if (obs_to_add(c, 1)) return true;
    return false;
  }
  // A Slice of the observation (its output v) that is no front-end block: its chain
  // feeds a Gemm / MatMul (layer 0 reads a slice) or a Concat that also
  // takes a value not computed from the observation alone (a skip Concat). A front-end
  // Concat takes observation blocks only.
  bool skip_slice(const std::string &v, int depth = 0) const {
    auto it = consumers.find(v);
    if (it == consumers.end() || depth > 16) return false;
    for (size_t c : it->second) {
      const Node &nd = nodes[c];
      if (nd.op == "Gemm" || nd.op == "MatMul") {
        if (!nd.in.empty() && nd.in[0] == v) return true;
      } else if (nd.op == "Concat") {
        for (auto &in : nd.in)
          if (!obs_derived(in)) return true;
      } else if ((nd.op == "Slice" || nd.op == "Identity" || nd.op == "Sub" || nd.op == "Div" || nd.op == "Mul" ||
                  nd.op == "Clip") &&
                 !nd.out.empty()) {
        // (arithmetic on the way too: where the chain ends decides, and the walker refuses it)
        if (skip_slice(nd.out[0], depth + 1)) return true;
      }
    }
    return false;
  }
};

const char *const kPartArith =
    "an observation part of a skip Concat must be taken from the value layer 0 reads (the observation after "
    "its prologue / front-end), with no arithmetic of its own";

}  // namespace
}  // namespace go2pi
