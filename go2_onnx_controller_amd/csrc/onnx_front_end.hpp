// The ONNX loader's per-block observation front-end. Internal to onnx_model.cpp.
//
// The observation Sliced into column blocks, each block through its own Sub / Div / Mul /
// Clip, then Concatenated on the feature axis (e.g. per-block normalisation of a controller's
// history blocks, controller.hpp:45-68). When the blocks cover the observation's columns in
// order, the front-end is exactly a per-column prologue: (x - sub[k]) / div[k] * mul[k],
// clipped, with each block's constants at its columns and the identity where a block has no
// such op. The blocks' Clip bounds must agree (the prologue clip is one interval). The walk
// then starts at the Concat's output; a graph with no Slice on the observation is left as it
// is. (The reference hands any graph to onnxruntime, onnx_actor.cpp:16; a front-end this
// cannot lower exactly is refused, never approximated.)
#pragma once

#include "onnx_graph.hpp"

namespace go2pi {
namespace {

struct Block {
  Cols cols;  // of the observation
  std::vector<float> sub, div, mul;
  float lo = -INFINITY, hi = INFINITY;
  bool clip = false;
  std::string tail;
};

// One block: the observation's Slice (node k) and its chain, Sub?, Div? / Mul?, Clip?, Identity
// anywhere, up to the Concat, which every block must share (concat: its node, SIZE_MAX before
// the first block).
Block read_block(const GraphView &gv, size_t k, int64_t F, std::vector<bool> &used, size_t &concat) {
  const Node &sl = gv.nodes[k];
  if (sl.op != "Slice" || sl.in.at(0) != gv.obs()) fail("the observation feeds a Slice front-end and a '" + sl.op + "'");
  Block bl;
  bl.cols = gv.slice_cols(sl, F);
  used[k] = true;
  const int64_t w = bl.cols.e - bl.cols.b;
  auto fconst = [&](const Node &nd, const std::string &x) {
    const std::string &o = nd.in.at(0) == x ? nd.in.at(1) : nd.in.at(0);
    auto it = gv.inits.find(o);
    if (it == gv.inits.end() || it->second.dtype != 1) fail(nd.op + " in the observation front-end needs a FLOAT constant");
    // (a constant first would be c / x or c - x: lowered as x / c or x - c, the wrong value)
    if ((nd.op == "Div" || nd.op == "Sub") && nd.in.at(0) != x)
      fail(nd.op + " in the observation front-end must take the observation as its first input");
    return broadcast(it->second, w, nd.op + " in the front-end must broadcast over its block's " + std::to_string(w) + " columns");
  };
  std::string x = sl.out.at(0);
  for (int hop = 0; hop < 16; ++hop) {
    const size_t n = gv.only_consumer(x);
    const Node &nd = gv.nodes[n];
    if (nd.op == "Concat") {
      if (concat != SIZE_MAX && concat != n) fail("the observation's Slices feed different Concats");
      concat = n;
      break;
    }
    used[n] = true;
    if (nd.op == "Identity") {
    } else if (nd.op == "Sub") {
      if (!bl.sub.empty() || !bl.div.empty() || !bl.mul.empty() || bl.clip) fail("front-end block: Sub must come first");
      bl.sub = fconst(nd, x);
    } else if (nd.op == "Div") {
      if (!bl.div.empty() || !bl.mul.empty() || bl.clip) fail("front-end block must be Sub, Div, Mul, then Clip");
      bl.div = fconst(nd, x);
    } else if (nd.op == "Mul") {
      if (!bl.mul.empty() || bl.clip) fail("front-end block must be Sub, Div, Mul, then Clip");
      bl.mul = fconst(nd, x);
    } else if (nd.op == "Clip") {
      if (bl.clip) fail("front-end block: two Clips");
      gv.clip_bounds(nd, "front-end Clip bounds must be FLOAT scalars", bl.lo, bl.hi);
      bl.clip = true;
    } else {
      fail("unsupported operator '" + nd.op + "' in the observation front-end (node '" + nd.name + "')");
    }
    if (nd.out.empty()) fail("node without output");
    x = nd.out[0];
  }
  if (concat == SIZE_MAX) fail("the observation's Slice chain does not reach a Concat");
  bl.tail = x;
  return bl;
}

// The blocks in the Concat's order must cover [0, F) in order and agree on their Clip; their
// constants side by side are the prologue's.
void concat_blocks(Model &m, const Node &cc, std::vector<Block> &blocks, int64_t F) {
  const int64_t axis = cc.iattr("axis", 1);
  if (axis != 1 && axis != -1) fail("Concat of the observation blocks must be on the feature axis");
  if (cc.in.size() != blocks.size()) fail("the Concat after the observation Slices takes other inputs too");
  std::vector<Block *> order;
  for (const auto &name : cc.in) {
    Block *hit = nullptr;
    for (auto &bl : blocks)
      if (bl.tail == name && !hit) hit = &bl;
    if (!hit) fail("Concat input '" + name + "' is not an observation block");
    order.push_back(hit);
  }
  int64_t at = 0;
  for (Block *bl : order) {
    if (bl->cols.b != at) fail("the observation blocks must cover its columns in order (a reordering front-end is unsupported)");
    at = bl->cols.e;
  }
  if (at != F) fail("the observation blocks must cover all of its columns");
  bool any_clip = false;  // (m's prologue is still empty: the front-end comes before any prologue op)
  for (Block *bl : order)
    if (bl->clip) {
      if (any_clip && (bl->lo != m.pre_lo || bl->hi != m.pre_hi)) fail("the observation blocks' Clip bounds differ");
      any_clip = true;
      m.pre_lo = bl->lo;
      m.pre_hi = bl->hi;
    }
  if (any_clip)
    for (Block *bl : order)
      if (!bl->clip) fail("only some observation blocks are clipped");
  // (an op no block has leaves the prologue's vector empty)
  auto cat = [&](std::vector<float> Block::*f, float ident, std::vector<float> &dst) {
    bool any = false;
    for (Block *bl : order) any |= !(bl->*f).empty();
    if (!any) return;
    dst.clear();
    for (Block *bl : order) {
      const auto &v = bl->*f;
      if (v.empty()) dst.insert(dst.end(), (size_t)(bl->cols.e - bl->cols.b), ident);
      else dst.insert(dst.end(), v.begin(), v.end());
    }
  };
  cat(&Block::sub, 0.f, m.pre_sub);
  cat(&Block::div, 1.f, m.pre_div);
  cat(&Block::mul, 1.f, m.pre_mul);
}

// Lowers a front-end into m's prologue and moves cur behind its Concat; leaves the graph alone
// where the observation's Slices are the walker's (skip parts, layer 0's own input).
void front_end(Model &m, const GraphView &gv, std::vector<bool> &used, std::string &cur) {
  auto ci = gv.consumers.find(gv.obs());
  if (ci == gv.consumers.end()) return;
  // a graph input with both kinds of Slice has parts that skipped the front-end's arithmetic
  size_t n_slice = 0, n_skip = 0;
  for (size_t k : ci->second)
    if (gv.nodes[k].op == "Slice" && !gv.nodes[k].out.empty()) {
      if (gv.to_res_add(gv.nodes[k].out[0]))
        fail("the observation (or a Slice of it) as the added operand of a residual connection is unsupported");
      ++n_slice;
      n_skip += gv.skip_slice(gv.nodes[k].out[0]) ? 1 : 0;
    }
  if (n_slice == 0 || n_skip == n_slice) return;
  if (n_skip) fail(kPartArith);
  const auto &shape = m.inputs[0].shape;
  if (shape.size() != 2 || shape[1] <= 0) fail("Slice on the observation needs a static [batch, features] input shape");
  std::vector<Block> blocks;
  size_t concat = SIZE_MAX;
  for (size_t k : ci->second) blocks.push_back(read_block(gv, k, shape[1], used, concat));
  concat_blocks(m, gv.nodes[concat], blocks, shape[1]);
  used[concat] = true;
  cur = gv.nodes[concat].out.at(0);
}

}  // namespace
}  // namespace go2pi
