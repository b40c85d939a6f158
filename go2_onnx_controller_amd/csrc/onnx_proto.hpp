// The ONNX loader's protobuf reader: a model file's bytes to a Graph (nodes, initializers, who
// consumes and who produces each value, the graph's inputs and outputs). No pattern knowledge.
// Internal to onnx_model.cpp, the one unit that includes it (hence the unnamed namespace).
//
// Wire format: proto3 (varint=0, fixed64=1, length-delimited=2, fixed32=5).
// Field numbers from onnx.proto: ModelProto{ir_version=1, producer_name=2,
// graph=7, opset_import=8}; GraphProto{node=1, initializer=5, input=11,
// output=12}; NodeProto{input=1, output=2, name=3, op_type=4, attribute=5};
// AttributeProto{name=1, f=2, i=3, floats=7, ints=8}; TensorProto{dims=1,
// data_type=2, float_data=4, int64_data=7, name=8, raw_data=9};
// ValueInfoProto{name=1, type=2}; TypeProto{tensor_type=1};
// Tensor{elem_type=1, shape=2}; TensorShapeProto{dim=1};
// Dimension{dim_value=1, dim_param=2}.
//
// Initializer payloads sit at unaligned file offsets (e.g. 0.weight of the
// shipped model at byte 730), so every payload is memcpy'd, never aliased.
#pragma once

#include <cstdint>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "onnx_model.hpp"

namespace go2pi {
namespace {

[[noreturn]] void fail(const std::string &m) { throw std::runtime_error("onnx: " + m); }

struct Span {
  const uint8_t *p = nullptr;
  size_t n = 0;
};

struct Field {
  uint32_t no = 0, wt = 0;
  uint64_t v = 0;  // varint / fixed payload
  Span s;          // length-delimited payload
};

class Reader {
 public:
  explicit Reader(Span s) : p_(s.p), end_(s.p + s.n) {}
  bool next(Field &f) {
    if (p_ >= end_) return false;
    uint64_t key = varint();
    f.no = uint32_t(key >> 3);
    f.wt = uint32_t(key & 7);
    f.v = 0;
    f.s = {};
    switch (f.wt) {
      case 0: f.v = varint(); break;
      case 1: need(8); std::memcpy(&f.v, p_, 8); p_ += 8; break;
      case 2: {
        uint64_t ln = varint();
        need(ln);
        f.s = {p_, size_t(ln)};
        p_ += ln;
        break;
      }
      case 5: { uint32_t w; need(4); std::memcpy(&w, p_, 4); f.v = w; p_ += 4; break; }
      default: fail("unsupported protobuf wire type " + std::to_string(f.wt));
    }
    return true;
  }

 private:
  void need(uint64_t k) {
    if (uint64_t(end_ - p_) < k) fail("truncated protobuf");
  }
  uint64_t varint() {
    uint64_t out = 0;
    for (int shift = 0; shift < 64; shift += 7) {
      need(1);
      uint8_t b = *p_++;
      out |= uint64_t(b & 0x7F) << shift;
      if (!(b & 0x80)) return out;
    }
    fail("bad varint");
  }
  const uint8_t *p_, *end_;
};

std::string str(Span s) { return std::string(reinterpret_cast<const char *>(s.p), s.n); }

void packed_varints(const Field &f, std::vector<int64_t> &out) {
  if (f.wt == 0) {
    out.push_back(int64_t(f.v));
    return;
  }
  // packed: a run of bare varints; reuse the reader by faking keys is awkward, decode directly
  const uint8_t *p = f.s.p, *e = f.s.p + f.s.n;
  while (p < e) {
    uint64_t v = 0;
    int shift = 0;
    while (true) {
      if (p >= e) fail("bad packed varint");
      uint8_t b = *p++;
      v |= uint64_t(b & 0x7F) << shift;
      if (!(b & 0x80)) break;
      shift += 7;
    }
    out.push_back(int64_t(v));
  }
}

float as_f32(uint64_t v) {
  uint32_t w = uint32_t(v);
  float f;
  std::memcpy(&f, &w, 4);
  return f;
}

struct Tensor {
  std::string name;
  std::vector<int64_t> dims;
  std::vector<float> f;  // FLOAT data
  std::vector<int64_t> i; // INT64 data (Unsqueeze/Squeeze axes in opset 13+)
  int dtype = 0;
  // -1 for a negative dim or a product past int64 (never equal to a real element count)
  int64_t numel() const {
    int64_t n = 1;
    for (auto d : dims)
      if (d < 0 || __builtin_mul_overflow(n, d, &n)) return -1;
    return n;
  }
};

Tensor parse_tensor(Span s) {
  Tensor t;
  Span raw;
  bool has_raw = false;
  Reader r(s);
  Field f;
  while (r.next(f)) {
    switch (f.no) {
      case 1: packed_varints(f, t.dims); break;
      case 2: t.dtype = int(f.v); break;
      case 4:
        if (f.wt == 2) {
          size_t n = f.s.n / 4;
          size_t o = t.f.size();
          t.f.resize(o + n);
          if (n) std::memcpy(t.f.data() + o, f.s.p, n * 4);
        } else {
          t.f.push_back(as_f32(f.v));
        }
        break;
      case 7: packed_varints(f, t.i); break;
      case 8: t.name = str(f.s); break;
      case 9: raw = f.s; has_raw = true; break;
      default: break;
    }
  }
  if (has_raw) {
    if (t.dtype == 1) {
      if (raw.n % 4) fail("raw_data size of " + t.name);
      t.f.resize(raw.n / 4);
      if (raw.n) std::memcpy(t.f.data(), raw.p, raw.n);  // unaligned source
    } else if (t.dtype == 7) {
      if (raw.n % 8) fail("raw_data size of " + t.name);
      t.i.resize(raw.n / 8);
      if (raw.n) std::memcpy(t.i.data(), raw.p, raw.n);
    }
  }
  if (t.dtype == 1 && int64_t(t.f.size()) != t.numel()) fail("element count mismatch in " + t.name);
  return t;
}

struct Attr {
  float f = 0.f;
  int64_t i = 0;
  bool has_f = false, has_i = false, has_t = false;
  std::vector<int64_t> ints;
  std::vector<float> floats;
  Tensor t;  // AttributeProto.t (a Constant node's value)
};

struct Node {
  std::string op, name;
  std::vector<std::string> in, out;
  std::map<std::string, Attr> attrs;
  float fattr(const char *k, float d) const {
    auto it = attrs.find(k);
    return it == attrs.end() ? d : (it->second.has_f ? it->second.f : float(it->second.i));
  }
  int64_t iattr(const char *k, int64_t d) const {
    auto it = attrs.find(k);
    return it == attrs.end() ? d : (it->second.has_i ? it->second.i : int64_t(it->second.f));
  }
};

Node parse_node(Span s) {
  Node n;
  Reader r(s);
  Field f;
  while (r.next(f)) {
    switch (f.no) {
      case 1: n.in.push_back(str(f.s)); break;
      case 2: n.out.push_back(str(f.s)); break;
      case 3: n.name = str(f.s); break;
      case 4: n.op = str(f.s); break;
      case 5: {
        Attr a;
        std::string name;
        Reader ar(f.s);
        Field g;
        while (ar.next(g)) {
          if (g.no == 1) name = str(g.s);
          else if (g.no == 2) { a.f = as_f32(g.v); a.has_f = true; }
          else if (g.no == 3) { a.i = int64_t(g.v); a.has_i = true; }
          else if (g.no == 5 && g.wt == 2) { a.t = parse_tensor(g.s); a.has_t = true; }
          else if (g.no == 7) {
            if (g.wt == 2) {
              size_t k = g.s.n / 4, o = a.floats.size();
              a.floats.resize(o + k);
              if (k) std::memcpy(a.floats.data() + o, g.s.p, k * 4);
            } else a.floats.push_back(as_f32(g.v));
          } else if (g.no == 8) packed_varints(g, a.ints);
        }
        n.attrs[name] = a;
        break;
      }
      default: break;
    }
  }
  return n;
}

IoInfo parse_value_info(Span s) {
  IoInfo io;
  Reader r(s);
  Field f;
  while (r.next(f)) {
    if (f.no == 1) io.name = str(f.s);
    else if (f.no == 2) {
      Reader tr(f.s);
      Field t;
      while (tr.next(t)) {
        if (t.no != 1) continue;  // tensor_type
        Reader tt(t.s);
        Field u;
        while (tt.next(u)) {
          if (u.no != 2) continue;  // shape
          Reader sh(u.s);
          Field d;
          while (sh.next(d)) {
            if (d.no != 1) continue;
            int64_t val = -1;
            Reader dr(d.s);
            Field dv;
            while (dr.next(dv))
              if (dv.no == 1) val = int64_t(dv.v);
            io.shape.push_back(val);
          }
        }
      }
    }
  }
  return io;
}

// A model file as read: the nodes in file order, the initializers by name (Constant nodes
// among them), each value's consumers (node indices, in node order) and producer (the first
// in node order), and the graph inputs that are no initializers.
struct Graph {
  std::vector<Node> nodes;
  std::unordered_map<std::string, Tensor> inits;
  std::unordered_map<std::string, std::vector<size_t>> consumers;
  std::unordered_map<std::string, size_t> producers;
  std::vector<IoInfo> inputs, outputs;
};

// (the model's own fields, ir_version, producer_name and the opset, go straight into m)
Graph read_graph(const uint8_t *data, size_t n, Model &m) {
  if (!data || n == 0) fail("empty model");
  Graph g;
  Span graph;
  bool has_graph = false;
  {
    Reader r({data, n});
    Field f;
    while (r.next(f)) {
      if (f.no == 1) m.ir_version = int64_t(f.v);
      else if (f.no == 2) m.producer = str(f.s);
      else if (f.no == 7) { graph = f.s; has_graph = true; }
      else if (f.no == 8) {
        Reader o(f.s);
        Field h;
        while (o.next(h))
          if (h.no == 2 && int64_t(h.v) > m.opset) m.opset = int64_t(h.v);
      }
    }
  }
  if (!has_graph) fail("model has no graph");

  std::vector<IoInfo> raw_inputs;
  {
    Reader r(graph);
    Field f;
    while (r.next(f)) {
      if (f.no == 1) g.nodes.push_back(parse_node(f.s));
      else if (f.no == 5) {
        Tensor t = parse_tensor(f.s);
        g.inits[t.name] = std::move(t);
      } else if (f.no == 11) raw_inputs.push_back(parse_value_info(f.s));
      else if (f.no == 12) g.outputs.push_back(parse_value_info(f.s));
    }
  }
  // Constant nodes (torch.onnx.export writes scalars such as a Clip bound or a Mul
  // factor this way) become initializers of their output
  for (auto &nd : g.nodes) {
    if (nd.op != "Constant" || nd.out.empty()) continue;
    Tensor t;
    auto it = nd.attrs.find("value");
    if (it != nd.attrs.end() && it->second.has_t) t = it->second.t;
    else if ((it = nd.attrs.find("value_float")) != nd.attrs.end()) { t.dtype = 1; t.f = {it->second.f}; }
    else if ((it = nd.attrs.find("value_floats")) != nd.attrs.end()) {
      t.dtype = 1;
      t.f = it->second.floats;
      t.dims = {int64_t(t.f.size())};
    } else fail("Constant node '" + nd.name + "' without a value");
    t.name = nd.out[0];
    g.inits[t.name] = std::move(t);
  }
  for (auto &io : raw_inputs)
    if (!g.inits.count(io.name)) g.inputs.push_back(io);
  if (g.inputs.empty() || g.outputs.empty()) fail("graph needs at least one input and one output");

  for (size_t i = 0; i < g.nodes.size(); ++i)
    for (auto &in : g.nodes[i].in)
      if (!in.empty()) g.consumers[in].push_back(i);
  for (size_t i = 0; i < g.nodes.size(); ++i)
    for (auto &o : g.nodes[i].out)
      if (!o.empty()) g.producers.emplace(o, i);
  return g;
}

}  // namespace
}  // namespace go2pi
