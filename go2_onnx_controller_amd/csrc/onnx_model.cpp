// ONNX policy loader (see onnx_model.hpp): one compiled unit over four internal headers, each
// including the one before it:
//   onnx_proto.hpp      the protobuf reader: the file's bytes -> Graph
//   onnx_graph.hpp      GraphView: the queries on a Graph, each written once
//   onnx_front_end.hpp  the per-block observation front-end -> Model's prologue
//   onnx_walker.hpp     Walker: the main chain, one handler per operator -> Model's program
#include "onnx_model.hpp"

#include <cstdio>

#include "onnx_walker.hpp"

namespace go2pi {

Model parse_onnx(const uint8_t *data, size_t n) {
  Model m;
  const GraphView g{read_graph(data, n, m)};
  m.inputs = g.inputs;
  m.outputs = g.outputs;
  Walker(g, m).run();
  return m;
}

namespace {

std::string json_num(double v) {
  if (std::isnan(v)) return "null";
  if (std::isinf(v)) return v > 0 ? "1e308" : "-1e308";
  char t[64];
  std::snprintf(t, sizeof t, "%.17g", v);
  return t;
}

// a JSON string literal (names come from the file: quotes, backslashes and control bytes escaped)
std::string json_str(const std::string &s) {
  std::string o = "\"";
  for (unsigned char c : s) {
    if (c == '"' || c == '\\') {
      o += '\\';
      o += (char)c;
    } else if (c < 0x20 || c >= 0x7F) {
      char t[8];
      std::snprintf(t, sizeof t, "\\u%04x", c);
      o += t;
    } else {
      o += (char)c;
    }
  }
  return o + "\"";
}

double sum_of(const std::vector<float> &v) {
  double s = 0;
  for (float x : v) s += x;
  return s;
}

std::string io_json(const std::vector<IoInfo> &v) {
  std::string s = "[";
  for (size_t i = 0; i < v.size(); ++i) {
    s += (i ? "," : "") + std::string("{\"name\":") + json_str(v[i].name) + ",\"shape\":[";
    for (size_t d = 0; d < v[i].shape.size(); ++d) s += (d ? "," : "") + std::to_string(v[i].shape[d]);
    s += "]}";
  }
  return s + "]";
}

}  // namespace

std::string inspect_json(const Model &m) {
  std::string j = "{\"ir_version\":" + std::to_string(m.ir_version) + ",\"opset\":" + std::to_string(m.opset) +
                  ",\"producer\":" + json_str(m.producer) + ",\"inputs\":" + io_json(m.inputs) +
                  ",\"outputs\":" + io_json(m.outputs) + ",\"in_dim\":" + std::to_string(m.in_dim) +
                  ",\"out_dim\":" + std::to_string(m.out_dim) + ",\"layers\":[";
  for (size_t l = 0; l < m.layers.size(); ++l) {
    const auto &d = m.layers[l];
    j += (l ? "," : "") + std::string("{\"K\":") + std::to_string(d.K) + ",\"N\":" + std::to_string(d.N) +
         ",\"act\":" + std::to_string(d.act) + ",\"alpha\":" + json_num(d.alpha) + ",\"beta\":" + json_num(d.beta) +
         ",\"w_sum\":" + json_num(sum_of(d.W)) + ",\"b_sum\":" + json_num(sum_of(d.b)) +
         ",\"ln\":" + std::to_string(d.ln) + ",\"ln_eps\":" + json_num(d.ln_eps) +
         ",\"ln_g_sum\":" + json_num(sum_of(d.ln_g)) + ",\"ln_b_sum\":" + json_num(sum_of(d.ln_b)) + ",\"skip\":[";
    for (size_t i = 0; i < d.skip.size(); ++i) j += (i ? "," : "") + std::to_string(d.skip[i]);
    j += "],\"res\":" + std::to_string(d.res) + "}";
  }
  j += "],\"gru\":";
  if (m.has_gru)
    j += "{\"cell\":\"" + std::string(m.gru.cell ? "LSTM" : "GRU") + "\",\"I\":" + std::to_string(m.gru.I) +
         ",\"H\":" + std::to_string(m.gru.H) + ",\"lbr\":" + std::to_string(m.gru.lbr) +
         ",\"w_sum\":" + json_num(sum_of(m.gru.W)) + ",\"r_sum\":" + json_num(sum_of(m.gru.R)) +
         ",\"b_sum\":" + json_num(sum_of(m.gru.Wb) + sum_of(m.gru.Rb)) + "}";
  else
    j += "null";
  j += ",\"pre_sub\":" + std::to_string(m.pre_sub.size()) + ",\"pre_div\":" + std::to_string(m.pre_div.size()) +
       ",\"pre_mul\":" + std::to_string(m.pre_mul.size()) + ",\"pre_clip\":[" + json_num(m.pre_lo) + "," +
       json_num(m.pre_hi) + "],\"clip\":[" + json_num(m.clip_lo) + "," + json_num(m.clip_hi) +
       "],\"post_scale\":" + json_num(m.post_scale) + "}";
  return j;
}

}  // namespace go2pi
