// Host-only driver of the ONNX loader for tools/loader_diff.py: the same program built against
// two versions of csrc/onnx_model.cpp must print the same text for every file of a corpus.
//
//   loader_dump LIST          one line per path named in LIST (a text file, a path per line):
//                             "ok <hash> <inspect_json>" or "error <what>"
//   loader_dump --time N F    the median of N timed parse_onnx(F), in microseconds
//
// <hash> is FNV-1a (64 bit) over the bit patterns of every field of Model: inspect_json carries
// only sums of the weights, and a wrong skip-Concat column permutation leaves those unchanged.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "onnx_model.hpp"

namespace {

struct Fnv {
  uint64_t h = 1469598103934665603ull;
  void bytes(const void *p, size_t n) {
    const unsigned char *b = static_cast<const unsigned char *>(p);
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
  }
  template <class T> void pod(T v) { bytes(&v, sizeof v); }
  template <class T> void vec(const std::vector<T> &v) {  // (the length too: [a][bc] is not [ab][c])
    pod(uint64_t(v.size()));
    if (!v.empty()) bytes(v.data(), v.size() * sizeof(T));
  }
  void str(const std::string &s) {
    pod(uint64_t(s.size()));
    bytes(s.data(), s.size());
  }
  void io(const std::vector<go2pi::IoInfo> &v) {
    pod(uint64_t(v.size()));
    for (auto &i : v) {
      str(i.name);
      vec(i.shape);
    }
  }
};

uint64_t hash_of(const go2pi::Model &m) {
  Fnv f;
  f.io(m.inputs);
  f.io(m.outputs);
  f.pod(m.ir_version);
  f.pod(m.opset);
  f.str(m.producer);
  f.vec(m.pre_sub);
  f.vec(m.pre_div);
  f.vec(m.pre_mul);
  f.pod(m.pre_lo);
  f.pod(m.pre_hi);
  f.pod(int(m.has_gru));
  const go2pi::Gru &g = m.gru;
  for (int v : {g.cell, g.G, g.I, g.H, g.lbr}) f.pod(v);
  f.vec(g.W);
  f.vec(g.R);
  f.vec(g.Wb);
  f.vec(g.Rb);
  f.pod(uint64_t(m.layers.size()));
  for (auto &d : m.layers) {
    for (int v : {d.K, d.N, d.act, d.ln, d.res}) f.pod(v);
    for (float v : {d.alpha, d.beta, d.ln_eps}) f.pod(v);
    f.vec(d.W);
    f.vec(d.b);
    f.vec(d.ln_g);
    f.vec(d.ln_b);
    f.vec(d.skip);
  }
  f.pod(m.clip_lo);
  f.pod(m.clip_hi);
  f.pod(m.post_scale);
  f.pod(m.in_dim);
  f.pod(m.out_dim);
  return f.h;
}

std::vector<uint8_t> read_file(const std::string &path) {
  std::ifstream f(path, std::ios::binary);
  return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

}  // namespace

int main(int argc, char **argv) {
  if (argc == 4 && !std::strcmp(argv[1], "--time")) {
    const std::vector<uint8_t> bytes = read_file(argv[3]);
    std::vector<double> us;
    for (int i = 0, n = std::atoi(argv[2]); i < n; ++i) {
      const auto t0 = std::chrono::steady_clock::now();
      const go2pi::Model m = go2pi::parse_onnx(bytes.data(), bytes.size());
      us.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() +
                   0.0 * m.in_dim);
    }
    if (us.empty()) return 2;
    std::sort(us.begin(), us.end());
    std::printf("%.1f\n", us[us.size() / 2]);
    return 0;
  }
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s LIST | --time N FILE\n", argv[0]);
    return 2;
  }
  std::ifstream list(argv[1]);
  for (std::string path; std::getline(list, path);) {
    const std::vector<uint8_t> bytes = read_file(path);
    std::string line;
    try {
      const go2pi::Model m = go2pi::parse_onnx(bytes.data(), bytes.size());
      char h[24];
      std::snprintf(h, sizeof h, "%016llx", (unsigned long long)hash_of(m));
      line = std::string("ok ") + h + " " + go2pi::inspect_json(m);
    } catch (const std::exception &ex) {
      line = std::string("error ") + ex.what();
    }
    for (char &c : line)  // (names from the file: one line per file whatever they hold)
      if (c == '\n' || c == '\r') c = '?';
    std::printf("%s\n", line.c_str());
  }
  return 0;
}
