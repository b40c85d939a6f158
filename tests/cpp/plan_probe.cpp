// The engine's plan for a model, without a device: parse, plan (csrc/plan.hpp) and print
// one JSON object with the kernels the engine would report and the plan's scalars.
//
//   plan_probe MODEL [key=value ...] [GO2PI_SWITCH[=value] ...] [ring=vram|host]
//
// key: a go2pi_opts field (waves, small_batch, resident_ms, ln_small, action_tanh,
// obs_clip, action_clip, action_scale, use_graph; obs_mean / obs_std: one value for every
// feature). A GO2PI_* argument is put into the environment and read by Switches::read(),
// as an engine reads it. ring: where the resident request ring ended up (default vram).
// A refusal prints {"error": ..., "code": ...} and exits 1. tests/test_cpu_plan.py runs it.
// "lds": the dynamic-LDS layout (csrc/lds_layout.hpp) of every small-batch launcher the
// plan uses, as its launcher sizes it: regions [name, offset, size] in floats, total_bytes,
// and the arguments it was made from (tests/test_cpu_lds_layout.py).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "plan.hpp"

namespace {

// FNV-1a over the floats' bytes: position-sensitive, so a pack in another order differs
uint64_t fnv(const std::vector<float> &v) {
  uint64_t h = 0xcbf29ce484222325ull;
  const unsigned char *b = reinterpret_cast<const unsigned char *>(v.data());
  for (size_t i = 0; i < v.size() * sizeof(float); ++i) h = (h ^ b[i]) * 0x100000001b3ull;
  return h;
}

// one layout as {"regions": [[name, offset, size], ...], "total_bytes": n, <args>}
struct Regions {
  std::string out;
  void add(const char *name, go2pi::lds::Span s, int base = 0) {
    out += (out.empty() ? "[\"" : ", [\"") + std::string(name) + "\", " + std::to_string(base + s.off) + ", " +
           std::to_string(s.size) + "]";
  }
  void image(int in_dim, go2pi::lds::Span at) {  // the controller image's regions in place of `at`
    const go2pi::CtlImage I = go2pi::ctl_image(GO2PI_SMALL_MAXB, in_dim);
    if (at.size == 0) return;
    add("image.q0", I.q0, at.off), add("image.st", I.st, at.off), add("image.jy", I.jy, at.off);
    add("image.act", I.act, at.off), add("image.obs", I.obs, at.off), add("image.nanf", I.nanf, at.off);
  }
  void print(const char *key, int total, const std::string &args = "") const {
    std::printf("  \"%s\": {\"regions\": [%s], \"total_bytes\": %zu%s}", key, out.c_str(), sizeof(float) * (size_t)total,
                args.c_str());
  }
};

void print_latency(const char *key, const go2pi::DevProgram &p, bool ctl) {
  const go2pi::LatencyLds L = go2pi::latency_lds_of(p, ctl);
  Regions r;
  r.add("xs", L.xs), r.add("part", L.part), r.add("flag", L.flag);
  if (ctl) {
    const go2pi::LatencyCtlLds C = go2pi::latency_ctl_lds(p.in_dim);
    r.add("okeep", C.okeep, L.ctl.off), r.image(p.in_dim, {L.ctl.off + C.image.off, C.image.size});
    r.add("slack", C.slack, L.ctl.off);
  }
  r.print(key, L.total);
}

void print_resident(const char *key, go2pi::ResForm form, const go2pi::DevProgram &p, bool ctl, bool tiled0) {
  Regions r;
  char args[160] = "";
  int total = 0;
  if (form == go2pi::ResForm::Act1) {
    const go2pi::Act1Lds L = go2pi::act1_lds_of(p, ctl);
    r.add("x0", L.x0), r.add("xa", L.xa), r.add("xb", L.xb), r.add("st", L.st), r.image(p.in_dim, L.image);
    r.add("w0l", L.w0l), r.add("wol", L.wol), r.add("obsn", L.obsn);
    std::snprintf(args, sizeof args, ", \"form\": \"act1\", \"h\": %d, \"nl\": %d, \"f0\": %d", L.h, L.nl, L.f0);
    total = L.total;
  } else if (form == go2pi::ResForm::R1) {
    const go2pi::R1Lds L = go2pi::r1_lds_of(p, ctl);
    r.add("x0", L.x0), r.add("xa", L.xa), r.add("xb", L.xb), r.add("st", L.st), r.add("obsv", L.obsv);
    r.image(p.in_dim, L.image), r.add("craw", L.craw);
    std::snprintf(args, sizeof args, ", \"form\": \"r1\"");
    total = L.total;
  } else if (form == go2pi::ResForm::Wide) {
    const go2pi::WideLds L = go2pi::wide_lds_of(p);
    const go2pi::WideShape w = go2pi::wide_shape(p);
    r.add("x0", L.x0), r.add("h0", L.h0), r.add("hh", L.hh), r.add("ho", L.ho), r.add("pp", L.pp), r.add("st", L.st);
    std::snprintf(args, sizeof args, ", \"form\": \"wide\", \"cw\": %d, \"f0\": %d", w.cw, w.f0);
    total = L.total;
  } else {
    const go2pi::MultiLds L = go2pi::multi_lds_of(p, ctl, tiled0);
    r.add("xs", L.xs), r.add("part", L.part), r.add("st", L.st), r.add("obsv", L.obsv), r.add("x0", L.x0);
    r.add("p0", L.p0), r.image(p.in_dim, L.image), r.add("craw", L.craw);
    if (p.has_gru) {
      const go2pi::CellLds C = go2pi::cell_lds(p.gru.I_pad, p.gru.H);
      r.add("hx", C.hx, L.cell.off), r.add("hpart", C.hpart, L.cell.off), r.add("le", C.le, L.cell.off);
      r.add("lb", C.lb, L.cell.off), r.add("hown", C.hown, L.cell.off), r.add("cown", C.cown, L.cell.off);
      r.add("hst", C.hst, L.cell.off), r.add("cst", C.cst, L.cell.off);
    }
    std::snprintf(args, sizeof args, ", \"form\": \"multi\", \"nf\": %d, \"tiled0\": %d", L.nf, (int)tiled0);
    total = L.total;
  }
  r.print(key, total, args);
}

void print_lds(const go2pi::DevProgram &p, const go2pi::ResForms &res, bool latency_ok, bool tiled0) {
  std::printf(" \"lds\": {\"lds_stride\": %d, \"in_dim\": %d, \"nl\": %d, \"k0_pad\": %d, \"n0_pad\": %d, \"ln\": %d, "
              "\"rnn\": %d, \"i_pad\": %d, \"gru_h\": %d,\n  \"gemv\": [",
              p.lds_stride, p.in_dim, p.nl, p.L[0].K_pad, p.L[0].N_pad, (int)go2pi::program_has_ln(p), p.has_gru,
              p.has_gru ? p.gru.I_pad : 0, p.has_gru ? p.gru.H : 0);
  for (int l = 0; l < p.nl; ++l) {
    const go2pi::GemvLds L = go2pi::gemv_lds_of(p, l);
    Regions r;
    r.add("xs", L.xs), r.add("part", L.part);
    std::printf("%s{\"k_pad\": %d, \"regions\": [%s], \"total_bytes\": %zu}", l ? ", " : "", p.L[l].K_pad, r.out.c_str(),
                sizeof(float) * (size_t)L.total);
  }
  std::printf("]");
  if (latency_ok) {
    std::printf(",\n"), print_latency("latency", p, false);
    std::printf(",\n"), print_latency("latency_ctl", p, true);
  }
  if (res.act != go2pi::ResForm::None) std::printf(",\n"), print_resident("act", res.act, p, false, tiled0);
  if (res.ctl != go2pi::ResForm::None) std::printf(",\n"), print_resident("ctl", res.ctl, p, true, tiled0);
  std::printf("},\n");
}

int run(int argc, char **argv) {
  go2pi_opts o;
  go2pi_default_opts(&o);
  std::vector<float> mean, stdv;
  bool ring_vram = true;
  std::ifstream f(argv[1], std::ios::binary);
  if (!f) throw go2pi::ApiError(std::string("cannot open model file '") + argv[1] + "'", GO2PI_E_MODEL);
  const std::vector<uint8_t> bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  go2pi::Model m;
  try {
    m = go2pi::parse_onnx(bytes.data(), bytes.size());
  } catch (const std::exception &ex) {
    throw go2pi::ApiError(ex.what(), GO2PI_E_MODEL);
  }
  go2pi::check_model(m);
  for (int i = 2; i < argc; ++i) {
    const std::string a = argv[i];
    const size_t eq = a.find('=');
    const std::string k = a.substr(0, eq), v = eq == std::string::npos ? "1" : a.substr(eq + 1);
    if (k.rfind("GO2PI_", 0) == 0) setenv(k.c_str(), v.c_str(), 1);
    else if (k == "ring") ring_vram = v != "host";
    else if (k == "waves") o.waves = std::atoi(v.c_str());
    else if (k == "small_batch") o.small_batch = std::atoi(v.c_str());
    else if (k == "resident_ms") o.resident_ms = std::atoi(v.c_str());
    else if (k == "ln_small") o.ln_small = std::atoi(v.c_str());
    else if (k == "use_graph") o.use_graph = std::atoi(v.c_str());
    else if (k == "action_tanh") o.action_tanh = std::atoi(v.c_str());
    else if (k == "obs_clip") o.obs_clip = std::strtof(v.c_str(), nullptr);
    else if (k == "action_clip") o.action_clip = std::strtof(v.c_str(), nullptr);
    else if (k == "action_scale") o.action_scale = std::strtof(v.c_str(), nullptr);
    else if (k == "obs_mean") mean.assign(m.in_dim, std::strtof(v.c_str(), nullptr)), o.obs_mean = mean.data();
    else if (k == "obs_std") stdv.assign(m.in_dim, std::strtof(v.c_str(), nullptr)), o.obs_std = stdv.data();
    else throw go2pi::ApiError("plan_probe: unknown argument '" + a + "'", GO2PI_E_INVALID);
  }
  const go2pi::Switches sw = go2pi::Switches::read();
  go2pi::Plan pl = go2pi::plan_program(m, o, sw);
  const bool resident_ok = pl.resident(o);
  const bool vram = resident_ok && ring_vram && !sw.req_host;  // (REQ_HOST: bar_take hands out no device block)
  const go2pi::ResForms res = go2pi::plan_resident(pl, sw, resident_ok, vram);
  go2pi::DevProgram &p = pl.prog;
  // (the wide kernel's name says whether the policy has an observation prologue, which the
  // launcher reads from these pointers; never dereferenced here)
  p.pre_sub = pl.buf.pre_sub.empty() ? nullptr : pl.buf.pre_sub.data();
  p.pre_div = pl.buf.pre_div.empty() ? nullptr : pl.buf.pre_div.data();
  p.pre_mul = pl.buf.pre_mul.empty() ? nullptr : pl.buf.pre_mul.data();
  char batched[128], small[128], ract[128], rctl[128];
  go2pi::batched_kernel_name(p, pl.waves, batched, sizeof batched);
  go2pi::small_kernel_name(p, pl.waves, pl.small_batch, pl.latency_ok, o.use_graph != 0, small, sizeof small);
  go2pi::resident_kernel_name(res.act, p, vram, ract, sizeof ract);
  go2pi::resident_kernel_name(res.ctl, p, vram, rctl, sizeof rctl);
  std::printf("{\"batched_kernel\": \"%s\", \"small_kernel\": \"%s\", \"resident_kernel\": \"%s\", "
              "\"controller_kernel\": \"%s\",\n",
              batched, small, ract, rctl);
  std::printf(" \"waves\": %d, \"w4_tpw\": %d, \"head_fuse\": %d, \"w4_c0m\": %d, \"w4_plain\": %d, \"w4_actc\": %d, "
              "\"w4_nhc\": %d, \"w4_gru_lean\": %d, \"lds_stride\": %d, \"in_pad\": %d, \"zero_fill\": %d,\n",
              pl.waves, p.w4_tpw, p.head_fuse, p.w4_c0m, p.w4_plain, p.w4_actc, p.w4_nhc, p.w4_gru_lean, p.lds_stride,
              p.in_pad, p.zero_fill);
  std::printf(" \"latency_ok\": %d, \"one_round\": %d, \"done_ok\": %d, \"ctl_hist\": %d, \"small_batch\": %d,\n",
              (int)pl.latency_ok, (int)pl.one_round, (int)pl.done_ok, pl.ctl_hist, pl.small_batch);
  std::printf(" \"cost\": {\"flops_per_row\": %.17g, \"weight_bytes\": %.17g, \"io_bytes_per_row\": %.17g, "
              "\"n_layers\": %d, \"has_gru\": %d},\n",
              pl.cost.flops_per_row, pl.cost.weight_bytes, pl.cost.io_bytes_per_row, (int)pl.cost.n_layers,
              (int)pl.cost.has_gru);
  std::printf(" \"bpack\": {\"len\": %zu, \"fnv\": \"%016llx\"}, \"bias\": [", pl.buf.bpack.size(),
              (unsigned long long)fnv(pl.buf.bpack));
  for (int l = 0; l < p.nl; ++l)
    std::printf("%s{\"len\": %zu, \"fnv\": \"%016llx\"}", l ? ", " : "", pl.buf.bias[l].size(),
                (unsigned long long)fnv(pl.buf.bias[l]));
  std::printf("],\n");
  print_lds(p, res, pl.latency_ok, sw.res_tiled0);
  // the recurrent cell's fragments and gate biases (empty without a cell)
  std::printf(" \"gru_w\": {\"len\": %zu, \"fnv\": \"%016llx\"}, \"gru_bzr\": {\"len\": %zu, \"fnv\": \"%016llx\"}, "
              "\"gru_bh\": {\"len\": %zu, \"fnv\": \"%016llx\"}}\n",
              pl.buf.gru_w.size(), (unsigned long long)fnv(pl.buf.gru_w), pl.buf.gru_bzr.size(),
              (unsigned long long)fnv(pl.buf.gru_bzr), pl.buf.gru_bh.size(), (unsigned long long)fnv(pl.buf.gru_bh));
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: plan_probe MODEL [key=value ...] [GO2PI_SWITCH ...] [ring=vram|host]\n");
    return 2;
  }
  try {
    return run(argc, argv);
  } catch (const go2pi::ApiError &ex) {
    std::string msg;
    for (const char *c = ex.what(); *c; ++c) msg += (*c == '"' || *c == '\\') ? std::string("\\") + *c : std::string(1, *c);
    std::printf("{\"error\": \"%s\", \"code\": %d}\n", msg.c_str(), ex.code);
    return 1;
  }
}
