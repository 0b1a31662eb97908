// host_runtime_driver.cpp - the device-facing host code of libseigen_hip (api.cpp, stages.cpp, transfer.cpp, comm.cpp,
// devxfer.cpp, frame.cpp and the host halves of kernels*.hip) on the CPU, under ASan and UBSan, over the HIP runtime double of
// tests/fake_hip (`make -C seigen_amd/csrc host-runtime-asan`; tests/test_host_runtime.py).  Nothing runs on a device and no
// kernel runs at all: the double logs every launch with its argument bytes and audits the device pointers among them.  One
// program of three suites over host_runtime_common.hpp: this file's, per block (a) - (d) and once (e), and those of the
// device transfers (host_runtime_xfer.cpp) and the frames (host_runtime_frame.cpp) on blocks of their own.  Per block:
//   (a) a whole life of a handle - every setter twice, stepping by graph replay and eagerly, host-driven stages, transfers,
//       destroy - with the audit and the sanitizers silent and nothing of the runtime left alive;
//   (b) the launches of that life under graph replay equal to those with SEIGEN_HIP_GRAPH=0, but for the members of kMask;
//   (c) a failure injected into every runtime call of every entry point: the error code, the message, nothing leaked,
//       the handle as it was, and the next steps launching what a twin launches that never saw the failure;
//   (d) sizes that cannot be met;
//   (e) the kernel objects the program registered, printed for the wrapper to compare with the tests' lists.
// usage: host_runtime_driver [block | xfer | frames | kernels | blocks ...]   (no argument: every block and both suites; (e)
// comes first in every run, and alone with `kernels`; `blocks`: the names of kBlocks, one per line, and nothing else)
#include <map>
#include <set>
#include <sstream>

#include "host_runtime_common.hpp"

namespace {

// ---- the blocks: the smallest of each kernel family -----------------------------------------------------------------

const BlockDef kBlocks[] = {
    {"mfma-P4-f64", nullptr, 3, 4, {3, 2, 2}, 0, 0, 0, true, Family::Mfma},
    {"mfma-P2-f32", nullptr, 3, 2, {17, 1, 2}, 0, 1, 0, true, Family::Mfma},
    {"tile-tri-P3", nullptr, 2, 3, {5, 3, 1}, 0, 0, 0, true, Family::Tile2d},
    {"tile-quad-DQ2", nullptr, 2, 2, {5, 3, 1}, 2, 0, 0, true, Family::Tile2d},
    {"hexm-DQ3", nullptr, 3, 3, {3, 2, 2}, 2, 0, 0, true, Family::Hexm},
    {"lane-2d-P2", "lane", 2, 2, {5, 3, 1}, 0, 0, 0, false, Family::Lane},
    {"generic-1d-P2", nullptr, 1, 2, {37, 1, 1}, 0, 0, 0, true, Family::Generic},
    {"mfma-P3-nbr", nullptr, 3, 3, {3, 2, 2}, 0, 0, (1 << 1) | (1 << 2), true, Family::Mfma},
};

uint64_t g_seed = 1;
double rnd() {   // in (0.5, 1.5)
  g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull;
  return 0.5 + (double)(g_seed >> 11) / (double)(1ull << 53);
}
std::vector<double> rnds(size_t n, double scale = 1.0) {
  std::vector<double> v(n);
  for (double& x : v) x = scale * rnd();
  return v;
}

// ---- what the script hands the setters (v = 0, 1: two sets of values) -----------------------------------------------

int nodes_of(int dim, int degree, bool tensor) {
  if (tensor) return dim == 2 ? (degree + 1) * (degree + 1) : (degree + 1) * (degree + 1) * (degree + 1);
  int n = 1;
  for (int k = 1; k <= dim; ++k) n = n * (degree + k) / k;
  return n;
}

int set_material(Ctx& c, int v) {
  const std::vector<double> lam = rnds((size_t)c.ncells, 2.0 + v), mu = rnds((size_t)c.ncells, 1.0 + v);
  return sg_set_params(c.h, 1.0 + 0.5 * v, 1e-3, lam.data(), mu.data(), 1);
}
int set_density(Ctx& c, int v) {
  const std::vector<double> rho = rnds((size_t)c.ncells, 1.0 + v);
  return sg_set_density(c.h, rho.data(), 1, v);
}
// DG4 nodal sigma with cells of four kinds by cell % 4 (tests/test_mfma_family_gpu.py _sponge): none, one value, general
// nodal, affine in x
int set_sponge(Ctx& c, int v) {
  const int q = 4, nq = nodes_of(c.dim, q, c.b->diagonal == 2);
  std::vector<double> X((size_t)c.ncells * nq * c.dim), sigma((size_t)c.ncells * nq, 0.0);
  if (int rc = sg_node_coords(c.h, q, X.data(), X.size() * sizeof(double))) return rc;
  for (int64_t e = 0; e < c.ncells; ++e) {
    const int kind = (int)((e + v) % 4);
    const double s0 = 10.0 * rnd(), g[3] = {4.0 * rnd(), -3.0 * rnd(), 2.0 * rnd()};
    for (int a = 0; a < nq; ++a) {
      double& s = sigma[(size_t)e * nq + a];
      if (kind == 1) s = s0;
      if (kind == 2) s = 20.0 * rnd();
      if (kind == 3) {
        s = 30.0 + s0;
        for (int k = 0; k < c.dim; ++k) s += g[k] * (X[((size_t)e * nq + a) * c.dim + k] - X[(size_t)e * nq * c.dim + k]);
      }
    }
  }
  return sg_set_absorption(c.h, sigma.data(), q);
}
constexpr int64_t kSeries = 64;   // steps every series of the script covers: more than the script ever takes
std::vector<int64_t> source_nodes(const Ctx& c) { return {0, 5, c.ncells * c.nd - 1, c.ncells * c.nd / 2, 5}; }
std::vector<double> tensors(const Ctx& c, size_t count, bool symmetric) {
  const int d = c.dim;
  std::vector<double> t = rnds(count * d * d);
  for (size_t k = 0; k < count && symmetric; ++k)
    for (int i = 0; i < d; ++i)
      for (int j = 0; j < i; ++j) t[(k * d + i) * d + j] = t[(k * d + j) * d + i];
  return t;
}
int set_source_table(Ctx& c, bool symmetric) {
  const std::vector<int64_t> nodes = source_nodes(c);
  const std::vector<double> vals = tensors(c, (size_t)kSeries * nodes.size(), symmetric);
  return sg_set_source(c.h, (int64_t)nodes.size(), nodes.data(), kSeries, vals.data());
}
int set_source_separable(Ctx& c, bool symmetric) {
  const std::vector<int64_t> nodes = source_nodes(c);
  const std::vector<double> pat = tensors(c, nodes.size(), symmetric), w = rnds((size_t)kSeries);
  return sg_set_source_separable(c.h, (int64_t)nodes.size(), nodes.data(), pat.data(), kSeries, w.data());
}
int set_source_box(Ctx& c) {
  const double lo[3] = {0.2, 0.0, 0.0}, hi[3] = {0.8, 0.6, 0.6};
  return sg_set_source_box_ricker(c.h, lo, hi, 100.0, 0.05, 1e-3, 1e-3, kSeries);
}
// three points: in the first cube, in the last one, outside the mesh
std::vector<double> points(const Ctx& c) {
  std::vector<double> p;
  for (int k = 0; k < 3; ++k)
    for (int a = 0; a < c.dim; ++a) p.push_back(k == 0 ? 0.11 + 0.07 * a : (k == 1 ? 0.5 * c.b->n[a] - 0.13 - 0.05 * a : -3.0));
  return p;
}
constexpr int64_t kRecEvery = 2, kRecCap = 32, kMonCap = 64;
int set_receivers(Ctx& c, int v) {
  const std::vector<double> p = points(c);
  int32_t owned[3];
  return sg_set_receivers(c.h, 3, p.data(), v ? 1 : 3, kRecEvery, kRecCap, owned);
}
int set_monitor(Ctx& c, int v) {
  const std::vector<double> w = rnds((size_t)c.ncells * 3);
  return sg_set_monitor(c.h, 1, kMonCap, w.data(), v ? 0 : 1);
}
int set_spectra(Ctx& c, int v) {
  const int nfreq = 2 + v;
  const std::vector<double> wu = rnds((size_t)kSeries * nfreq * 2), ws = rnds((size_t)kSeries * nfreq * 2);
  return sg_set_spectra(c.h, nfreq, 3, 1, kSeries, wu.data(), ws.data());
}
std::vector<double> injector_amps(const Ctx& c, int64_t nsteps, bool symmetric) {
  const int d = c.dim, ncomp = d + d * d;
  std::vector<double> amp = rnds((size_t)nsteps * 3 * ncomp);
  for (size_t k = 0; k < (size_t)nsteps * 3 && symmetric; ++k)
    for (int i = 0; i < d; ++i)
      for (int j = 0; j < i; ++j) amp[k * ncomp + d + i * d + j] = amp[k * ncomp + d + j * d + i];
  return amp;
}
int set_injectors(Ctx& c, bool symmetric) {
  const std::vector<double> p = points(c), amp = injector_amps(c, kSeries, symmetric);
  int32_t owned[3];
  return sg_set_injectors(c.h, 3, p.data(), 3, kSeries, amp.data(), owned);
}
int inject_once(Ctx& c, bool symmetric) {
  const std::vector<double> p = points(c), amp = injector_amps(c, 1, symmetric);
  return sg_inject(c.h, 3, p.data(), 3, amp.data());
}

// n LF4 steps: sg_step, or - a block with neighbours and no communicator - the host's own FIRST / SECOND launches with the
// packs between them and sg_end_step
int host_step(Ctx& c) {
  const bool nbr = c.b->nbr_mask != 0;
  for (int st = 0; st < 6; ++st) {
    if (int rc = sg_run_stage(c.h, st, nbr ? SG_REGION_FIRST : SG_REGION_ALL)) return rc;
    if (!nbr) continue;
    if (int rc = sg_run_stage(c.h, st, SG_REGION_SECOND)) return rc;
  }
  return sg_end_step(c.h);
}
int steps(Ctx& c, int64_t n) {
  if (c.b->nbr_mask == 0) return sg_step(c.h, n);
  for (int64_t k = 0; k < n; ++k)
    if (int rc = host_step(c)) return rc;
  return SG_OK;
}

// every setter of the script, in its order
int configure(Ctx& c, int v) {
  if (int rc = set_material(c, v)) return rc;
  if (int rc = set_density(c, v)) return rc;
  if (int rc = set_sponge(c, v)) return rc;
  if (int rc = set_source_table(c, true)) return rc;
  if (int rc = set_source_separable(c, true)) return rc;
  if (int rc = set_receivers(c, v)) return rc;
  if (int rc = set_monitor(c, v)) return rc;
  if (int rc = set_spectra(c, v)) return rc;
  return set_injectors(c, true);
}

// ---- logs compared: pointers by the order their allocations appear in, masked members left out --------------------------

// Argument members that legitimately differ between a captured launch and an eager one, member by member.  A captured launch
// takes the step from a device-side counter, an eager one is handed it by the host:
struct MaskEntry {
  const char* kernel;   // prefix of the kernel's name ("": any)
  const char* type;     // the parameter's type, or null: parameter `index`
  int index;
  size_t at, size;      // the member inside the parameter (size 0: the whole parameter)
  const char* why;
};
#define MEMBER(T, m) offsetof(T, m), sizeof(((T*)nullptr)->m)
const MaskEntry kMask[] = {
    // the fused source of the 2-D tile family: slice, weight and stepper of the step
    {"", "sg::StageArgs", -1, MEMBER(StageArgs, src_vals), "stages.cpp:101 a.src_vals = sn.values: the host's slice against slice 0 and SrcStep::ctr"},
    {"", "sg::StageArgs", -1, MEMBER(StageArgs, src_scale), "stages.cpp:102 a.src_scale = sn.at.scale: the host's weight against SrcStep::weights"},
    {"", "sg::StageArgs", -1, MEMBER(StageArgs, src_step), "stages.cpp:95,103 a.src_step = sn.stepper: null under eager launches (stages.cpp:32-39)"},
    {"", "sg::StageArgs", -1, MEMBER(StageArgs, src_bump), "stages.cpp:96 a.src_bump = 1: the capture's UH1 bumps the counter"},
    // the source launch of the other families (launch_source's values, scale and SrcStep)
    {"void sg::source_kernel<", nullptr, 5, 0, 0, "stages.cpp:251 sn.values + off: the host's slice against slice 0"},
    {"void sg::source_kernel<", nullptr, 7, 0, 0, "stages.cpp:251 sn.at.scale: the host's weight against SrcStep::weights"},
    {"void sg::source_kernel<", nullptr, 8, 0, 0, "stages.cpp:252 sn.stepper: null under eager launches"},
    // the end-of-step hooks: the step by value against the hook's device counter (stages.cpp:550 hook_step)
    {"", "sg::RecvArgs", -1, MEMBER(RecvArgs, ctr), "stages.cpp:418 a.ctr"},
    {"", "sg::RecvArgs", -1, MEMBER(RecvArgs, step), "stages.cpp:419 a.step"},
    {"", "sg::measure::Args", -1, MEMBER(measure::Args, ctr), "stages.cpp:445 a.ctr"},
    {"", "sg::measure::Args", -1, MEMBER(measure::Args, step), "stages.cpp:446 a.step"},
    {"", "sg::spectra::Args", -1, MEMBER(spectra::Args, ctr), "stages.cpp:495 a.ctr"},
    {"", "sg::spectra::Args", -1, MEMBER(spectra::Args, step), "stages.cpp:496 a.step"},
    {"", "sg::inject::Args", -1, MEMBER(inject::Args, ctr), "stages.cpp:327 a.ctr"},
    {"", "sg::inject::Args", -1, MEMBER(inject::Args, step), "stages.cpp:328 a.step"},
};
// ... and the one-thread launches that set and bump those counters exist under replay only (stages.cpp:551, :609, :675, :679)
const char* const kReplayOnlyKernel = "sg::step_counter_kernel(";

bool masked(const FakeHipLaunch& e, size_t byte) {
  for (const MaskEntry& m : kMask) {
    if (e.name.compare(0, std::strlen(m.kernel), m.kernel) != 0) continue;
    for (size_t i = 0; i < e.params.size(); ++i) {
      const FakeHipParam& p = e.params[i];
      if (m.type ? p.type != m.type : (int)i != m.index) continue;
      const size_t lo = p.at + m.at, hi = lo + (m.size ? m.size : p.size);
      if (byte >= lo && byte < hi) return true;
    }
  }
  return false;
}

// one line per launch; `from`: the first entry of the log to take
std::vector<std::string> canon(size_t from, bool mask) {
  const std::vector<FakeHipLaunch>& log = fakehip_log();
  std::map<long, int> alloc_ix;
  std::map<void*, int> stream_ix;
  std::vector<std::string> out;
  for (size_t n = from; n < log.size(); ++n) {
    const FakeHipLaunch& e = log[n];
    if (mask && e.name.find(kReplayOnlyKernel) != std::string::npos) continue;
    std::ostringstream s;
    if (!stream_ix.count(e.stream)) stream_ix.emplace(e.stream, (int)stream_ix.size());
    s << e.name << " grid " << e.grid[0] << "," << e.grid[1] << "," << e.grid[2] << " block " << e.block[0] << "," << e.block[1] << ","
      << e.block[2] << " lds " << e.lds << " stream " << stream_ix[e.stream] << " args";
    std::vector<unsigned char> bytes = e.args;
    std::vector<char> skip(bytes.size(), 0);
    for (size_t i = 0; i < bytes.size(); ++i)
      if (mask && masked(e, i)) skip[i] = 1;
    std::string ptrs;
    for (const FakeHipPtr& p : e.ptrs) {
      for (int k = 0; k < 8; ++k) bytes[p.at + k] = 0;
      if (skip[p.at]) continue;
      if (p.ordinal >= 0 && !alloc_ix.count(p.ordinal)) alloc_ix.emplace(p.ordinal, (int)alloc_ix.size());
      ptrs += " @" + std::to_string(p.at) + "=";
      ptrs += p.ordinal == -1 ? "null" : (p.ordinal < 0 ? "DEAD" : "A" + std::to_string(alloc_ix[p.ordinal]) + "+" + std::to_string(p.offset) +
                                                                          "/" + std::to_string(p.size));
    }
    static const char hex[] = "0123456789abcdef";
    std::string body;
    for (size_t i = 0; i < bytes.size(); ++i) {
      const unsigned char b = skip[i] ? 0 : bytes[i];
      body += hex[b >> 4];
      body += hex[b & 15];
    }
    s << " " << body << ptrs;
    out.push_back(s.str());
  }
  return out;
}

void compare_logs(const std::vector<std::string>& a, const std::vector<std::string>& b, const char* what_a, const char* what_b) {
  if (a.size() != b.size())
    error(std::string("launch counts differ: ") + what_a + " " + std::to_string(a.size()) + ", " + what_b + " " + std::to_string(b.size()));
  for (size_t i = 0; i < std::min(a.size(), b.size()); ++i)
    if (a[i] != b[i]) {
      // (the first difference: the two kernels where the names differ, else the place in the line - two hex digits per byte)
      const std::string na = a[i].substr(0, a[i].find(" grid ")), nb = b[i].substr(0, b[i].find(" grid "));
      size_t at = 0;
      while (at < a[i].size() && at < b[i].size() && a[i][at] == b[i][at]) at += 1;
      const size_t args = a[i].find(" args ") + 6;
      error(std::string("launch ") + std::to_string(i) + " differs: " + what_a + " " + na + (na != nb ? ", " + std::string(what_b) + " " + nb : "") +
            (na == nb && at >= args ? ", from argument byte " + std::to_string((at - args) / 2) : "") + "\n    " + a[i].substr(at > 40 ? at - 40 : 0, 120) +
            "\n    " + b[i].substr(at > 40 ? at - 40 : 0, 120));
      return;
    }
}

// the audit's one extent: a field buffer holds the layout's field_alloc words of the block's type
void check_field_extents(Ctx& c) {
  for (int f = 0; f < 4; ++f) {
    const size_t need = c.h->field_alloc[f] * (c.h->f32 ? sizeof(float) : sizeof(double));
    REQUIRE(fakehip_alloc_size(c.h->field.read(f)) >= need, "a field buffer is shorter than the layout's field_alloc");
  }
}

// the names the double logged for the stage launches since `from` are the six that sg_stage_kernel_name gives, no other
void check_stage_names(Ctx& c, size_t from) {
  const int region = c.b->nbr_mask ? SG_REGION_FIRST : SG_REGION_ALL;
  std::set<std::string> logged, named;
  for (size_t n = from; n < fakehip_log().size(); ++n) {
    const std::string& nm = fakehip_log()[n].name;
    if (nm.find("(sg::StageArgs") != std::string::npos) logged.insert(nm);
  }
  for (int st = 0; st < 6; ++st) {
    char buf[512] = "";
    REQUIRE(sg_stage_kernel_name(c.h, st, region, buf, sizeof(buf)) == SG_OK && buf[0], "sg_stage_kernel_name failed");
    named.insert(buf);
    if (!logged.count(buf)) error("stage " + std::to_string(st) + ": sg_stage_kernel_name says '" + buf + "', no launch does");
  }
  for (int st = 0; st < 6 && c.b->nbr_mask; ++st) {   // (a split block also launches the kernels of its SECOND regions)
    char buf[512] = "";
    if (sg_stage_kernel_name(c.h, st, SG_REGION_SECOND, buf, sizeof(buf)) == SG_OK && buf[0]) named.insert(buf);
  }
  for (const std::string& nm : logged)
    if (!named.count(nm)) error("a stage launch of '" + nm + "', which sg_stage_kernel_name does not name");
}

// ---- (a), (b): a whole life under the audit, by graph replay and eagerly ----------------------------------------------

std::vector<std::string> life(const BlockDef& b, bool graphs) {
  g_seed = 12345;
  setenv("SEIGEN_HIP_GRAPH", graphs ? "1" : "0", 1);
  fakehip_log_clear();
  Ctx c, twin;
  if (open_block(b, c) != SG_OK || open_block(b, twin) != SG_OK) {
    error(std::string("sg_create failed: ") + sg_last_error(nullptr));
    return {};
  }
  REQUIRE(c.h->family == b.family, "the block is not of the family it stands for");
  REQUIRE(c.h->graph_ok == graphs, "SEIGEN_HIP_GRAPH ignored");
  check_field_extents(c);
  auto ok = [&](int rc, const std::string& what) {
    if (rc != SG_OK) error(what + " returned " + std::to_string(rc) + ": " + sg_last_error(c.h));
    no_violations(what);
  };
  ok(configure(c, 0), "the setters");
  ok(configure(twin, 0), "the twin's setters");
  size_t mark = fakehip_log().size();
  ok(steps(c, 1), "sg_step(1)");
  check_stage_names(c, mark);
  mark = fakehip_log().size();
  ok(steps(c, 3), "sg_step(3)");
  check_stage_names(c, mark);
  // each setter on its own between two stepping calls: what it changed must reach the launches that follow (a captured graph
  // is out of date after every one of them)
  const std::pair<const char*, std::function<int()>> alone[] = {
      {"sg_set_params", [&]() { return set_material(c, 1); }},
      {"sg_set_density", [&]() { return set_density(c, 1); }},
      {"sg_set_absorption", [&]() { return set_sponge(c, 1); }},
      {"sg_set_source", [&]() { return set_source_table(c, true); }},
      {"sg_set_source_separable", [&]() { return set_source_separable(c, true); }},
      {"sg_set_receivers", [&]() { return set_receivers(c, 1); }},
      {"sg_set_monitor", [&]() { return set_monitor(c, 1); }},
      {"sg_set_spectra", [&]() { return set_spectra(c, 1); }},
      {"sg_set_injectors", [&]() { return set_injectors(c, true); }},
  };
  for (const auto& one : alone) {
    ok(one.second(), one.first);
    ok(steps(c, 2), std::string("sg_step(2) after ") + one.first + " alone");
  }
  ok(configure(c, 0), "the setters, again");
  ok(set_source_box(c), "sg_set_source_box_ricker");
  mark = fakehip_log().size();
  ok(steps(c, 2), "sg_step(2)");
  check_stage_names(c, mark);
  double sample[5];
  const std::vector<double> w = rnds((size_t)c.ncells * 3);
  ok(sg_measure(c.h, w.data(), 1, sample), "sg_measure");
  ok(sg_measure(c.h, w.data(), 0, sample), "sg_measure");
  ok(inject_once(c, true), "sg_inject");
  ok(sg_correlate(c.h, twin.h, nullptr), "sg_correlate");
  ok(sg_correlate(c.h, c.h, w.data()), "sg_correlate with itself");
  const double z[2] = {0.5, -0.25};
  ok(sg_correlate_spectra(c.h, 1, twin.h, 0, nullptr, z), "sg_correlate_spectra");
  std::vector<double> acc((size_t)c.ncells * 3);
  ok(sg_get_correlation(c.h, acc.data(), acc.size() * sizeof(double)), "sg_get_correlation");
  ok(sg_reset_correlation(c.h, 0), "sg_reset_correlation");
  ok(sg_reset_correlation(c.h, 1), "sg_reset_correlation, release");
  // transfers, whole and by range
  for (int f = 0; f < 4; ++f) {
    const size_t len = c.words(f), per = len / (size_t)c.ncells;
    std::vector<double> host = field_is_stress(f) ? tensors(c, len / (c.dim * c.dim), true) : rnds(len);
    ok(sg_set_field(c.h, f, host.data(), len * sizeof(double)), "sg_set_field");
    ok(sg_get_field(c.h, f, host.data(), len * sizeof(double)), "sg_get_field");
    const int64_t c0 = c.ncells / 3, nc = c.ncells - c0 - 1;
    ok(sg_set_field_range(c.h, f, c0, nc, host.data(), (size_t)nc * per * sizeof(double)), "sg_set_field_range");
    ok(sg_get_field_range(c.h, f, c0, nc, host.data(), (size_t)nc * per * sizeof(double)), "sg_get_field_range");
  }
  std::vector<double> spec(c.words(SG_FIELD_S));
  ok(sg_get_spectrum(c.h, 1, 1, 1, spec.data(), spec.size() * sizeof(double)), "sg_get_spectrum");
  std::vector<double> rec((size_t)kRecCap * 3 * (c.dim + c.dim * c.dim)), mon((size_t)kMonCap * 5);
  int64_t ns = 0;
  ok(sg_get_receivers(c.h, rec.data(), rec.size() * sizeof(double), &ns), "sg_get_receivers");
  ok(sg_get_monitor(c.h, mon.data(), mon.size() * sizeof(double), &ns), "sg_get_monitor");
  REQUIRE(ns == 2, "the monitor re-armed before sg_step(2) holds " + std::to_string(ns) + " samples");
  ok(steps(c, 2), "sg_step(2) after the transfers");
  ok(sg_leave_sym(c.h), "sg_leave_sym");
  int sym = 1;
  sg_get_sym(c.h, &sym);
  REQUIRE(sym == 0, "sg_leave_sym left the block in symmetric storage");
  ok(steps(c, 2), "sg_step(2) in full storage");
  // host-driven stages, packs, the un-fused operators, timing
  void* outs[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  for (int side = 0; side < 2 * c.dim; ++side) {
    size_t nb = 0;
    sg_halo_bytes(c.h, SG_FIELD_S, side, &nb);
    outs[side] = dev_alloc(c, nb);
  }
  ok(sg_halo_pack_sides(c.h, SG_FIELD_S, outs), "sg_halo_pack_sides");
  ok(sg_halo_pack(c.h, SG_FIELD_U, 0, outs[0]), "sg_halo_pack");
  ok(host_step(c), "host-driven stages with sg_end_step");
  ok(sg_enable_timing(c.h, 1), "sg_enable_timing");
  ok(host_step(c), "host-driven stages, timed");
  if (!b.nbr_mask) ok(sg_step(c.h, 2), "sg_step(2), timed");
  sg_counters_t counters;
  ok(sg_get_counters(c.h, &counters), "sg_get_counters");
  ok(sg_enable_timing(c.h, 0), "sg_enable_timing off");
  if (!b.nbr_mask) {
    ok(sg_apply_F(c.h, SG_FIELD_S, SG_FIELD_U, SG_FIELD_UH), "sg_apply_F");
    ok(sg_apply_G(c.h, SG_FIELD_U, SG_FIELD_SH, 1), "sg_apply_G");
  }
  // disarm everything, step on, destroy
  ok(sg_set_receivers(c.h, 0, nullptr, 0, 0, 0, nullptr), "disarm the receivers");
  ok(sg_set_monitor(c.h, 0, 0, nullptr, 0), "disarm the monitor");
  ok(sg_set_spectra(c.h, 0, 0, 0, 0, nullptr, nullptr), "disarm the spectra");
  ok(sg_set_injectors(c.h, 0, nullptr, 0, 0, nullptr, nullptr), "disarm the injectors");
  ok(sg_set_source(c.h, 0, nullptr, 0, nullptr), "disarm the source");
  ok(sg_set_absorption(c.h, nullptr, 0), "disarm the sponge");
  ok(steps(c, 3), "sg_step(3), bare");
  ok(sg_sync(c.h), "sg_sync");
  // comm.cpp: what needs no second rank
  const int32_t none[6] = {-1, -1, -1, -1, -1, -1};
  REQUIRE(sg_comm_check(c.h, 2, 2, none) == SG_ERR_ARG, "sg_comm_check took a rank outside the communicator");
  int32_t peers[6];
  for (int s = 0; s < 6; ++s) peers[s] = ((b.nbr_mask >> s) & 1) ? 0 : -1;
  const int cc = sg_comm_check(c.h, 0, 1, peers);
  REQUIRE(cc == SG_OK || cc == SG_ERR_STATE || (cc == SG_ERR_ARG && b.nbr_mask), "sg_comm_check: " + std::string(sg_last_error(c.h)));
  for (int s = 0; s < 6; ++s) peers[s] = ((b.nbr_mask >> s) & 1) ? -1 : 0;
  REQUIRE(sg_comm_check(c.h, 0, 1, peers) != SG_OK, "sg_comm_check took peers that contradict nbr_mask");
  REQUIRE(sg_comm_exchange(c.h, SG_FIELD_U) != SG_OK, "sg_comm_exchange without a communicator");
  const std::vector<std::string> lines = canon(0, true);
  close_block(twin, false);
  close_block(c);
  no_violations("during sg_destroy");
  return lines;
}

// ---- (c) the failure sweep -----------------------------------------------------------------------------------------------

// what a failed call must leave as it was, read through the C-ABI
struct Observed {
  int sym = -1;
  std::string names[6];
  int64_t spectra = -1, receivers = -1, monitor = -1;
  bool operator==(const Observed& o) const {
    for (int s = 0; s < 6; ++s)
      if (names[s] != o.names[s]) return false;
    return sym == o.sym && spectra == o.spectra && receivers == o.receivers && monitor == o.monitor;
  }
};
Observed observe(Ctx& c) {
  Observed o;
  sg_get_sym(c.h, &o.sym);
  for (int st = 0; st < 6; ++st) {
    char buf[512] = "";
    if (sg_stage_kernel_name(c.h, st, c.b->nbr_mask ? SG_REGION_FIRST : SG_REGION_ALL, buf, sizeof(buf)) != SG_OK) buf[0] = '?';
    o.names[st] = buf;
  }
  sg_spectra_samples(c.h, &o.spectra);
  std::vector<double> rec((size_t)kRecCap * 3 * (c.dim + c.dim * c.dim)), mon((size_t)kMonCap * 5);
  if (sg_get_receivers(c.h, rec.data(), rec.size() * sizeof(double), &o.receivers) != SG_OK) o.receivers = -2;
  if (sg_get_monitor(c.h, mon.data(), mon.size() * sizeof(double), &o.monitor) != SG_OK) o.monitor = -2;
  return o;
}

// The places where the library deliberately tolerates a failure of the runtime: the call returns SG_OK.  Told apart by the
// entry point that returned the injected failure and by whether a stream was capturing then.
struct Tolerated {
  const char* fired_at;   // the runtime's entry point, or null: any while a stream is capturing
  const char* where;
  const char* why;
};
const Tolerated kTolerated[] = {
    {"hipOccupancyMaxActiveBlocksPerMultiprocessor", "stages.cpp:166 tile_resident; kernels_mfma.hip:1477 prepare_sponge_affine_mfma",
     "the resident blocks of a persistent grid fall back to 2 per CU"},
    {"hipStreamBeginCapture", "stages.cpp:624 capture_steps", "a capture that fails switches graph replay off for the handle (stages.cpp:668): the steps run eagerly"},
    {"hipStreamEndCapture", "stages.cpp:630 capture_steps", "the same"},
    {"hipGraphInstantiate", "stages.cpp:632 capture_steps", "the same"},
    {nullptr, "stages.cpp:628 capture_steps", "the same: a launch that fails inside the capture fails the capture, not the call"},
};
// 0: not tolerated; 1: tolerated; 2: tolerated, and the handle steps eagerly from here on (a failed capture)
int tolerated(const char* call) {
  const bool stepping = std::strncmp(call, "sg_step", 7) == 0;
  for (const Tolerated& t : kTolerated) {
    if (t.fired_at ? std::strcmp(t.fired_at, fakehip_fired_at()) != 0 : !fakehip_fired_capturing()) continue;
    const bool capture = !t.fired_at || std::strncmp(t.fired_at, "hipOcc", 6) != 0;
    if (capture && !stepping) continue;   // the capture's entries: stepping calls only
    return capture ? 2 : 1;
  }
  return 0;
}

enum Base { BASE_SET = 0, BASE_STEPPED = 1 };   // every setter called; ... and sg_step(2) after them (graphs captured)
struct Call {
  const char* name;
  Base base;
  bool twin;            // the call takes a second handle, brought to the same state
  bool stepping;        // a failed call may leave the fields in any state: only leaks, captures and destruction are checked
  bool with_nbr;        // runs on the block with neighbours too (sg_step needs a communicator there)
  std::function<int(Ctx&, Ctx&)> run;
  std::function<int(Ctx&, Ctx&)> prepare;   // what the call needs beyond the base state (may be empty); not swept
};

std::vector<Call> calls() {
  std::vector<Call> v;
  auto add = [&](const char* name, Base base, std::function<int(Ctx&, Ctx&)> f, bool twin = false, bool stepping = false, bool with_nbr = true) {
    v.push_back({name, base, twin, stepping, with_nbr, std::move(f), nullptr});
  };
  add("sg_set_params", BASE_STEPPED, [](Ctx& c, Ctx&) { return set_material(c, 1); });
  add("sg_set_density", BASE_STEPPED, [](Ctx& c, Ctx&) { return set_density(c, 1); });
  add("sg_set_absorption", BASE_STEPPED, [](Ctx& c, Ctx&) { return set_sponge(c, 1); });
  // (tables that are not symmetric: the call also makes the block leave symmetric storage)
  add("sg_set_source", BASE_STEPPED, [](Ctx& c, Ctx&) { return set_source_table(c, false); });
  add("sg_set_source_separable", BASE_STEPPED, [](Ctx& c, Ctx&) { return set_source_separable(c, false); });
  add("sg_set_source_box_ricker", BASE_STEPPED, [](Ctx& c, Ctx&) { return set_source_box(c); });
  add("sg_set_receivers", BASE_STEPPED, [](Ctx& c, Ctx&) { return set_receivers(c, 1); });
  add("sg_set_injectors", BASE_STEPPED, [](Ctx& c, Ctx&) { return set_injectors(c, false); });
  add("sg_inject", BASE_STEPPED, [](Ctx& c, Ctx&) { return inject_once(c, true); });
  add("sg_inject (a table that is not symmetric)", BASE_STEPPED, [](Ctx& c, Ctx&) { return inject_once(c, false); });
  add("sg_set_monitor", BASE_STEPPED, [](Ctx& c, Ctx&) { return set_monitor(c, 1); });
  add("sg_measure", BASE_STEPPED, [](Ctx& c, Ctx&) {
    double out[5];
    const std::vector<double> w = rnds((size_t)c.ncells * 3);
    return sg_measure(c.h, w.data(), 1, out);
  });
  add("sg_set_spectra", BASE_STEPPED, [](Ctx& c, Ctx&) { return set_spectra(c, 1); });
  add("sg_correlate", BASE_STEPPED, [](Ctx& c, Ctx& t) { return sg_correlate(c.h, t.h, nullptr); }, true);
  add("sg_correlate_spectra", BASE_STEPPED, [](Ctx& c, Ctx& t) {
    const double z[2] = {0.5, -0.25};
    return sg_correlate_spectra(c.h, 1, t.h, 0, nullptr, z);
  }, true);
  add("sg_reset_correlation", BASE_STEPPED, [](Ctx& c, Ctx&) { return sg_reset_correlation(c.h, 0); });
  v.back().prepare = [](Ctx& c, Ctx&) { return sg_correlate(c.h, c.h, nullptr); };   // (an accumulator to zero)
  add("sg_set_field", BASE_STEPPED, [](Ctx& c, Ctx&) {
    const std::vector<double> host = tensors(c, c.words(SG_FIELD_S) / (c.dim * c.dim), true);
    return sg_set_field(c.h, SG_FIELD_S, host.data(), host.size() * sizeof(double));
  });
  add("sg_get_field", BASE_STEPPED, [](Ctx& c, Ctx&) {
    std::vector<double> host(c.words(SG_FIELD_U));
    return sg_get_field(c.h, SG_FIELD_U, host.data(), host.size() * sizeof(double));
  });
  add("sg_set_field_range", BASE_STEPPED, [](Ctx& c, Ctx&) {
    const size_t per = c.words(SG_FIELD_U) / (size_t)c.ncells;
    const std::vector<double> host = rnds(per * 2);
    return sg_set_field_range(c.h, SG_FIELD_U, 1, 2, host.data(), host.size() * sizeof(double));
  });
  add("sg_get_field_range", BASE_STEPPED, [](Ctx& c, Ctx&) {
    const size_t per = c.words(SG_FIELD_S) / (size_t)c.ncells;
    std::vector<double> host(per * 2);
    return sg_get_field_range(c.h, SG_FIELD_S, 1, 2, host.data(), host.size() * sizeof(double));
  });
  add("sg_get_spectrum", BASE_STEPPED, [](Ctx& c, Ctx&) {
    std::vector<double> host(c.words(SG_FIELD_S));
    return sg_get_spectrum(c.h, 1, 1, 0, host.data(), host.size() * sizeof(double));
  });
  add("sg_halo_attach + sg_halo_pack_sides", BASE_STEPPED, [](Ctx& c, Ctx&) {
    void* outs[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    for (int side = 0; side < 2 * c.dim; ++side) {
      if (((c.b->nbr_mask >> side) & 1) && sg_halo_attach(c.h, SG_FIELD_S, side, c.h->ghost[SG_FIELD_S][side]) != SG_OK) return SG_ERR_ARG;
      outs[side] = (void*)c.h->field.read(SG_FIELD_SH);   // (any live buffer: nothing runs)
    }
    return sg_halo_pack_sides(c.h, SG_FIELD_S, outs);
  });
  add("sg_step (first: capture and instantiate)", BASE_SET, [](Ctx& c, Ctx&) { return sg_step(c.h, 2); }, false, true, false);
  add("sg_step (replay)", BASE_STEPPED, [](Ctx& c, Ctx&) { return sg_step(c.h, 3); }, false, true, false);
  add("sg_run_stage", BASE_STEPPED, [](Ctx& c, Ctx&) { return sg_run_stage(c.h, SG_STAGE_U1, c.b->nbr_mask ? SG_REGION_FIRST : SG_REGION_ALL); },
      false, true);
  return v;
}

bool bring_to(const BlockDef& b, Base base, Ctx& c) {
  g_seed = 777;
  if (open_block(b, c) != SG_OK || configure(c, 0) != SG_OK) return false;
  return base == BASE_SET || steps(c, 2) == SG_OK;
}

long g_failures_injected = 0, g_tolerated = 0;

void sweep_create(const BlockDef& b) {
  for (int kind = 0; kind < FAKEHIP_NKINDS; ++kind) {
    g_where = std::string(b.name) + " sg_create kind " + std::to_string(kind);
    long n = 0;
    {
      Ctx c;
      if (!b.own_stream) (void)hipStreamCreateWithPriority(&c.user_stream, hipStreamNonBlocking, 0);
      fakehip_fail(kind, -1);
      const int rc = create_block(b, c);
      n = fakehip_calls(kind);
      REQUIRE(rc == SG_OK, "the clean call failed");
      close_block(c);
    }
    for (long k = 0; k < n; ++k) {
      Ctx c;
      if (!b.own_stream) (void)hipStreamCreateWithPriority(&c.user_stream, hipStreamNonBlocking, 0);
      fakehip_counts before, after;
      fakehip_get_counts(&before);
      fakehip_fail(kind, k);
      c.h = (sg_handle*)0x1;
      const int rc = create_block(b, c);
      REQUIRE(fakehip_fired(), "failure " + std::to_string(k) + " of " + std::to_string(n) + " was skipped");
      g_failures_injected += 1;
      if (rc == SG_OK) {
        if (!tolerated("sg_create")) error("k = " + std::to_string(k) + " (" + fakehip_fired_at() + "): SG_OK from a call the runtime failed in");
      } else {
        REQUIRE(rc == (kind == FAKEHIP_ALLOC ? SG_ERR_NOMEM : SG_ERR_DEVICE), "k = " + std::to_string(k) + " (" + fakehip_fired_at() + "): returned " + std::to_string(rc));
        REQUIRE(c.h == nullptr, "a failed sg_create left *out set");
        REQUIRE(sg_last_error(nullptr)[0] != 0, "no message");
        fakehip_get_counts(&after);
        REQUIRE(same_counts(before, after), "k = " + std::to_string(k) + " (" + fakehip_fired_at() + "): before " + show(before) + ", after " + show(after));
        c.h = nullptr;
      }
      close_block(c);
      no_violations("in a failed sg_create");
    }
  }
}

void sweep_block(const BlockDef& b) {
  setenv("SEIGEN_HIP_GRAPH", "1", 1);
  sweep_create(b);
  // what sg_step(2) launches after each base state, on a handle that never saw a failure
  std::vector<std::string> want[2];
  for (int base = 0; base < 2; ++base) {
    g_where = std::string(b.name) + " reference steps";
    Ctx c;
    REQUIRE(bring_to(b, (Base)base, c), "the base state failed");
    const size_t mark = fakehip_log().size();
    REQUIRE(steps(c, 2) == SG_OK, "sg_step(2) failed");
    want[base] = canon(mark, true);
    close_block(c);
    fakehip_log_clear();
  }
  for (const Call& call : calls()) {
    if (b.nbr_mask && !call.with_nbr) continue;
    long swept = 0;   // over the four kinds: a call that reaches the runtime nowhere is not the call the sweep is about
    for (int kind = 0; kind < FAKEHIP_NKINDS; ++kind) {
      g_where = std::string(b.name) + " " + call.name + " kind " + std::to_string(kind);
      long n = 0;
      {
        Ctx c, t;
        REQUIRE(bring_to(b, call.base, c) && (!call.twin || bring_to(b, call.base, t)), "the base state failed");
        REQUIRE(!call.prepare || call.prepare(c, t) == SG_OK, "the call's preparation failed");
        fakehip_fail(kind, -1);
        const int rc = call.run(c, t);
        n = fakehip_calls(kind);
        if (rc != SG_OK) error("the clean call returned " + std::to_string(rc) + ": " + sg_last_error(c.h));
        if (call.twin) close_block(t, false);
        close_block(c);
      }
      swept += n;
      for (long k = 0; k < n; ++k) {
        const std::string at = "k = " + std::to_string(k) + " of " + std::to_string(n);
        Ctx c, t;
        REQUIRE(bring_to(b, call.base, c) && (!call.twin || bring_to(b, call.base, t)), "the base state failed");
        REQUIRE(!call.prepare || call.prepare(c, t) == SG_OK, "the call's preparation failed");
        const Observed was = observe(c);
        fakehip_counts before, after;
        fakehip_get_counts(&before);
        fakehip_log_clear();
        fakehip_fail(kind, k);
        const int rc = call.run(c, t);
        REQUIRE(fakehip_fired(), at + ": the failure was skipped");
        g_failures_injected += 1;
        const std::string who = at + " (" + fakehip_fired_at() + ")";
        fakehip_get_counts(&after);
        REQUIRE(after.capturing == 0, who + ": a stream was left capturing");
        if (rc == SG_OK) {
          const int how = tolerated(call.name);
          if (!how) error(who + ": SG_OK from a call the runtime failed in");
          // the call succeeded: the steps that follow launch what they launch on a twin whose call met no failure - one
          // that steps eagerly where the failure was a capture's, which switched graph replay off
          if (how) {
            g_tolerated += 1;
            const size_t mark = fakehip_log().size();
            const int rs = steps(c, 2);
            REQUIRE(rs == SG_OK, who + ": sg_step(2) after the tolerated failure returned " + std::to_string(rs) + ": " + sg_last_error(c.h));
            const std::vector<std::string> got = canon(mark, true);
            Ctx r, rt;
            setenv("SEIGEN_HIP_GRAPH", how == 2 ? "0" : "1", 1);
            REQUIRE(bring_to(b, call.base, r) && (!call.twin || bring_to(b, call.base, rt)), "the twin's base state failed");
            REQUIRE(!call.prepare || call.prepare(r, rt) == SG_OK, "the twin's preparation failed");
            REQUIRE(call.run(r, rt) == SG_OK, "the twin's clean call failed");
            const size_t mark_r = fakehip_log().size();
            REQUIRE(steps(r, 2) == SG_OK, "the twin's sg_step(2) failed");
            g_where += " " + who + ", sg_step(2) after the tolerated failure";
            compare_logs(got, canon(mark_r, true), "after the tolerated failure", how == 2 ? "the eager twin" : "the twin");
            g_where = std::string(b.name) + " " + call.name + " kind " + std::to_string(kind);
            setenv("SEIGEN_HIP_GRAPH", "1", 1);
            if (call.twin) close_block(rt, false);
            close_block(r, false);
          }
        } else {
          REQUIRE(rc == (kind == FAKEHIP_ALLOC ? SG_ERR_NOMEM : SG_ERR_DEVICE), who + ": returned " + std::to_string(rc) + ": " + sg_last_error(c.h));
          REQUIRE(sg_last_error(c.h)[0] != 0, who + ": no message");
          // (only a failed sg_step may leave more behind than it found: a captured graph, the handle's event pool)
          if (std::strncmp(call.name, "sg_step", 7) != 0) REQUIRE(same_counts(before, after), who + ": before " + show(before) + ", after " + show(after));
          if (!call.stepping) {
            const Observed is = observe(c);
            REQUIRE(is == was, who + ": the handle is not as it was (storage mode " + std::to_string(was.sym) + " -> " + std::to_string(is.sym) +
                                   ", spectra " + std::to_string(was.spectra) + " -> " + std::to_string(is.spectra) + ", receivers " +
                                   std::to_string(was.receivers) + " -> " + std::to_string(is.receivers) + ", monitor " +
                                   std::to_string(was.monitor) + " -> " + std::to_string(is.monitor) + ")");
            const size_t mark = fakehip_log().size();
            const int rs = steps(c, 2);
            REQUIRE(rs == SG_OK, who + ": sg_step(2) after the failed call returned " + std::to_string(rs) + ": " + sg_last_error(c.h));
            g_where += " " + who + ", sg_step(2) after it";
            compare_logs(canon(mark, true), want[call.base], "after the failed call", "the twin");
            g_where = std::string(b.name) + " " + call.name + " kind " + std::to_string(kind);
          }
        }
        no_violations("in or after the failed call, " + who);
        if (call.twin) close_block(t, false);
        close_block(c);   // destroyable, nothing left
        no_violations("in sg_destroy after a failed call");
      }
    }
    g_where = std::string(b.name) + " " + call.name;
    REQUIRE(swept > 0, "the call made no runtime call that a failure could be injected into");
  }
}

// ---- (d) sizes that cannot be met ------------------------------------------------------------------------------------

void impossible_sizes(const BlockDef& b) {
  g_where = std::string(b.name) + " sizes that cannot be met";
  Ctx c;
  REQUIRE(bring_to(b, BASE_STEPPED, c), "the base state failed");
  const Observed was = observe(c);
  fakehip_counts before, after;
  fakehip_get_counts(&before);
  fakehip_heap_limit(before.bytes + ((size_t)1 << 20));
  const std::vector<double> p = points(c), w = rnds(3);
  int rc = sg_set_receivers(c.h, 3, p.data(), 3, 1, (int64_t)1 << 40, nullptr);
  REQUIRE(rc == SG_ERR_NOMEM || rc == SG_ERR_ARG, "sg_set_receivers with 2^40 samples returned " + std::to_string(rc));
  rc = sg_set_monitor(c.h, 1, (int64_t)1 << 40, w.data(), 0);
  REQUIRE(rc == SG_ERR_NOMEM || rc == SG_ERR_ARG, "sg_set_monitor with 2^40 samples returned " + std::to_string(rc));
  fakehip_heap_limit(before.bytes + 4096);
  const std::vector<double> wt = rnds((size_t)4 * 8 * 2);
  rc = sg_set_spectra(c.h, 8, 3, 1, 4, wt.data(), wt.data());
  REQUIRE(rc == SG_ERR_NOMEM, "sg_set_spectra with 8 frequencies under a heap limit returned " + std::to_string(rc));
  fakehip_heap_limit(0);
  fakehip_get_counts(&after);
  REQUIRE(same_counts(before, after), "before " + show(before) + ", after " + show(after));
  REQUIRE(observe(c) == was, "the previous tables are not armed as they were");
  REQUIRE(steps(c, 2) == SG_OK, "sg_step(2) afterwards failed");
  no_violations("");
  close_block(c);
}

}  // namespace

int main(int argc, char** argv) {
  const std::vector<std::string> only(argv + 1, argv + argc);
  const auto asked = [&](const char* what) { return only.empty() || std::find(only.begin(), only.end(), what) != only.end(); };
  if (!only.empty() && asked("blocks")) {
    for (const BlockDef& b : kBlocks) std::printf("%s\n", b.name);
    return 0;
  }
  // (e) every kernel object the program holds, as registered
  const std::vector<std::string> kernels = fakehip_kernels();
  for (const std::string& k : kernels) std::printf("kernel: %s\n", k.c_str());
  std::printf("host_runtime_driver: %zu kernel objects registered\n", kernels.size());
  if (kernels.empty()) {
    g_where = "registration";
    error("no kernel registered itself");
  }
  for (const BlockDef& b : kBlocks) {
    if (!asked(b.name)) continue;
    const long injected = g_failures_injected;
    g_where = std::string(b.name) + " life, graph replay";
    const std::vector<std::string> replay = life(b, true);
    g_where = std::string(b.name) + " life, eager";
    const std::vector<std::string> eager = life(b, false);
    g_where = std::string(b.name) + " replay against eager";
    compare_logs(replay, eager, "graph replay", "SEIGEN_HIP_GRAPH=0");
    fakehip_log_clear();
    sweep_block(b);
    impossible_sizes(b);
    std::printf("host_runtime_driver: block %s: %zu launches in a life, %ld failures injected, %ld of them tolerated so far\n", b.name,
                replay.size(), g_failures_injected - injected, g_tolerated);
    std::fflush(stdout);
  }
  if (asked("xfer")) run_suite("xfer", xfer_block);
  if (asked("frames")) run_suite("frames", frame_block);
  if (g_errors) {
    std::printf("host_runtime_driver: %d errors\n", g_errors);
    return 1;
  }
  std::printf("host_runtime_driver: clean\n");
  return 0;
}
