// host_xfer_driver.cpp - the device transfers of libseigen_hip (devxfer.cpp and the host half of kernels_xfer.hip) on the CPU,
// under ASan and UBSan, over the HIP runtime double of tests/fake_hip (`make -C seigen_amd/csrc host-xfer-asan`;
// tests/test_device_transfer_runtime.py).  Nothing runs on a device and no kernel runs at all: the double logs every launch
// with its argument bytes and audits the device pointers among them.  On four blocks - 3-D MFMA, lane, tile f32, generic -
//   (a) sg_get_field_dev, sg_set_field_dev and sg_get_spectrum_dev on whole fields and on ranges, both buffer types, a stress
//       into a block in symmetric storage, spectra armed and not armed: the return codes, the launches (kernel, grid within
//       its cap, LDS within a block's 64 KB - the plan of sg_xfer_plan), the write counts, the audit silent;
//   (b) what the calls refuse: SG_ERR_ARG without a call of the runtime and with the handle as it was;
//   (c) a failure injected into every runtime call of every one of those transfers: the error code, a message, nothing
//       leaked, storage mode and epoch as they were, a write counted only where the launch went out, and the same call
//       succeeding afterwards.
// (No kernel runs, so the word that reports an asymmetric stress stays zero: the second upload of that path is the GPU tests'.)
#include <functional>

#include "fake_hip.h"
#include "handle.hpp"

namespace {

int g_errors = 0;
std::string g_where;
void error(const std::string& what) {
  g_errors += 1;
  std::printf("ERROR [%s] %s\n", g_where.c_str(), what.c_str());
  std::fflush(stdout);
}
#define REQUIRE(cond, msg)                                  \
  do {                                                      \
    if (!(cond)) error(std::string(msg) + "  (" #cond ")"); \
  } while (0)

struct BlockDef {
  const char* name;
  const char* path;   // SEIGEN_HIP_PATH, or null
  int dim, degree, n[3], diagonal, dtype, gw;
};
const BlockDef kBlocks[] = {
    {"mfma-P4-f64", nullptr, 3, 4, {3, 2, 2}, 0, 0, 16},
    {"lane-2d-P2", "lane", 2, 2, {9, 8, 1}, 0, 0, 64},
    {"tile-tri-P3-f32", nullptr, 2, 3, {7, 5, 1}, 0, 1, 16},
    {"generic-1d-P2", nullptr, 1, 2, {37, 1, 1}, 0, 0, 1},
};

struct Ctx {
  const BlockDef* b = nullptr;
  sg_handle* h = nullptr;
  void* buf = nullptr;   // the caller's device buffer: room for a stress field in double
  int dim = 0, nd = 0;
  int64_t ncells = 0;
  size_t words(int f) const { return (size_t)ncells * nd * (field_is_stress(f) ? dim * dim : dim); }
  size_t cell_words(int f) const { return words(f) / (size_t)ncells; }
};

bool open_block(const BlockDef& b, Ctx& c) {
  c.b = &b;
  if (b.path) setenv("SEIGEN_HIP_PATH", b.path, 1);
  else unsetenv("SEIGEN_HIP_PATH");
  sg_config cfg;
  std::memset(&cfg, 0, sizeof(cfg));
  cfg.dim = b.dim;
  cfg.degree = b.degree;
  for (int a = 0; a < 3; ++a) {
    cfg.n[a] = b.n[a];
    cfg.h[a] = 0.5;
  }
  cfg.diagonal = b.diagonal;
  cfg.dtype = b.dtype;
  if (sg_create(&cfg, &c.h) != SG_OK) return false;
  sg_info_t info;
  sg_get_info(c.h, &info);
  c.dim = info.dim;
  c.nd = info.nd;
  c.ncells = info.ncells;
  const double lam = 2.0, mu = 1.0;
  if (sg_set_params(c.h, 1.0, 1e-3, &lam, &mu, 0) != SG_OK) return false;
  return hipMalloc(&c.buf, c.words(SG_FIELD_S) * sizeof(double)) == hipSuccess;
}

void close_block(Ctx& c) {
  if (c.buf) (void)hipFree(c.buf);
  if (c.h) sg_destroy(c.h);
  c.buf = nullptr;
  c.h = nullptr;
  fakehip_counts n;
  fakehip_get_counts(&n);
  REQUIRE(n.allocs == 0 && n.bytes == 0, "device allocations left after sg_destroy: " + std::to_string(n.allocs));
  REQUIRE(n.streams == 0 && n.events == 0 && n.graphs == 0 && n.execs == 0 && n.pinned == 0 && n.capturing == 0, "something of the runtime left after sg_destroy");
}

int arm_spectra(Ctx& c, int nfreq) {
  const std::vector<double> w((size_t)8 * (nfreq > 0 ? nfreq : 1) * 2, 0.25);
  return sg_set_spectra(c.h, nfreq, nfreq > 0 ? 3 : 0, 1, 8, w.data(), w.data());
}

// what a failed or refused call must leave as it was
struct State {
  int sym = -1;
  uint64_t epoch = 0, ver[4] = {0, 0, 0, 0};
};
State state_of(const Ctx& c) {
  State s;
  sg_get_sym(c.h, &s.sym);
  s.epoch = c.h->epoch;
  for (int f = 0; f < 4; ++f) s.ver[f] = c.h->field.versions().v[f];
  return s;
}
bool same_but_versions(const State& a, const State& b) { return a.sym == b.sym && a.epoch == b.epoch; }
bool same(const State& a, const State& b) {
  for (int f = 0; f < 4; ++f)
    if (a.ver[f] != b.ver[f]) return false;
  return same_but_versions(a, b);
}

void no_violations(const std::string& when) {
  for (size_t i = 0; i < fakehip_violations(); ++i) error("the runtime double objects " + when + ": " + fakehip_violation(i));
  fakehip_clear_violations();
}

// the launches of namespace sg::xfer in the log
std::vector<const FakeHipLaunch*> xfer_launches() {
  std::vector<const FakeHipLaunch*> r;
  for (const FakeHipLaunch& l : fakehip_log())
    if (l.op == 0 && l.name.find("sg::xfer::") != std::string::npos) r.push_back(&l);
  return r;
}

struct Call {
  std::string name;
  int writes;         // the field sg_set_field_dev writes, -1: a download
  bool kernel;        // a kernel moves it (not the device-to-device copy of gw = 1 with equal types)
  int64_t cell0, ncells;
  int ncomp, dev_bytes, caller_bytes;
  std::function<int(Ctx&)> run;
};

std::vector<Call> calls(const Ctx& c) {
  std::vector<Call> v;
  const int gw = c.b->gw, fb = c.b->dtype ? 4 : 8;
  const int64_t n = c.ncells;
  // ranges: whole; start and end inside a cube; across the first group boundary where there is one
  std::vector<std::pair<int64_t, int64_t>> ranges = {{0, n}, {1, std::min<int64_t>(n - 2, 2 * c.h->ncls + 1)}};
  if (gw > 1 && n > (int64_t)gw * c.h->ncls + c.h->ncls + 2) ranges.push_back({(int64_t)gw * c.h->ncls - c.h->ncls - 1, 2 * c.h->ncls + 3});
  for (const auto& r : ranges)
    for (int f : {SG_FIELD_U, SG_FIELD_S, SG_FIELD_SH})
      for (int dtype = 0; dtype < 2; ++dtype)
        for (int set = 0; set < 2; ++set) {
          const int64_t c0 = r.first, k = r.second;
          const size_t nbytes = (size_t)k * c.cell_words(f) * (dtype ? 4 : 8);
          const bool kernel = gw != 1 || (dtype ? 4 : 8) != fb;
          const std::string name = std::string(set ? "sg_set_field_dev" : "sg_get_field_dev") + " field " + std::to_string(f) + " cells " +
                                   std::to_string(c0) + "+" + std::to_string(k) + (dtype ? " float" : " double");
          v.push_back({name, set ? f : -1, kernel, c0, k, (int)(c.cell_words(f) / c.nd), fb, dtype ? 4 : 8, [=](Ctx& x) {
                         return set ? sg_set_field_dev(x.h, f, c0, k, x.buf, dtype, nbytes) : sg_get_field_dev(x.h, f, c0, k, x.buf, dtype, nbytes);
                       }});
        }
  for (int field = 0; field < 2; ++field)
    for (int dtype = 0; dtype < 2; ++dtype) {
      const int f = field ? SG_FIELD_S : SG_FIELD_U;
      const size_t nbytes = c.words(f) * (dtype ? 4 : 8);
      v.push_back({std::string("sg_get_spectrum_dev field ") + std::to_string(field) + (dtype ? " float" : " double"), -1, gw != 1 || dtype != 0, 0, n,
                   (int)(c.cell_words(f) / c.nd), 8, dtype ? 4 : 8, [=](Ctx& x) { return sg_get_spectrum_dev(x.h, field, 1, field, x.buf, dtype, nbytes); }});
    }
  return v;
}

// (a) one clean call: return code, launches against the plan, write counts
void clean_call(Ctx& c, const Call& call) {
  const State was = state_of(c);
  fakehip_log_clear();
  const int rc = call.run(c);
  REQUIRE(rc == SG_OK, "returned " + std::to_string(rc) + ": " + sg_last_error(c.h));
  const State is = state_of(c);
  REQUIRE(same_but_versions(was, is), "a transfer of symmetric or zero data changed the storage mode or the epoch");
  for (int f = 0; f < 4; ++f) REQUIRE(is.ver[f] == was.ver[f] + (f == call.writes ? 1 : 0), "write count of field " + std::to_string(f));
  const auto ls = xfer_launches();
  REQUIRE(ls.size() == (call.kernel ? 1u : 0u), std::to_string(ls.size()) + " transfer launches");
  int64_t plan[6];
  REQUIRE(sg_xfer_plan(c.b->gw, c.h->ncls, c.nd, call.ncomp, call.dev_bytes, call.caller_bytes, call.cell0, call.ncells, plan) == SG_OK, "sg_xfer_plan");
  for (const FakeHipLaunch* l : ls) {
    REQUIRE(l->name.find(c.b->gw == 1 ? "sg::xfer::flat<" : "sg::xfer::tiled<") != std::string::npos, "the kernel is " + l->name);
    REQUIRE(l->grid[0] == (unsigned)plan[4] && l->grid[0] <= SG_XFER_GRID_CAP && l->grid[1] == 1 && l->grid[2] == 1, "grid " + std::to_string(l->grid[0]));
    REQUIRE(l->block[0] == 256 && l->block[1] == 1, "block");
    REQUIRE(l->lds == (size_t)plan[5] && l->lds <= 65536, "LDS bytes " + std::to_string(l->lds));
    REQUIRE(l->stream == (void*)c.h->stream, "not on the handle's stream");
    REQUIRE(!l->ptrs.empty(), "no device pointer among the arguments");
    for (const FakeHipPtr& p : l->ptrs) REQUIRE(p.ordinal >= -1, "a device pointer in no live allocation");
  }
  no_violations("in " + call.name);
}

// (b) what the calls refuse
void refusals(Ctx& c) {
  const State was = state_of(c);
  const size_t nu = c.words(SG_FIELD_U) * 8, per = c.cell_words(SG_FIELD_U) * 8;
  fakehip_fail(FAKEHIP_LAUNCH, -1);
  fakehip_log_clear();
  const int rcs[] = {
      sg_get_field_dev(nullptr, 0, 0, c.ncells, c.buf, 0, nu),      sg_set_field_dev(nullptr, 0, 0, c.ncells, c.buf, 0, nu),
      sg_get_spectrum_dev(nullptr, 0, 0, 0, c.buf, 0, nu),          sg_get_field_dev(c.h, 0, 0, c.ncells, nullptr, 0, nu),
      sg_set_field_dev(c.h, 0, 0, c.ncells, nullptr, 0, nu),        sg_get_spectrum_dev(c.h, 0, 0, 0, nullptr, 0, nu),
      sg_get_field_dev(c.h, 4, 0, c.ncells, c.buf, 0, nu),          sg_set_field_dev(c.h, -1, 0, c.ncells, c.buf, 0, nu),
      sg_get_field_dev(c.h, 0, 0, c.ncells, c.buf, 2, nu),          sg_set_field_dev(c.h, 0, 0, c.ncells, c.buf, -1, nu),
      sg_get_field_dev(c.h, 0, 0, c.ncells, c.buf, 1, nu),          sg_set_field_dev(c.h, 0, 0, c.ncells, c.buf, 0, nu - 8),
      sg_get_field_dev(c.h, 0, 1, c.ncells, c.buf, 0, nu),          sg_set_field_dev(c.h, 0, -1, 2, c.buf, 0, 2 * per),
      sg_set_field_dev(c.h, 0, 0, -1, c.buf, 0, 0),                 sg_get_field_dev(c.h, 0, c.ncells, 1, c.buf, 0, per),
      sg_get_spectrum_dev(c.h, 2, 0, 0, c.buf, 0, nu),              sg_get_spectrum_dev(c.h, 0, 2, 0, c.buf, 0, nu),
      sg_get_spectrum_dev(c.h, 0, 0, 2, c.buf, 0, nu),              sg_get_spectrum_dev(c.h, 0, 0, 0, c.buf, 0, nu + 8),
      sg_get_spectrum_dev(c.h, 0, 0, 0, c.buf, 3, nu),
  };
  for (size_t i = 0; i < sizeof(rcs) / sizeof(rcs[0]); ++i) REQUIRE(rcs[i] == SG_ERR_ARG, "refusal " + std::to_string(i) + " returned " + std::to_string(rcs[i]));
  long reached = 0;
  for (int kind = 0; kind < FAKEHIP_NKINDS; ++kind) reached += fakehip_calls(kind);
  REQUIRE(reached == 0 && fakehip_log().empty(), "a refused call reached the runtime");
  REQUIRE(same(was, state_of(c)), "a refused call changed the handle");
  // an empty range moves nothing and is no error
  REQUIRE(sg_get_field_dev(c.h, 0, 3, 0, c.buf, 0, 0) == SG_OK && sg_set_field_dev(c.h, 0, 3, 0, c.buf, 1, 0) == SG_OK, "an empty range");
  REQUIRE(xfer_launches().empty() && same(was, state_of(c)), "an empty range launched or counted a write");
  no_violations("in the refusals");
}

long g_failures_injected = 0;

// (c) a failure in every runtime call of one transfer
void sweep(Ctx& c, const Call& call) {
  for (int kind = 0; kind < FAKEHIP_NKINDS; ++kind) {
    fakehip_fail(kind, -1);
    REQUIRE(call.run(c) == SG_OK, "the clean call failed");
    const long n = fakehip_calls(kind);
    for (long k = 0; k < n; ++k) {
      const std::string who = "kind " + std::to_string(kind) + ", k = " + std::to_string(k) + " of " + std::to_string(n);
      const State was = state_of(c);
      fakehip_counts before, after;
      fakehip_get_counts(&before);
      fakehip_log_clear();
      fakehip_fail(kind, k);
      const int rc = call.run(c);
      REQUIRE(fakehip_fired(), who + ": the failure was skipped");
      g_failures_injected += 1;
      const std::string at = who + " (" + fakehip_fired_at() + ")";
      REQUIRE(rc == (kind == FAKEHIP_ALLOC ? SG_ERR_NOMEM : SG_ERR_DEVICE), at + ": returned " + std::to_string(rc));
      REQUIRE(sg_last_error(c.h)[0] != 0, at + ": no message");
      fakehip_get_counts(&after);
      REQUIRE(before.allocs == after.allocs && before.bytes == after.bytes && before.events == after.events && before.streams == after.streams &&
                  before.pinned == after.pinned && after.capturing == 0,
              at + ": something leaked");
      const State is = state_of(c);
      REQUIRE(same_but_versions(was, is), at + ": storage mode or epoch changed");
      // a write is counted where, and only where, the launch that writes went out
      const uint64_t out = call.writes >= 0 ? (call.kernel ? xfer_launches().size() : (is.ver[call.writes] - was.ver[call.writes])) : 0;
      for (int f = 0; f < 4; ++f) REQUIRE(is.ver[f] == was.ver[f] + (f == call.writes ? out : 0), at + ": write count of field " + std::to_string(f));
      REQUIRE(out <= 1, at + ": more than one write");
      no_violations("in the failed call, " + at);
      fakehip_fail(kind, -1);
      REQUIRE(call.run(c) == SG_OK, at + ": the same call fails afterwards: " + sg_last_error(c.h));
    }
  }
}

void run_block(const BlockDef& b) {
  g_where = b.name;
  Ctx c;
  REQUIRE(open_block(b, c), std::string("the block does not open: ") + sg_last_error(c.h));
  if (!c.h || !c.buf) return;
  REQUIRE((int)c.h->md.gw == b.gw, "the block's layout is not the family's");
  int sym = -1;
  sg_get_sym(c.h, &sym);
  REQUIRE(sym == (b.gw != 1 ? 1 : 0), "storage mode of a fresh block");
  // spectra not armed: SG_ERR_STATE, nothing launched
  fakehip_log_clear();
  for (int field = 0; field < 2; ++field)
    REQUIRE(sg_get_spectrum_dev(c.h, field, 0, 0, c.buf, 0, c.words(field ? SG_FIELD_S : SG_FIELD_U) * 8) == SG_ERR_STATE, "spectra not armed");
  REQUIRE(fakehip_log().empty(), "a launch without spectra");
  REQUIRE(arm_spectra(c, 2) == SG_OK, "sg_set_spectra");
  const std::vector<Call> all = calls(c);
  for (const Call& call : all) {
    g_where = std::string(b.name) + " " + call.name;
    clean_call(c, call);
  }
  g_where = std::string(b.name) + " refusals";
  refusals(c);
  for (const Call& call : all) {
    g_where = std::string(b.name) + " " + call.name + " sweep";
    sweep(c, call);
  }
  g_where = b.name;
  REQUIRE(arm_spectra(c, 0) == SG_OK, "disarming the spectra");
  REQUIRE(sg_get_spectrum_dev(c.h, 1, 0, 0, c.buf, 0, c.words(SG_FIELD_S) * 8) == SG_ERR_STATE, "spectra disarmed");
  std::printf("%s: %zu transfers\n", b.name, all.size());
  close_block(c);
  no_violations("during sg_destroy");
}

}  // namespace

int main() {
  unsetenv("SEIGEN_HIP_SYM");
  for (const BlockDef& b : kBlocks) run_block(b);
  std::printf("host_xfer_driver: %ld failures injected, %d errors\n", g_failures_injected, g_errors);
  if (g_errors) return 1;
  std::printf("host_xfer_driver: clean\n");
  return 0;
}
