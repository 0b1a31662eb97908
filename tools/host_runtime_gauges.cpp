// host_runtime_gauges.cpp - the gauges of libseigen_hip (gauge.cpp, the sixth hook of stages.cpp and the host half of
// kernels_gauge.hip) on the CPU under ASan and UBSan over the HIP runtime double of tests/fake_hip: a program of its own,
// build_tools/host_runtime_gauges (`make -C seigen_amd/csrc host-runtime-asan`; tests/test_gauges_runtime.py), over the objects
// and the helpers of host_runtime_driver (host_runtime_common.hpp) - that program's kernel objects are a closed list, which
// this kernel is no part of.  It prints the kernel objects it registered, then on the four blocks of kSuiteBlocks
//   (a) a life of the gauges with graph replay and with SEIGEN_HIP_GRAPH=0: nothing armed, armed, stepped by sg_step(1) and by
//       longer calls up to the capacity, refused beyond it before anything is queued, read out, probed once, armed again with
//       another `every` and kind, stepped through sg_end_step up to its refusal, disarmed - the return codes, the counts of
//       samples, the allocations, every launch of sg::gauge:: under the pointer audit (the field, the tables and the trace against
//       the extents the kernel walks), and the launches of graph replay equal to those of eager steps but for the step (by
//       value against the hook's counter);
//   (b) what the calls refuse: SG_ERR_ARG without a call of the runtime and with the handle as it was;
//   (c) a failure injected into every runtime call of sg_set_gauges, sg_get_gauges and sg_probe_gradient, with gauges armed
//       before and not: the error code, a message, nothing leaked, the gauges armed before with their count intact, and the
//       same call succeeding afterwards.
// (No kernel runs: what the samples hold is the GPU tests' business.)
#include <sstream>

#include "host_runtime_common.hpp"

namespace {

// what a failed or refused call must leave as it was: the armed gauges, their clock, the epoch, fields and storage mode
struct State : FieldState {
  int64_t npts = 0, nown = 0, every = 0, count = 0, steps = 0;
  int kind = 0;
  const void* buf[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
};
State state_of(const Ctx& c) {
  State s;
  static_cast<FieldState&>(s) = field_state_of(c);
  const GaugeTables& t = c.h->gge;
  s.npts = t.npts;
  s.nown = t.nown;
  s.kind = t.kind;
  s.every = t.clock.every;
  s.count = t.clock.count;
  s.steps = t.clock.steps;
  const void* p[7] = {t.item.get(), t.lane.get(), t.cls.get(), t.D.get(), t.J.get(), t.trace.get(), t.ctr.get()};
  for (int k = 0; k < 7; ++k) s.buf[k] = p[k];
  return s;
}
bool same(const State& a, const State& b) {
  for (int k = 0; k < 7; ++k)
    if (a.buf[k] != b.buf[k]) return false;
  return same_fields(a, b) && a.npts == b.npts && a.nown == b.nown && a.kind == b.kind && a.every == b.every && a.count == b.count &&
         a.steps == b.steps;
}

// six points of the block (h = 0.5 on every axis): four inside cells, one on a grid line, one outside the mesh
constexpr int kPoints = 6, kOwned = 5;
std::vector<double> points_of(const Ctx& c) {
  const double fr[kPoints][3] = {{0.31, 0.22, 0.17}, {0.55, 0.41, 0.63}, {0.12, 0.83, 0.35}, {0.93, 0.07, 0.71}, {0.5, 0.33, 0.5}, {-0.4, -0.4, -0.4}};
  std::vector<double> p;
  for (int k = 0; k < kPoints; ++k)
    for (int a = 0; a < c.dim; ++a) {
      const double extent = 0.5 * c.b->n[a];
      // (the grid-line point: a cube boundary along every axis that has more than one cube)
      p.push_back(k == 4 && c.b->n[a] > 1 ? 0.5 * (c.b->n[a] / 2) : fr[k][a] * extent);
    }
  return p;
}
int ncomp_of(const Ctx& c, int kind) { return grad_ncomp(c.dim, kind); }

template <typename T>
T scalar(const FakeHipLaunch& l, size_t i) {
  T v = T();
  if (i < l.params.size() && l.params[i].size == sizeof(T)) std::memcpy(&v, l.args.data() + l.params[i].at, sizeof(T));
  else error("parameter " + std::to_string(i) + " of " + l.name + " is not of " + std::to_string(sizeof(T)) + " bytes");
  return v;
}
const FakeHipPtr* pointer(const FakeHipLaunch& l, size_t i) {
  if (i >= l.params.size()) return nullptr;
  for (const FakeHipPtr& p : l.ptrs)
    if (p.at == l.params[i].at) return &p;
  return nullptr;
}
void holds(const FakeHipLaunch& l, size_t i, size_t bytes, const char* what, bool may_be_null = false) {
  const FakeHipPtr* p = pointer(l, i);
  if (!p) return error(std::string(what) + ": parameter " + std::to_string(i) + " of " + l.name + " is no device pointer");
  if (p->ordinal == -1 && may_be_null) return;
  REQUIRE(p->ordinal >= 0, std::string(what) + " is null or in no live allocation");
  REQUIRE(p->ordinal < 0 || p->size - p->offset >= bytes, std::string(what) + " is shorter than the " + std::to_string(bytes) + " bytes the kernel walks");
}

// The pointer audit of every sg::gauge:: launch in the log, against the extents the kernel walks; `probe`: the launches are
// one-shots (step = every = capacity = 1, tables of their own).  Returns the launches as lines that graph replay and eager
// steps must share: everything but the step (parameters 1 and 2).
std::vector<std::string> audit(Ctx& c, int kind, int64_t every, int64_t capacity, bool probe = false) {
  std::vector<std::string> lines;
  const size_t fb = c.b->dtype ? 4 : 8;
  const size_t field_words = (size_t)c.h->md.ncube_pad * c.h->ncls * c.nd * c.dim;
  for (const FakeHipLaunch* l : launches_of("sg::gauge::")) {
    REQUIRE(l->stream == (void*)c.h->stream, "not on the handle's stream");
    REQUIRE(l->block[0] == 256 && l->block[1] == 1 && l->block[2] == 1 && l->lds == 0, "block or LDS of " + l->name);
    REQUIRE(l->grid[0] == (unsigned)((kOwned + 3) / 4) && l->grid[1] == 1 && l->grid[2] == 1, "grid of " + l->name);
    for (const FakeHipPtr& p : l->ptrs) REQUIRE(p.ordinal >= -1, "a device pointer in no live allocation");
    for (const FakeHipParam& p : l->params) REQUIRE(p.type.find("sg::") == std::string::npos, "a struct by value: " + p.type);
    REQUIRE(l->name.find(c.b->dtype ? "sample<float>" : "sample<double>") != std::string::npos, "the kernel is " + l->name);
    REQUIRE(l->params.size() == 17, "parameters of " + l->name);
    if (l->params.size() != 17) continue;
    const int64_t nown = scalar<int64_t>(*l, 11);
    const int ncomp = scalar<int>(*l, 12);
    REQUIRE(nown == kOwned && ncomp == ncomp_of(c, kind) && scalar<int>(*l, 13) == kind, "nown, ncomp, kind");
    REQUIRE(scalar<int>(*l, 14) == c.dim && scalar<int>(*l, 15) == c.nd && scalar<int>(*l, 16) == c.b->gw, "dim, nd, gw");
    REQUIRE(scalar<int64_t>(*l, 3) == every && scalar<int64_t>(*l, 4) == capacity, "every, capacity");
    REQUIRE(c.nd * c.dim <= gauge::MAX_VALUES, "the element does not fit a wave's slab");
    holds(*l, 0, field_words * fb, "the field");
    holds(*l, 1, 8, "the step counter", true);
    holds(*l, 5, (size_t)nown * 8, "item");
    holds(*l, 6, (size_t)nown * 4, "lane");
    holds(*l, 7, (size_t)nown * 4, "cls");
    holds(*l, 8, (size_t)nown * c.dim * c.nd * 8, "D");
    holds(*l, 9, (size_t)c.h->ncls * 9 * 8, "J");
    holds(*l, 10, (size_t)capacity * nown * ncomp * 8, "the trace");
    const FakeHipPtr* ctr = pointer(*l, 1);
    REQUIRE(ctr && (l->replay ? ctr->ordinal >= 0 : ctr->ordinal == -1), "the step comes by value in eager launches, from the counter in a replay");
    if (probe) REQUIRE(!l->replay && scalar<int64_t>(*l, 2) == 1, "a one-shot names step 1");
    std::ostringstream s;
    s << l->name << " grid " << l->grid[0];
    for (size_t i = 3; i < 5; ++i) s << " " << (long long)scalar<int64_t>(*l, i);
    for (size_t i = 11; i < 17; ++i) s << " " << (l->params[i].size == 8 ? (long long)scalar<int64_t>(*l, i) : (long long)scalar<int>(*l, i));
    for (size_t i : {0, 5, 6, 7, 8, 9, 10}) {
      const FakeHipPtr* p = pointer(*l, i);
      s << " p" << i << "=" << (p ? p->offset : (size_t)-1) << "/" << (p ? p->size : 0);
    }
    lines.push_back(s.str());
  }
  return lines;
}

size_t samples_launched() { return launches_of("sg::gauge::sample<").size(); }

int64_t taken(Ctx& c, int64_t capacity, int ncomp) {
  std::vector<double> out((size_t)(capacity * kPoints * ncomp) + 1);
  int64_t n = -1;
  REQUIRE(sg_get_gauges(c.h, out.data(), (size_t)(capacity * kPoints * ncomp) * 8, &n) == SG_OK, std::string("sg_get_gauges: ") + sg_last_error(c.h));
  return n;
}

// (a) one life; the launches of its every = 1 part, for the comparison of the two modes
std::vector<std::string> life(const BlockDef& b, bool graphs) {
  setenv("SEIGEN_HIP_GRAPH", graphs ? "1" : "0", 1);
  Ctx c;
  REQUIRE(open_with_material(b, c), std::string("the block does not open: ") + sg_last_error(c.h));
  if (!c.h) return {};
  REQUIRE((int)c.h->md.gw == b.gw, "the block's layout is not the family's");
  REQUIRE(c.h->graph_ok == graphs, "SEIGEN_HIP_GRAPH ignored");
  const std::vector<double> pts = points_of(c);
  auto ok = [&](int rc, const std::string& what) {
    if (rc != SG_OK) error(what + " returned " + std::to_string(rc) + ": " + sg_last_error(c.h));
    no_violations(what);
  };
  // nothing armed: no launch in a step, the getter has nothing
  fakehip_log_clear();
  ok(sg_step(c.h, 3), "sg_step with nothing armed");
  REQUIRE(launches_of("sg::gauge::").empty() && taken(c, 0, 0) == 0, "a fresh handle has gauges");
  fakehip_counts bare, armed, now;
  fakehip_get_counts(&bare);
  // kind 3, every = 1, 16 samples: steps 1 + 5 + 10 fill the trace
  const int k3 = 3, n3 = ncomp_of(c, k3);
  int32_t owned[kPoints] = {-1, -1, -1, -1, -1, -1};
  uint64_t epoch = c.h->epoch;
  ok(sg_set_gauges(c.h, kPoints, pts.data(), k3, 1, 16, owned), "sg_set_gauges");
  for (int k = 0; k < kPoints; ++k) REQUIRE(owned[k] == (k < kOwned ? 1 : 0), "owned[" + std::to_string(k) + "]");
  fakehip_get_counts(&armed);
  REQUIRE(armed.allocs == bare.allocs + 7 && armed.bytes >= bare.bytes + (size_t)16 * kOwned * n3 * 8, "arming allocates five tables, the trace and the counter");
  REQUIRE(c.h->epoch == epoch + 1 && taken(c, 16, n3) == 0, "arming bumps the epoch and starts the count");
  fakehip_log_clear();
  ok(sg_step(c.h, 1), "sg_step(1)");
  REQUIRE(samples_launched() == 1 && taken(c, 16, n3) == 1, "one launch in a step");
  ok(sg_step(c.h, 5), "sg_step(5)");
  ok(sg_step(c.h, 10), "sg_step(10)");
  REQUIRE(samples_launched() == 16 && taken(c, 16, n3) == 16, std::to_string(samples_launched()) + " launches in 16 steps");
  const std::vector<std::string> lines = audit(c, k3, 1, 16);
  no_violations("in the steps");
  // the trace is full: the next step is refused before anything is queued
  State was = state_of(c);
  fakehip_log_clear();
  fakehip_fail(FAKEHIP_LAUNCH, -1);
  REQUIRE(sg_step(c.h, 1) == SG_ERR_STATE && std::string(sg_last_error(c.h)).find("gauge") != std::string::npos, "sg_step beyond the capacity");
  REQUIRE(fakehip_log().empty() && runtime_calls() == 0 && same(was, state_of(c)) && taken(c, 16, n3) == 16, "a refused step queued or counted something");
  // the one-shot: tables of its own, one launch, nothing left, nothing changed
  for (int field : {(int)SG_FIELD_U, (int)SG_FIELD_UH})
    for (int kind = 0; kind < 4; ++kind) {
      const int nc = ncomp_of(c, kind);
      if (nc == 0) continue;
      std::vector<double> out((size_t)kPoints * nc, -7.0);
      fakehip_log_clear();
      fakehip_fail(FAKEHIP_ALLOC, -1);
      ok(sg_probe_gradient(c.h, field, kind, kPoints, pts.data(), out.data(), out.size() * 8, owned), "sg_probe_gradient");
      REQUIRE(samples_launched() == 1 && fakehip_calls(FAKEHIP_ALLOC) == 6, "sg_probe_gradient: one launch, six temporary allocations");
      audit(c, kind, 1, 1, true);
      for (int q = 0; q < nc; ++q) REQUIRE(out[(size_t)(kPoints - 1) * nc + q] == 0.0, "the row of the point outside is not 0.0");
      REQUIRE(owned[0] == 1 && owned[kPoints - 1] == 0, "owned of the probe");
    }
  fakehip_get_counts(&now);
  REQUIRE(same_counts(now, armed) && same(was, state_of(c)), "a probe changed the handle or left something: " + show(now));
  // armed again with another every and kind: a fresh trace, the count from zero; a refusing hook launches at every step
  const int k1 = 1, n1 = ncomp_of(c, k1);
  epoch = c.h->epoch;
  ok(sg_set_gauges(c.h, kPoints, pts.data(), k1, 2, 3, nullptr), "arming again");
  fakehip_get_counts(&now);
  REQUIRE(now.allocs == bare.allocs + 7 && c.h->epoch == epoch + 1 && taken(c, 3, n1) == 0 && c.h->gge.clock.steps == 0, "arming again: " + show(now));
  fakehip_log_clear();
  ok(sg_step(c.h, 5), "sg_step(5), every = 2");
  REQUIRE(taken(c, 3, n1) == 2 && samples_launched() == 5, std::to_string(samples_launched()) + " launches in five steps of every = 2");
  audit(c, k1, 2, 3);
  REQUIRE(sg_step(c.h, 3) == SG_ERR_STATE, "sg_step(3) would take a fourth sample");
  ok(sg_step(c.h, 2), "sg_step(2), every = 2, up to the capacity");
  REQUIRE(taken(c, 3, n1) == 3, "three samples");
  // host-driven stages with sg_end_step: two samples, then the refusal, which does not count the step
  ok(sg_set_gauges(c.h, kPoints, pts.data(), 0, 1, 2, nullptr), "arming the gradient");
  const int n0 = ncomp_of(c, 0);
  fakehip_log_clear();
  for (int k = 0; k < 3; ++k) {
    for (int st = 0; st < 6; ++st) ok(sg_run_stage(c.h, st, SG_REGION_ALL), "sg_run_stage");
    if (k < 2) {
      ok(sg_end_step(c.h), "sg_end_step");
    } else {
      was = state_of(c);
      const size_t before = samples_launched();
      REQUIRE(sg_end_step(c.h) == SG_ERR_STATE && samples_launched() == before && c.h->gge.clock.steps == 2, "sg_end_step beyond the capacity");
    }
  }
  REQUIRE(samples_launched() == 2 && taken(c, 2, n0) == 2, "sg_end_step: a launch per step");
  audit(c, 0, 1, 2);
  // a failed arming call leaves these recording
  was = state_of(c);
  REQUIRE(sg_set_gauges(c.h, kPoints, pts.data(), 7, 1, 2, nullptr) == SG_ERR_ARG && same(was, state_of(c)), "a bad kind");
  // disarmed: everything freed
  epoch = c.h->epoch;
  ok(sg_set_gauges(c.h, 0, nullptr, 0, 0, 0, nullptr), "disarming");
  fakehip_get_counts(&now);
  REQUIRE(now.allocs == bare.allocs && now.bytes == bare.bytes && c.h->epoch == epoch + 1 && taken(c, 0, 0) == 0, "disarming frees the tables: " + show(now));
  fakehip_log_clear();
  ok(sg_step(c.h, 2), "sg_step after disarming");
  REQUIRE(launches_of("sg::gauge::").empty(), "a launch after disarming");
  close_block(c);
  no_violations("during sg_destroy");
  return lines;
}

// (b) what the calls refuse, with gauges armed
void refusals(Ctx& c, const std::vector<double>& pts) {
  const State was = state_of(c);
  const int n3 = ncomp_of(c, 3);
  std::vector<double> out((size_t)16 * kPoints * 9);
  int64_t k = 0;
  const size_t nb = (size_t)5 * kPoints * n3 * 8, pb = (size_t)kPoints * n3 * 8;
  watch_runtime();
  std::vector<int> rcs = {
      sg_set_gauges(nullptr, kPoints, pts.data(), 3, 1, 4, nullptr), sg_get_gauges(nullptr, out.data(), nb, &k), sg_get_gauges(c.h, out.data(), nb, nullptr),
      sg_probe_gradient(nullptr, SG_FIELD_U, 3, kPoints, pts.data(), out.data(), pb, nullptr),
      sg_set_gauges(c.h, -1, pts.data(), 3, 1, 4, nullptr), sg_set_gauges(c.h, kPoints, nullptr, 3, 1, 4, nullptr),
      sg_set_gauges(c.h, kPoints, pts.data(), -1, 1, 4, nullptr), sg_set_gauges(c.h, kPoints, pts.data(), 4, 1, 4, nullptr),
      sg_set_gauges(c.h, kPoints, pts.data(), 3, 0, 4, nullptr), sg_set_gauges(c.h, kPoints, pts.data(), 3, 1, -1, nullptr),
      sg_get_gauges(c.h, out.data(), nb - 8, &k), sg_get_gauges(c.h, out.data(), nb + 8, &k), sg_get_gauges(c.h, nullptr, nb, &k),
      sg_probe_gradient(c.h, SG_FIELD_S, 3, kPoints, pts.data(), out.data(), pb, nullptr),
      sg_probe_gradient(c.h, SG_FIELD_SH, 3, kPoints, pts.data(), out.data(), pb, nullptr),
      sg_probe_gradient(c.h, 4, 3, kPoints, pts.data(), out.data(), pb, nullptr), sg_probe_gradient(c.h, SG_FIELD_U, 4, kPoints, pts.data(), out.data(), pb, nullptr),
      sg_probe_gradient(c.h, SG_FIELD_U, -1, kPoints, pts.data(), out.data(), pb, nullptr),
      sg_probe_gradient(c.h, SG_FIELD_U, 3, kPoints, pts.data(), out.data(), pb - 8, nullptr),
      sg_probe_gradient(c.h, SG_FIELD_U, 3, kPoints, pts.data(), out.data(), pb + 8, nullptr),
      sg_probe_gradient(c.h, SG_FIELD_U, 3, kPoints, pts.data(), nullptr, pb, nullptr), sg_probe_gradient(c.h, SG_FIELD_U, 3, kPoints, nullptr, out.data(), pb, nullptr),
      sg_probe_gradient(c.h, SG_FIELD_U, 3, -1, pts.data(), out.data(), pb, nullptr),
  };
  if (c.dim == 1) {   // no curl in one dimension
    rcs.push_back(sg_set_gauges(c.h, kPoints, pts.data(), 2, 1, 4, nullptr));
    rcs.push_back(sg_probe_gradient(c.h, SG_FIELD_U, 2, kPoints, pts.data(), out.data(), (size_t)kPoints * 8, nullptr));
  }
  all_refused(rcs);
  REQUIRE(same(was, state_of(c)), "a refused call changed the handle");
  no_violations("in the refusals");
}

struct Call {
  std::string name;
  std::function<int(Ctx&)> run;
};

long sweep(Ctx& c, const Call& call, const std::function<int(Ctx&)>& before) {
  return sweep_in_place(c, call.run, before, [&]() { return state_of(c); },
                        [&](const State& was, const std::string& at) { REQUIRE(same(was, state_of(c)), at + ": the handle changed"); });
}

long sweeps(const BlockDef& b) {
  unsetenv("SEIGEN_HIP_GRAPH");
  Ctx c;
  REQUIRE(open_with_material(b, c), std::string("the block does not open: ") + sg_last_error(c.h));
  if (!c.h) return 0;
  const std::vector<double> pts = points_of(c);
  const double* const p = pts.data();
  const std::function<int(Ctx&)> armed_before = [p](Ctx& x) {
    if (int rc = sg_set_gauges(x.h, kPoints, p, 3, 2, 5, nullptr)) return rc;
    return sg_step(x.h, 3);
  };
  const std::function<int(Ctx&)> none_before = [](Ctx& x) { return sg_set_gauges(x.h, 0, nullptr, 0, 0, 0, nullptr); };
  REQUIRE(armed_before(c) == SG_OK, "arming and stepping");
  g_where = std::string(b.name) + " refusals";
  refusals(c, pts);
  long injected = 0;
  size_t calls = 0;
  for (int kind = 0; kind < 4; ++kind) {
    if (ncomp_of(c, kind) == 0) continue;
    const Call set{"sg_set_gauges kind " + std::to_string(kind), [=](Ctx& x) { return sg_set_gauges(x.h, kPoints, p, kind, 1, 7, nullptr); }};
    g_where = std::string(b.name) + " " + set.name + " sweep, gauges armed before";
    injected += sweep(c, set, armed_before);
    g_where = std::string(b.name) + " " + set.name + " sweep, nothing armed before";
    injected += sweep(c, set, none_before);
  }
  const Call off{"sg_set_gauges disarming", [](Ctx& x) { return sg_set_gauges(x.h, 0, nullptr, 0, 0, 0, nullptr); }};
  g_where = std::string(b.name) + " " + off.name + " sweep";
  injected += sweep(c, off, armed_before);
  // the getter and the probe, on stepped gauges
  REQUIRE(armed_before(c) == SG_OK, "arming and stepping");
  const int n3 = ncomp_of(c, 3);
  std::vector<double> out((size_t)5 * kPoints * 9);
  double* const o = out.data();
  const Call get{"sg_get_gauges", [=](Ctx& x) {
                   int64_t n = 0;
                   return sg_get_gauges(x.h, o, (size_t)5 * kPoints * n3 * 8, &n);
                 }};
  g_where = std::string(b.name) + " " + get.name + " sweep";
  injected += sweep(c, get, nullptr);
  calls += 1;
  for (int field : {(int)SG_FIELD_U, (int)SG_FIELD_UH})
    for (int kind = 0; kind < 4; ++kind) {
      const int nc = ncomp_of(c, kind);
      if (nc == 0) continue;
      const Call probe{"sg_probe_gradient field " + std::to_string(field) + " kind " + std::to_string(kind),
                       [=](Ctx& x) { return sg_probe_gradient(x.h, field, kind, kPoints, p, o, (size_t)kPoints * nc * 8, nullptr); }};
      g_where = std::string(b.name) + " " + probe.name + " sweep";
      injected += sweep(c, probe, nullptr);
      calls += 1;
    }
  g_where = b.name;
  std::printf("%s: %zu read-outs\n", b.name, calls);
  close_block(c);
  no_violations("during sg_destroy");
  return injected;
}

}  // namespace

static long gauge_block(const BlockDef& b) {
  g_where = std::string(b.name) + " life, graph replay";
  const std::vector<std::string> replay = life(b, true);
  g_where = std::string(b.name) + " life, eager";
  const std::vector<std::string> eager = life(b, false);
  g_where = std::string(b.name) + " replay against eager";
  REQUIRE(!replay.empty() && replay.size() == eager.size(), "launches: graph replay " + std::to_string(replay.size()) + ", SEIGEN_HIP_GRAPH=0 " + std::to_string(eager.size()));
  for (size_t i = 0; i < std::min(replay.size(), eager.size()); ++i)
    if (replay[i] != eager[i]) {
      error("launch " + std::to_string(i) + " differs:\n    " + replay[i] + "\n    " + eager[i]);
      break;
    }
  const long injected = sweeps(b);
  unsetenv("SEIGEN_HIP_GRAPH");
  return injected;
}

int main() {
  const std::vector<std::string> kernels = fakehip_kernels();
  for (const std::string& k : kernels) std::printf("kernel: %s\n", k.c_str());
  std::printf("host_runtime_gauges: %zu kernel objects registered\n", kernels.size());
  run_suite("gauges", gauge_block);
  if (g_errors) {
    std::printf("host_runtime_gauges: %d errors\n", g_errors);
    return 1;
  }
  std::printf("host_runtime_gauges: clean\n");
  return 0;
}
