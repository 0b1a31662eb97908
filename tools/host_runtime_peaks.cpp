// host_runtime_peaks.cpp - the peak maps of libseigen_hip (peak.cpp, the fifth hook of stages.cpp and the host half of
// kernels_peak.hip) on the CPU under ASan and UBSan over the HIP runtime double of tests/fake_hip: a program of its own,
// build_tools/host_runtime_peaks (`make -C seigen_amd/csrc host-runtime-asan`; tests/test_peaks_runtime.py), over the objects
// and the helpers of host_runtime_driver (host_runtime_common.hpp) - that program's kernel objects are a closed list, which
// these kernels are no part of.  It prints the kernel objects it registered, then on the four blocks of kSuiteBlocks
//   (a) a life of the maps with graph replay and with SEIGEN_HIP_GRAPH=0: nothing armed, armed, stepped by sg_step(1) and by
//       longer calls up to the end of the series and beyond it, read out with both getters, armed again with another
//       `every`, disarmed - the return codes, the counts of samples, the allocations, every launch of sg::peak:: under the
//       pointer audit (the field, val, idx and the caller's buffers against the extents the kernels walk), and the update
//       launches of graph replay equal to those of eager steps but for the step (by value against the hook's counter);
//   (b) what the calls refuse: SG_ERR_ARG without a call of the runtime and with the handle as it was;
//   (c) a failure injected into every runtime call of sg_set_peaks, sg_get_peaks and sg_get_peaks_dev, with maps armed before
//       and not: the error code, a message, nothing leaked, the maps armed before with their count intact, and the same call
//       succeeding afterwards.
// (No kernel runs: what the maps hold is the GPU tests' business.)
#include <sstream>

#include "host_runtime_common.hpp"

namespace {

// what a failed or refused call must leave as it was: the armed maps, their clock, the epoch, fields and storage mode
struct State : FieldState {
  int what = 0;
  int64_t every = 0, count = 0, steps = 0;
  const void* buf[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
};
State state_of(const Ctx& c) {
  State s;
  static_cast<FieldState&>(s) = field_state_of(c);
  const PeakTables& t = c.h->pk;
  s.what = t.what;
  s.every = t.clock.every;
  s.count = t.clock.count;
  s.steps = t.clock.steps;
  const void* p[5] = {t.val[0].get(), t.val[1].get(), t.idx[0].get(), t.idx[1].get(), t.ctr.get()};
  for (int k = 0; k < 5; ++k) s.buf[k] = p[k];
  return s;
}
bool same(const State& a, const State& b) {
  for (int k = 0; k < 5; ++k)
    if (a.buf[k] != b.buf[k]) return false;
  return same_fields(a, b) && a.what == b.what && a.every == b.every && a.count == b.count && a.steps == b.steps;
}

size_t nvalues(const Ctx& c) { return (size_t)c.ncells * c.nd; }
size_t node_words(const Ctx& c) { return (size_t)c.h->md.ncube_pad * c.h->ncls * c.nd; }
void* value_buf(const Ctx& c) { return c.bufs[0]; }
int32_t* sample_buf(const Ctx& c) { return (int32_t*)c.bufs[1]; }

template <typename T>
T scalar(const FakeHipLaunch& l, size_t i) {
  T v = T();
  if (i < l.params.size() && l.params[i].size == sizeof(T)) std::memcpy(&v, l.args.data() + l.params[i].at, sizeof(T));
  else error("parameter " + std::to_string(i) + " of " + l.name + " is not of " + std::to_string(sizeof(T)) + " bytes");
  return v;
}
// the device pointer that is parameter i of the launch, or null
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

// The pointer audit of every sg::peak:: launch in the log, against the extents the kernels walk; returns the update launches
// as lines that graph replay and eager steps must share: everything but the step (parameters 3 and 4).
std::vector<std::string> audit(Ctx& c) {
  std::vector<std::string> lines;
  const size_t n = node_words(c), fb = c.b->dtype ? 4 : 8;
  for (const FakeHipLaunch* l : launches_of("sg::peak::")) {
    REQUIRE(l->stream == (void*)c.h->stream, "not on the handle's stream");
    REQUIRE(l->block[0] == 256 && l->block[1] == 1 && l->block[2] == 1 && l->lds == 0, "block or LDS of " + l->name);
    REQUIRE(l->grid[0] >= 1 && l->grid[0] <= 8u * (unsigned)std::max(c.h->ncu, 1) && l->grid[1] == 1 && l->grid[2] == 1, "grid of " + l->name);
    for (const FakeHipPtr& p : l->ptrs) REQUIRE(p.ordinal >= -1, "a device pointer in no live allocation");
    for (const FakeHipParam& p : l->params) REQUIRE(p.type.find("sg::") == std::string::npos, "a struct by value: " + p.type);
    if (l->name.find("sg::peak::update<") != std::string::npos) {
      REQUIRE(l->name.find(c.b->dtype ? "update<float>" : "update<double>") != std::string::npos, "the kernel is " + l->name);
      REQUIRE(l->params.size() == 12, "parameters of " + l->name);
      if (l->params.size() != 12) continue;
      const int ncomp = scalar<int>(*l, 9), dim = scalar<int>(*l, 10), sym = scalar<int>(*l, 11);
      REQUIRE(scalar<int64_t>(*l, 7) == (int64_t)n, "n is not the node words of the layout");
      REQUIRE(1 << scalar<int>(*l, 8) == c.b->gw, "gw_shift is not the layout's");
      REQUIRE(dim == c.dim && (ncomp == dim || ncomp == dim * dim), "ncomp, dim");
      int hsym = 0;
      sg_get_sym(c.h, &hsym);
      // (only a tensor has the line rule; in 1-D both fields have the one line 0, with or without it)
      REQUIRE(dim == 1 ? (sym == 0 || sym == hsym) : sym == (ncomp == dim * dim ? hsym : 0), "sym is not the storage mode");
      REQUIRE(scalar<int64_t>(*l, 5) == c.h->pk.clock.every && scalar<int64_t>(*l, 6) == c.h->pk.clock.count, "every, nsamples");
      holds(*l, 0, n * ncomp * fb, "the field");
      holds(*l, 1, n * 8, "val");
      holds(*l, 2, n * 4, "idx");
      holds(*l, 3, 8, "the step counter", true);
      const FakeHipPtr* ctr = pointer(*l, 3);
      REQUIRE(ctr && (l->replay ? ctr->ordinal >= 0 : ctr->ordinal == -1), "the step comes by value in eager launches, from the counter in a replay");
      std::ostringstream s;
      s << l->name << " grid " << l->grid[0];
      for (size_t i = 5; i < 12; ++i) s << " " << (l->params[i].size == 8 ? (long long)scalar<int64_t>(*l, i) : (long long)scalar<int>(*l, i));
      for (size_t i = 0; i < 3; ++i) {
        const FakeHipPtr* p = pointer(*l, i);
        s << " p" << i << "=" << (p ? p->offset : (size_t)-1) << "/" << (p ? p->size : 0);
      }
      lines.push_back(s.str());
    } else if (l->name.find("sg::peak::gather<") != std::string::npos) {
      REQUIRE(l->params.size() == 9, "parameters of " + l->name);
      if (l->params.size() != 9) continue;
      REQUIRE(scalar<int64_t>(*l, 4) == (int64_t)n && 1 << scalar<int>(*l, 5) == c.b->gw && scalar<int>(*l, 6) == c.nd &&
                  scalar<int>(*l, 7) == c.h->ncls && scalar<int64_t>(*l, 8) == (int64_t)c.h->md.ncube,
              "the scalars of " + l->name);
      REQUIRE((int64_t)c.h->md.ncube * c.h->ncls == c.ncells, "ncube * ncls is not the block's cells");
      const size_t vb = l->name.find("gather<float>") != std::string::npos ? 4 : 8;
      holds(*l, 0, n * 8, "val");
      holds(*l, 1, n * 4, "idx");
      holds(*l, 2, nvalues(c) * vb, "the caller's values", true);
      holds(*l, 3, nvalues(c) * 4, "the caller's samples", true);
    } else {
      error("a kernel of sg::peak:: the suite does not know: " + l->name);
    }
  }
  return lines;
}

size_t updates() { return launches_of("sg::peak::update<").size(); }
size_t gathers() { return launches_of("sg::peak::gather<").size(); }

int64_t taken(Ctx& c) {
  int64_t n = -1;
  REQUIRE(sg_peaks_samples(c.h, &n) == SG_OK, "sg_peaks_samples");
  return n;
}

// (a) one life; the update launches of its every = 1 part, for the comparison of the two modes
std::vector<std::string> life(const BlockDef& b, bool graphs) {
  setenv("SEIGEN_HIP_GRAPH", graphs ? "1" : "0", 1);
  Ctx c;
  REQUIRE(open_with_material(b, c), std::string("the block does not open: ") + sg_last_error(c.h));
  if (!c.h) return {};
  REQUIRE(dev_alloc(c, nvalues(c) * 8) && dev_alloc(c, nvalues(c) * 4), "the caller's buffers");
  REQUIRE((int)c.h->md.gw == b.gw, "the block's layout is not the family's");
  REQUIRE(c.h->graph_ok == graphs, "SEIGEN_HIP_GRAPH ignored");
  std::vector<double> hv(nvalues(c));
  std::vector<int32_t> hs(nvalues(c));
  auto ok = [&](int rc, const std::string& what) {
    if (rc != SG_OK) error(what + " returned " + std::to_string(rc) + ": " + sg_last_error(c.h));
    no_violations(what);
  };
  // nothing armed: no launch in a step, the getters say so
  fakehip_log_clear();
  ok(sg_step(c.h, 3), "sg_step with nothing armed");
  REQUIRE(launches_of("sg::peak::").empty() && taken(c) == 0, "a fresh handle has peak maps");
  REQUIRE(sg_get_peaks(c.h, 0, hv.data(), hs.data(), nvalues(c)) == SG_ERR_STATE, "sg_get_peaks with nothing armed");
  REQUIRE(sg_get_peaks_dev(c.h, 1, value_buf(c), 0, sample_buf(c), nvalues(c)) == SG_ERR_STATE, "sg_get_peaks_dev with nothing armed");
  REQUIRE(launches_of("sg::peak::").empty(), "a getter launched with nothing armed");
  fakehip_counts bare, armed, now;
  fakehip_get_counts(&bare);
  // every = 1, 16 samples: steps 1 + 5 + 10 end with the series
  uint64_t epoch = c.h->epoch;
  ok(sg_set_peaks(c.h, 3, 1, 16), "sg_set_peaks");
  fakehip_get_counts(&armed);
  REQUIRE(armed.allocs == bare.allocs + 5 && armed.bytes >= bare.bytes + 2 * node_words(c) * 12, "arming allocates val and idx per field and the counter");
  REQUIRE(c.h->epoch == epoch + 1 && taken(c) == 0, "arming bumps the epoch and starts the count");
  fakehip_log_clear();
  ok(sg_step(c.h, 1), "sg_step(1)");
  REQUIRE(updates() == 2 && taken(c) == 1, "one update launch per field in a sample step");
  ok(sg_step(c.h, 5), "sg_step(5)");
  ok(sg_step(c.h, 10), "sg_step(10)");
  REQUIRE(updates() == 32 && taken(c) == 16, std::to_string(updates()) + " update launches in 16 sample steps of two fields");
  // (the launches of a step: behind the spectra's place and before the injectors' - with only the maps armed, the last of the step)
  const std::vector<std::string> lines = audit(c);
  no_violations("in the steps");
  // beyond the series: nothing is launched, recorded or refused
  fakehip_log_clear();
  ok(sg_step(c.h, 3), "sg_step beyond the series");
  REQUIRE(updates() == 0 && taken(c) == 16, "a launch beyond the series");
  // the read-outs: through the host (two buffers of its own, one launch, freed again) and on the stream (one launch, nothing else)
  const State was = state_of(c);
  for (int field = 0; field < 2; ++field)
    for (int which = 1; which < 4; ++which) {
      fakehip_log_clear();
      fakehip_fail(FAKEHIP_ALLOC, -1);
      ok(sg_get_peaks(c.h, field, (which & 1) ? hv.data() : nullptr, (which & 2) ? hs.data() : nullptr, nvalues(c)), "sg_get_peaks");
      REQUIRE(gathers() == 1 && updates() == 0 && fakehip_calls(FAKEHIP_ALLOC) == ((which & 1) ? 1 : 0) + ((which & 2) ? 1 : 0), "sg_get_peaks: launches, allocations");
      audit(c);
      for (int dtype = 0; dtype < 2; ++dtype) {
        fakehip_log_clear();
        fakehip_fail(FAKEHIP_ALLOC, -1);
        fakehip_fail(FAKEHIP_COPY, -1);
        ok(sg_get_peaks_dev(c.h, field, (which & 1) ? value_buf(c) : nullptr, dtype, (which & 2) ? sample_buf(c) : nullptr, nvalues(c)), "sg_get_peaks_dev");
        REQUIRE(gathers() == 1 && fakehip_calls(FAKEHIP_ALLOC) == 0 && fakehip_calls(FAKEHIP_COPY) == 0, "sg_get_peaks_dev: one launch and nothing else");
        const auto g = launches_of("sg::peak::gather<");
        REQUIRE(g.size() == 1 && g[0]->name.find(dtype ? "gather<float>" : "gather<double>") != std::string::npos, "the gather's type");
        audit(c);
      }
    }
  fakehip_log_clear();
  ok(sg_get_peaks(c.h, 0, nullptr, nullptr, nvalues(c)), "sg_get_peaks without a buffer");
  ok(sg_get_peaks_dev(c.h, 0, nullptr, 0, nullptr, nvalues(c)), "sg_get_peaks_dev without a buffer");
  REQUIRE(fakehip_log().empty(), "a read-out without a buffer launched");
  fakehip_get_counts(&now);
  REQUIRE(same_counts(now, armed) && same(was, state_of(c)), "a read-out changed the handle or left something: " + show(now));
  // armed again with another every and one field: fresh maps, the count from zero; eager steps launch at the due steps only,
  // a replayed graph at every step (its threads exit at once in the others)
  epoch = c.h->epoch;
  ok(sg_set_peaks(c.h, 2, 2, 3), "arming again");
  fakehip_get_counts(&now);
  REQUIRE(now.allocs == bare.allocs + 3 && c.h->epoch == epoch + 1 && taken(c) == 0 && c.h->pk.clock.steps == 0, "arming again: " + show(now));
  REQUIRE(sg_get_peaks(c.h, 0, hv.data(), hs.data(), nvalues(c)) == SG_ERR_STATE, "the velocity is no longer selected");
  fakehip_log_clear();
  ok(sg_step(c.h, 5), "sg_step(5), every = 2");
  REQUIRE(taken(c) == 2 && updates() == (graphs ? 5u : 2u), std::to_string(updates()) + " update launches in five steps of every = 2");
  audit(c);
  ok(sg_step(c.h, 4), "sg_step(4), every = 2, across the end of the series");
  REQUIRE(taken(c) == 3, "the count stops at nsamples");
  // host-driven stages with sg_end_step
  ok(sg_set_peaks(c.h, 1, 1, 2), "arming the velocity");
  fakehip_log_clear();
  for (int k = 0; k < 3; ++k) {
    for (int st = 0; st < 6; ++st) ok(sg_run_stage(c.h, st, SG_REGION_ALL), "sg_run_stage");
    ok(sg_end_step(c.h), "sg_end_step");
  }
  REQUIRE(updates() == 2 && taken(c) == 2, "sg_end_step: a launch per sample step, none beyond the series");
  audit(c);
  // disarmed: everything freed
  epoch = c.h->epoch;
  ok(sg_set_peaks(c.h, 0, 0, 0), "disarming");
  fakehip_get_counts(&now);
  REQUIRE(now.allocs == bare.allocs && now.bytes == bare.bytes && c.h->epoch == epoch + 1 && taken(c) == 0, "disarming frees the maps: " + show(now));
  REQUIRE(sg_get_peaks_dev(c.h, 0, value_buf(c), 0, sample_buf(c), nvalues(c)) == SG_ERR_STATE, "disarmed");
  fakehip_log_clear();
  ok(sg_step(c.h, 2), "sg_step after disarming");
  REQUIRE(launches_of("sg::peak::").empty(), "a launch after disarming");
  close_block(c);
  no_violations("during sg_destroy");
  return lines;
}

// (b) what the calls refuse, with maps armed
void refusals(Ctx& c) {
  const State was = state_of(c);
  const size_t n = nvalues(c);
  double* const hv = nullptr;
  int64_t k = 0;
  watch_runtime();
  all_refused({
      sg_set_peaks(nullptr, 1, 1, 1), sg_get_peaks(nullptr, 0, hv, nullptr, n), sg_get_peaks_dev(nullptr, 0, value_buf(c), 0, sample_buf(c), n),
      sg_peaks_samples(nullptr, &k), sg_peaks_samples(c.h, nullptr), sg_set_peaks(c.h, -1, 1, 1), sg_set_peaks(c.h, 4, 1, 1),
      sg_set_peaks(c.h, 3, 0, 1), sg_set_peaks(c.h, 1, -2, 1), sg_set_peaks(c.h, 3, 1, 0), sg_set_peaks(c.h, 2, 1, -1),
      sg_set_peaks(c.h, 3, 1, (int64_t)1 << 31), sg_get_peaks(c.h, 2, hv, sample_buf(c), n), sg_get_peaks(c.h, -1, hv, sample_buf(c), n),
      sg_get_peaks(c.h, 0, hv, nullptr, n - 1), sg_get_peaks(c.h, 1, hv, nullptr, n + 1), sg_get_peaks(c.h, 0, hv, nullptr, 0),
      sg_get_peaks_dev(c.h, 2, value_buf(c), 0, sample_buf(c), n), sg_get_peaks_dev(c.h, 0, value_buf(c), 2, sample_buf(c), n),
      sg_get_peaks_dev(c.h, 0, value_buf(c), -1, sample_buf(c), n), sg_get_peaks_dev(c.h, 1, value_buf(c), 1, sample_buf(c), n - 1),
      sg_get_peaks_dev(c.h, 1, value_buf(c), 0, sample_buf(c), (size_t)c.ncells),
  });
  REQUIRE(same(was, state_of(c)), "a refused call changed the handle");
  no_violations("in the refusals");
}

struct Call {
  std::string name;
  std::function<int(Ctx&)> run;
};

// (c) a failure in every runtime call of `call`, behind `before`: the maps armed before it, their count and the epoch as they were
long sweep(Ctx& c, const Call& call, const std::function<int(Ctx&)>& before) {
  return sweep_in_place(c, call.run, before, [&]() { return state_of(c); },
                        [&](const State& was, const std::string& at) { REQUIRE(same(was, state_of(c)), at + ": the handle changed"); });
}

long sweeps(const BlockDef& b) {
  unsetenv("SEIGEN_HIP_GRAPH");
  Ctx c;
  REQUIRE(open_with_material(b, c), std::string("the block does not open: ") + sg_last_error(c.h));
  if (!c.h) return 0;
  REQUIRE(dev_alloc(c, nvalues(c) * 8) && dev_alloc(c, nvalues(c) * 4), "the caller's buffers");
  REQUIRE(sg_set_peaks(c.h, 3, 2, 5) == SG_OK && sg_step(c.h, 3) == SG_OK, "arming and stepping");
  g_where = std::string(b.name) + " refusals";
  refusals(c);
  long injected = 0;
  // the setter, with maps armed and stepped before it, and with none
  const std::function<int(Ctx&)> armed_before = [](Ctx& x) {
    if (int rc = sg_set_peaks(x.h, 3, 2, 5)) return rc;
    return sg_step(x.h, 3);
  };
  const std::function<int(Ctx&)> none_before = [](Ctx& x) { return sg_set_peaks(x.h, 0, 0, 0); };
  for (int what = 0; what < 4; ++what) {
    const Call set{"sg_set_peaks what " + std::to_string(what), [=](Ctx& x) { return sg_set_peaks(x.h, what, 1, 7); }};
    g_where = std::string(b.name) + " " + set.name + " sweep, maps armed before";
    injected += sweep(c, set, armed_before);
    g_where = std::string(b.name) + " " + set.name + " sweep, nothing armed before";
    injected += sweep(c, set, none_before);
  }
  // the getters, on stepped maps
  REQUIRE(armed_before(c) == SG_OK, "arming and stepping");
  std::vector<double> hv(nvalues(c));
  std::vector<int32_t> hs(nvalues(c));
  size_t calls = 0;
  for (int field = 0; field < 2; ++field)
    for (int which = 1; which < 4; ++which) {
      const size_t n = nvalues(c);
      double* const v = (which & 1) ? hv.data() : nullptr;
      int32_t* const s = (which & 2) ? hs.data() : nullptr;
      const Call get{"sg_get_peaks field " + std::to_string(field) + " buffers " + std::to_string(which), [=](Ctx& x) { return sg_get_peaks(x.h, field, v, s, n); }};
      g_where = std::string(b.name) + " " + get.name + " sweep";
      injected += sweep(c, get, nullptr);
      calls += 1;
      for (int dtype = 0; dtype < 2; ++dtype) {
        const Call dev{"sg_get_peaks_dev field " + std::to_string(field) + " buffers " + std::to_string(which) + (dtype ? " float" : " double"), [=](Ctx& x) {
                         return sg_get_peaks_dev(x.h, field, (which & 1) ? value_buf(x) : nullptr, dtype, (which & 2) ? sample_buf(x) : nullptr, n);
                       }};
        g_where = std::string(b.name) + " " + dev.name + " sweep";
        injected += sweep(c, dev, nullptr);
        calls += 1;
      }
    }
  g_where = b.name;
  std::printf("%s: %zu read-outs\n", b.name, calls);
  close_block(c);
  no_violations("during sg_destroy");
  return injected;
}

}  // namespace

static long peak_block(const BlockDef& b) {
  g_where = std::string(b.name) + " life, graph replay";
  const std::vector<std::string> replay = life(b, true);
  g_where = std::string(b.name) + " life, eager";
  const std::vector<std::string> eager = life(b, false);
  g_where = std::string(b.name) + " replay against eager";
  REQUIRE(!replay.empty() && replay.size() == eager.size(), "update launches: graph replay " + std::to_string(replay.size()) + ", SEIGEN_HIP_GRAPH=0 " + std::to_string(eager.size()));
  for (size_t i = 0; i < std::min(replay.size(), eager.size()); ++i)
    if (replay[i] != eager[i]) {
      error("update launch " + std::to_string(i) + " differs:\n    " + replay[i] + "\n    " + eager[i]);
      break;
    }
  const long injected = sweeps(b);
  unsetenv("SEIGEN_HIP_GRAPH");
  return injected;
}

int main() {
  const std::vector<std::string> kernels = fakehip_kernels();
  for (const std::string& k : kernels) std::printf("kernel: %s\n", k.c_str());
  std::printf("host_runtime_peaks: %zu kernel objects registered\n", kernels.size());
  run_suite("peaks", peak_block);
  if (g_errors) {
    std::printf("host_runtime_peaks: %d errors\n", g_errors);
    return 1;
  }
  std::printf("host_runtime_peaks: clean\n");
  return 0;
}
