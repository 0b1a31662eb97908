// host_runtime_grad.cpp - the gradient of libseigen_hip (grad.cpp and the host half of kernels_grad.hip) on the CPU under ASan
// and UBSan over the HIP runtime double of tests/fake_hip: a program of its own, build_tools/host_runtime_grad (`make -C
// seigen_amd/csrc host-runtime-asan`; tests/test_grad_runtime.py), over the objects and the helpers of host_runtime_driver
// (host_runtime_common.hpp) - that program's kernel objects are a closed list, which these kernels are no part of.  It prints
// the kernel objects it registered, then on the four blocks of kSuiteBlocks
//   (a) sg_get_gradient_dev and sg_get_gradient of both velocity fields, every kind the dimension has, both buffer types, on
//       the whole block and on ranges: the return codes, the one launch of sg::grad:: with its kernel, grid, LDS and every
//       scalar against sg_gradient_plan, its pointers against the extents the kernel walks (the field's items, the caller's
//       range, the two tables), the tables built by the first call and by no later one, the host getter's buffer freed again,
//       fields, storage mode, write counts and epoch as they were;
//   (b) what the calls refuse: SG_ERR_ARG without a call of the runtime and with the handle as it was;
//   (c) a failure injected into every runtime call of both getters, with the tables built before and not: the error code, a
//       message, nothing leaked, the tables of the call before intact (or still none), and the same call succeeding afterwards.
// (No kernel runs: what the values are is the GPU tests' business.)
#include "host_runtime_common.hpp"

namespace {

// what a failed or refused call must leave as it was
struct State : FieldState {
  bool ready = false;
  const void *C = nullptr, *J = nullptr;
  int n1 = 0;
};
State state_of(const Ctx& c) {
  State s;
  static_cast<FieldState&>(s) = field_state_of(c);
  s.ready = c.h->grd.ready;
  s.C = c.h->grd.C.get();
  s.J = c.h->grd.J.get();
  s.n1 = c.h->grd.n1;
  return s;
}
bool same(const State& a, const State& b) { return same_fields(a, b) && a.ready == b.ready && a.C == b.C && a.J == b.J && a.n1 == b.n1; }

int ncomp_of(int dim, int kind) { return kind == 1 ? 1 : (kind == 2 ? (dim == 3 ? 3 : 1) : dim * dim); }

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
void holds(const FakeHipLaunch& l, size_t i, size_t bytes, const char* what) {
  const FakeHipPtr* p = pointer(l, i);
  if (!p) return error(std::string(what) + ": parameter " + std::to_string(i) + " of " + l.name + " is no device pointer");
  REQUIRE(p->ordinal >= 0, std::string(what) + " is null or in no live allocation");
  REQUIRE(p->ordinal < 0 || p->size - p->offset >= bytes, std::string(what) + " is shorter than the " + std::to_string(bytes) + " bytes the kernel walks");
}

struct Call {
  std::string name;
  bool host;
  int field, kind, dtype;
  int64_t cell0, ncells;
  std::function<int(Ctx&)> run;
};

std::vector<double>& host_buf() {
  static std::vector<double> b;
  return b;
}

std::vector<Call> calls(const Ctx& c) {
  std::vector<Call> v;
  const int gw = c.b->gw, d = c.dim;
  const int64_t n = c.ncells;
  // ranges: whole; start and end inside a cube; across the first group boundary where there is one
  std::vector<std::pair<int64_t, int64_t>> ranges = {{0, n}, {1, std::min<int64_t>(n - 2, 2 * c.h->ncls + 1)}};
  if (gw > 1 && n > (int64_t)gw * c.h->ncls + c.h->ncls + 2) ranges.push_back({(int64_t)gw * c.h->ncls - c.h->ncls - 1, 2 * c.h->ncls + 3});
  for (const auto& r : ranges)
    for (int f : {SG_FIELD_U, SG_FIELD_UH})
      for (int kind = 0; kind < 4; ++kind) {
        if (kind == 2 && d == 1) continue;
        const int64_t c0 = r.first, k = r.second;
        const size_t words = (size_t)k * c.nd * ncomp_of(d, kind);
        const std::string tail = " field " + std::to_string(f) + " kind " + std::to_string(kind) + " cells " + std::to_string(c0) + "+" + std::to_string(k);
        for (int dtype = 0; dtype < 2; ++dtype)
          v.push_back({"sg_get_gradient_dev" + tail + (dtype ? " float" : " double"), false, f, kind, dtype, c0, k,
                       [=](Ctx& x) { return sg_get_gradient_dev(x.h, f, kind, c0, k, x.buf(), dtype, words * (dtype ? 4 : 8)); }});
        if (f == SG_FIELD_U || kind == 0)
          v.push_back({"sg_get_gradient" + tail, true, f, kind, 0, c0, k,
                       [=](Ctx& x) { return sg_get_gradient(x.h, f, kind, c0, k, host_buf().data(), words * 8); }});
      }
  return v;
}

// the one launch of a call in the log against the plan and the extents the kernel walks
void audit(Ctx& c, const Call& call) {
  const auto ls = launches_of("sg::grad::");
  REQUIRE(ls.size() == 1, std::to_string(ls.size()) + " gradient launches");
  const int gw = c.b->gw, d = c.dim, nd = c.nd, ncls = c.h->ncls, ncomp = ncomp_of(d, call.kind);
  const int fb = c.b->dtype ? 4 : 8, cb = call.dtype ? 4 : 8;
  int64_t plan[6];
  REQUIRE(sg_gradient_plan(gw, ncls, nd, d, ncomp, fb, cb, call.cell0, call.ncells, plan) == SG_OK, "sg_gradient_plan");
  for (const FakeHipLaunch* l : ls) {
    const std::string want = std::string(gw == 1 ? "sg::grad::flat<" : "sg::grad::lanes<") + (fb == 4 ? "float, " : "double, ") + (cb == 4 ? "float>" : "double>");
    REQUIRE(l->name.find(want) != std::string::npos, "the kernel is " + l->name + ", not " + want);
    REQUIRE(l->grid[0] == (unsigned)plan[4] && l->grid[0] >= 1 && l->grid[0] <= SG_XFER_GRID_CAP && l->grid[1] == 1 && l->grid[2] == 1, "grid " + std::to_string(l->grid[0]));
    REQUIRE(l->block[0] == 256 && l->block[1] == 1 && l->block[2] == 1, "block");
    REQUIRE(l->lds == (size_t)plan[5] && l->lds <= 65536, "LDS bytes " + std::to_string(l->lds));
    REQUIRE(l->stream == (void*)c.h->stream, "not on the handle's stream");
    for (const FakeHipPtr& p : l->ptrs) REQUIRE(p.ordinal >= 0, "a device pointer that is null or in no live allocation");
    for (const FakeHipParam& p : l->params) REQUIRE(p.type.find("sg::") == std::string::npos, "a struct by value: " + p.type);
    REQUIRE(l->params.size() == 19, "parameters of " + l->name);
    if (l->params.size() != 19) continue;
    const int64_t item0 = scalar<int64_t>(*l, 4), units = scalar<int64_t>(*l, 5);
    const int slices = scalar<int>(*l, 8), nps = scalar<int>(*l, 9), pitch = scalar<int>(*l, 10), out_offset = scalar<int>(*l, 11);
    REQUIRE(item0 == plan[0] && slices == plan[3] && nps == plan[2], "item0, slices, nodes per slice are not the plan's");
    REQUIRE(units == (gw == 1 ? (call.ncells * nd + 255) / 256 : plan[1] * plan[3]), "units");
    REQUIRE(scalar<int64_t>(*l, 6) == call.cell0 && scalar<int64_t>(*l, 7) == call.ncells, "the range");
    REQUIRE(scalar<int>(*l, 12) == gw && scalar<int>(*l, 13) == ncls && scalar<int>(*l, 14) == nd && scalar<int>(*l, 15) == d &&
                scalar<int>(*l, 16) == ncomp && scalar<int>(*l, 17) == call.kind,
            "gw, ncls, nd, dim, ncomp, kind");
    const int n1 = scalar<int>(*l, 18);
    REQUIRE(n1 == (c.h->re.kind == KIND_TENSOR ? c.b->degree + 1 : 0) && n1 == c.h->grd.n1, "n1");
    REQUIRE((int64_t)slices * nps >= nd && (int64_t)(slices - 1) * nps < nd, "the slices do not cover the nodes once");
    if (gw > 1) {
      REQUIRE(pitch == gw + 1 && out_offset % 16 == 0 && out_offset >= nd * d * pitch * 8, "pitch, offset of the values' image");
      REQUIRE((size_t)out_offset + (size_t)nps * ncomp * pitch * 8 <= l->lds, "the images do not fit the launch's LDS");
      // the items the grid walks lie in the field: (item0 + nitems) blocks of nd * dim * gw words from its start
      holds(*l, 0, (size_t)(plan[0] + plan[1]) * nd * d * gw * fb, "the field");
      REQUIRE((plan[0] + plan[1]) * (int64_t)gw <= c.h->md.ncube_pad * ncls, "items beyond the layout");
    } else {
      holds(*l, 0, (size_t)(call.cell0 + call.ncells) * nd * d * fb, "the field");
    }
    const FakeHipPtr* fp = pointer(*l, 0);
    REQUIRE(fp && fp->offset == 0 && fp->size >= c.h->field_alloc[call.field] * fb, "parameter 0 is not the start of a field");
    holds(*l, 1, (size_t)call.ncells * nd * ncomp * cb, "the caller's buffer");
    holds(*l, 2, (size_t)(n1 ? n1 * n1 : d * nd * nd) * 8, "C");
    holds(*l, 3, (size_t)ncls * 9 * 8, "J");
    const FakeHipPtr *pc = pointer(*l, 2), *pj = pointer(*l, 3);
    REQUIRE(pc && pj && pc->offset == 0 && pj->offset == 0, "the tables");
  }
}

// (a) one clean call
void clean_call(Ctx& c, const Call& call, bool first) {
  const State was = state_of(c);
  fakehip_counts before_it, after;
  fakehip_get_counts(&before_it);
  fakehip_log_clear();
  fakehip_fail(FAKEHIP_ALLOC, -1);
  const int rc = call.run(c);
  REQUIRE(rc == SG_OK, "returned " + std::to_string(rc) + ": " + sg_last_error(c.h));
  const long allocs = fakehip_calls(FAKEHIP_ALLOC), copies = fakehip_calls(FAKEHIP_COPY);
  fakehip_get_counts(&after);
  const State is = state_of(c);
  REQUIRE(same_fields(was, is), "a gradient changed the storage mode, the epoch or a write count");
  REQUIRE(is.ready && is.C && is.J, "no tables behind a successful call");
  if (first) {
    REQUIRE(!was.ready && allocs == 2 + (call.host ? 1 : 0) && after.allocs == before_it.allocs + 2, "the first call builds the two tables");
  } else {
    REQUIRE(same(was, is), "a later call touched the tables");
    REQUIRE(allocs == (call.host ? 1 : 0) && copies == (call.host ? 1 : 0) && same_counts(before_it, after),
            "a later call allocates or copies: " + std::to_string(allocs) + " allocations, " + std::to_string(copies) + " copies");
  }
  audit(c, call);
  no_violations("in " + call.name);
}

// (b) what the calls refuse
void refusals(Ctx& c) {
  const State was = state_of(c);
  const int d = c.dim;
  const size_t per = (size_t)c.nd * d * d * 8, all = (size_t)c.ncells * per;
  void* const buf = c.buf();
  double* const hb = host_buf().data();
  watch_runtime();
  std::vector<int> rcs = {
      sg_get_gradient_dev(nullptr, 0, 0, 0, c.ncells, buf, 0, all), sg_get_gradient(nullptr, 0, 0, 0, c.ncells, hb, all),
      sg_get_gradient_dev(c.h, 0, 0, 0, c.ncells, nullptr, 0, all), sg_get_gradient(c.h, 0, 0, 0, c.ncells, nullptr, all),
      sg_get_gradient_dev(c.h, SG_FIELD_S, 0, 0, c.ncells, buf, 0, all), sg_get_gradient(c.h, SG_FIELD_SH, 0, 0, c.ncells, hb, all),
      sg_get_gradient_dev(c.h, 4, 0, 0, c.ncells, buf, 0, all), sg_get_gradient(c.h, -1, 0, 0, c.ncells, hb, all),
      sg_get_gradient_dev(c.h, 0, 4, 0, c.ncells, buf, 0, all), sg_get_gradient(c.h, 0, -1, 0, c.ncells, hb, all),
      sg_get_gradient_dev(c.h, 0, 0, 0, c.ncells, buf, 2, all), sg_get_gradient_dev(c.h, 0, 0, 0, c.ncells, buf, -1, all),
      sg_get_gradient_dev(c.h, 0, 0, 0, c.ncells, buf, 1, all), sg_get_gradient_dev(c.h, 0, 0, 0, c.ncells, buf, 0, all - 8),
      sg_get_gradient(c.h, 0, 0, 0, c.ncells, hb, all + 8), sg_get_gradient_dev(c.h, 0, 0, 1, c.ncells, buf, 0, all),
      sg_get_gradient_dev(c.h, 0, 0, -1, 2, buf, 0, 2 * per), sg_get_gradient(c.h, 0, 0, 0, -1, hb, 0),
      sg_get_gradient_dev(c.h, 0, 0, c.ncells, 1, buf, 0, per), sg_get_gradient(c.h, 0, 3, 0, c.ncells + 1, hb, all + per),
  };
  if (d == 1) {
    rcs.push_back(sg_get_gradient_dev(c.h, 0, 2, 0, c.ncells, buf, 0, all));
    rcs.push_back(sg_get_gradient(c.h, 0, 2, 0, c.ncells, hb, all));
  } else {
    rcs.push_back(sg_get_gradient_dev(c.h, 0, 1, 0, c.ncells, buf, 0, all));   // the divergence has one component
    rcs.push_back(sg_get_gradient(c.h, 0, 2, 0, c.ncells, hb, all));
  }
  all_refused(rcs);
  REQUIRE(same(was, state_of(c)), "a refused call changed the handle");
  // an empty range is no error: nothing is launched
  REQUIRE(sg_get_gradient_dev(c.h, 0, 0, 3, 0, buf, 1, 0) == SG_OK, "an empty range");
  REQUIRE(launches_of("sg::grad::").empty() && same(was, state_of(c)), "an empty range launched");
  no_violations("in the refusals");
}

// (c) a failure in every runtime call of `call`; tables = false: the handle has none when the call starts
long sweep(Ctx& c, const Call& call, bool tables) {
  std::function<int(Ctx&)> before;
  if (!tables) before = [](Ctx& x) {
    x.h->grd = GradTables();
    return (int)SG_OK;
  };
  return sweep_in_place(c, call.run, before, [&]() { return state_of(c); }, [&](const State& was, const std::string& at) {
    REQUIRE(same(was, state_of(c)), at + ": the handle changed");
    REQUIRE(was.ready == tables, at + ": the tables before the call");
  });
}

}  // namespace

static long grad_block(const BlockDef& b) {
  g_where = b.name;
  Ctx c;
  REQUIRE(open_with_material(b, c) && dev_alloc(c, c.words(SG_FIELD_S) * sizeof(double)),   // (room for a gradient in double)
          std::string("the block does not open: ") + sg_last_error(c.h));
  if (!c.h || c.bufs.empty()) return 0;
  host_buf().assign(c.words(SG_FIELD_S) + 64, 0.0);
  REQUIRE((int)c.h->md.gw == b.gw, "the block's layout is not the family's");
  REQUIRE(!c.h->grd.ready && !c.h->grd.C.get(), "a fresh handle has gradient tables");
  REQUIRE(sg_step(c.h, 2) == SG_OK, "stepping");
  const std::vector<Call> all = calls(c);
  bool first = true;
  for (const Call& call : all) {
    g_where = std::string(b.name) + " " + call.name;
    clean_call(c, call, first);
    first = false;
  }
  // between two stepping calls (graph replays where the block has them): again one launch, nothing else
  REQUIRE(sg_step(c.h, 8) == SG_OK, "stepping");
  g_where = std::string(b.name) + " between stepping calls";
  clean_call(c, all.front(), false);
  REQUIRE(sg_step(c.h, 8) == SG_OK, "stepping");
  g_where = std::string(b.name) + " refusals";
  refusals(c);
  long injected = 0;
  size_t k = 0;
  for (const Call& call : all) {
    // every call with its tables in place; every fifth one also on a handle without
    g_where = std::string(b.name) + " " + call.name + " sweep";
    injected += sweep(c, call, true);
    if (k++ % 5 == 0) {
      g_where = std::string(b.name) + " " + call.name + " sweep, no tables before";
      injected += sweep(c, call, false);
    }
  }
  g_where = b.name;
  std::printf("%s: %zu gradient calls\n", b.name, all.size());
  close_block(c);
  no_violations("during sg_destroy");
  return injected;
}

int main() {
  const std::vector<std::string> kernels = fakehip_kernels();
  for (const std::string& k : kernels) std::printf("kernel: %s\n", k.c_str());
  std::printf("host_runtime_grad: %zu kernel objects registered\n", kernels.size());
  run_suite("gradients", grad_block);
  if (g_errors) {
    std::printf("host_runtime_grad: %d errors\n", g_errors);
    return 1;
  }
  std::printf("host_runtime_grad: clean\n");
  return 0;
}
