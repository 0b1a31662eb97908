// host_runtime_frame.cpp - the suite of host_runtime_driver for the frames of libseigen_hip (frame.cpp and the host half of
// kernels_frame.hip): `host_runtime_driver frames`, tests/test_frame_runtime.py.  On the four blocks of kSuiteBlocks
// (host_runtime_common.hpp)
//   (a) sg_get_frame_dev of volumes and slices, velocity and stress, both buffer types, contiguous and strided: the return
//       code, the launch against sg_frame_plan (kernel, grid, no LDS, the handle's stream), fields, storage mode and epoch as
//       they were, the audit silent; a repeated specification allocates nothing, another one replaces the tables without a
//       leak; a slice of another block's layer launches nothing;
//   (b) what the call refuses: SG_ERR_ARG without a call of the runtime and with the handle as it was;
//   (c) a failure injected into every runtime call of every one of those frames, with the tables cached and not: the error
//       code, a message, nothing leaked, the handle - its cached tables included - as it was, and the same call succeeding
//       afterwards.
#include "host_runtime_common.hpp"

namespace {

// room for the largest frame below: 9 components, 64 pixels a cube, strided twice as wide, in double
size_t buf_bytes(const Ctx& c) { return (size_t)9 * 64 * c.b->n[0] * c.b->n[1] * c.b->n[2] * 2 * sizeof(double) + 64; }

// what a failed or refused call must leave as it was: fields, storage mode, epoch, and the cached tables
struct State : FieldState {
  bool ready = false;
  sg_frame key = {};
  const void* tables[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
};
State state_of(const Ctx& c) {
  State s;
  static_cast<FieldState&>(s) = field_state_of(c);
  const FrameTables& t = c.h->frm;
  s.ready = t.ready;
  s.key = t.key;
  const void* p[6] = {t.spec.get(), t.cls.get(), t.order.get(), t.cstart.get(), t.phi.get(), t.groups.get()};
  for (int k = 0; k < 6; ++k) s.tables[k] = p[k];
  return s;
}
bool same(const State& a, const State& b) {
  for (int k = 0; k < 6; ++k)
    if (a.tables[k] != b.tables[k]) return false;
  return same_fields(a, b) && a.ready == b.ready && std::memcmp(&a.key, &b.key, sizeof(sg_frame)) == 0;
}

std::vector<const FakeHipLaunch*> frame_launches() { return launches_of("sg::frame::"); }

sg_frame frame_of(int m0, int m1, int m2, int fixed_axis = -1, double at = 0.0) {
  sg_frame f;
  std::memset(&f, 0, sizeof(f));
  f.m[0] = m0;
  f.m[1] = m1;
  f.m[2] = m2;
  if (fixed_axis >= 0) {
    f.fixed[fixed_axis] = 1;
    f.at[fixed_axis] = at;
  }
  return f;
}

struct Call {
  std::string name;
  sg_frame fr;
  int field, dtype;
  bool strided;
  std::function<int(Ctx&)> run;
};

// the frames of a block (h = 1/2): volumes, and in 3-D slices inside a cube, on the interior grid plane and along x
std::vector<sg_frame> frames(const Ctx& c) {
  if (c.dim == 1) return {frame_of(4, 1, 1), frame_of(8, 1, 1)};
  if (c.dim == 2) return {frame_of(2, 3, 1), frame_of(1, 1, 1), frame_of(8, 8, 1), frame_of(3, 1, 1, 1, 1.3)};
  return {frame_of(2, 2, 2), frame_of(4, 4, 4), frame_of(2, 3, 1, 2, 0.2), frame_of(8, 8, 1, 2, 0.5), frame_of(1, 2, 3, 0, 1.25)};
}

std::vector<Call> calls(const Ctx& c) {
  std::vector<Call> v;
  int64_t plan[12];
  for (const sg_frame& fr : frames(c))
    for (int f : {SG_FIELD_U, SG_FIELD_S, SG_FIELD_SH})
      for (int dtype = 0; dtype < 2; ++dtype)
        for (int strided = 0; strided < 2; ++strided) {
          if (sg_frame_plan(&c.cfg, &fr, plan) != SG_OK) {
            error("sg_frame_plan refuses a frame of the list");
            continue;
          }
          const int ncomp = field_is_stress(f) ? c.dim * c.dim : c.dim;
          // strided: rows twice as long as the frame's, the component stride to match
          const int64_t P0 = plan[0], P1 = plan[1], P2 = plan[2];
          const int64_t st[4] = {2 * P0 * P1 * P2, 2 * P0 * P1, 2 * P0, 1};
          const size_t words = (size_t)ncomp * P0 * P1 * P2 * (strided ? 2 : 1);
          const size_t nbytes = words * (dtype ? 4 : 8);
          const std::string name = "frame m " + std::to_string(fr.m[0]) + "," + std::to_string(fr.m[1]) + "," + std::to_string(fr.m[2]) + " fixed " +
                                   std::to_string(fr.fixed[0]) + std::to_string(fr.fixed[1]) + std::to_string(fr.fixed[2]) + " field " + std::to_string(f) +
                                   (dtype ? " float" : " double") + (strided ? " strided" : "");
          v.push_back({name, fr, f, dtype, strided != 0, [=](Ctx& x) {
                         if (nbytes > buf_bytes(x)) return -100;
                         return sg_get_frame_dev(x.h, f, &fr, x.buf(), dtype, strided ? st : nullptr, nbytes);
                       }});
        }
  return v;
}

// (a) one clean call: return code, the launch against the plan, the handle's fields untouched
void clean_call(Ctx& c, const Call& call) {
  const State was = state_of(c);
  fakehip_log_clear();
  fakehip_fail(FAKEHIP_ALLOC, -1);
  const int rc = call.run(c);
  const long allocs = fakehip_calls(FAKEHIP_ALLOC);
  REQUIRE(rc == SG_OK, "returned " + std::to_string(rc) + ": " + sg_last_error(c.h));
  const State is = state_of(c);
  REQUIRE(same_fields(was, is), "a frame changed a field's write count, the storage mode or the epoch");
  int64_t plan[12];
  REQUIRE(sg_frame_plan(&c.cfg, &call.fr, plan) == SG_OK, "sg_frame_plan");
  REQUIRE(plan[11] == c.b->gw, "the plan's group width is not the block's");
  const auto ls = frame_launches();
  REQUIRE(ls.size() == (plan[4] ? 1u : 0u), std::to_string(ls.size()) + " frame launches");
  const int ncomp = field_is_stress(call.field) ? c.dim * c.dim : c.dim;
  for (const FakeHipLaunch* l : ls) {
    REQUIRE(l->name.find(c.b->gw == 1 ? "sg::frame::flat<" : "sg::frame::lanes<") != std::string::npos, "the kernel is " + l->name);
    const std::string types = std::string(c.b->dtype ? "<float, " : "<double, ") + (call.dtype ? "float>" : "double>");
    REQUIRE(l->name.find(types) != std::string::npos, "the kernel is " + l->name + ", not " + types);
    REQUIRE(l->grid[0] == (unsigned)plan[10] && l->grid[0] >= 1 && l->grid[0] <= SG_FRAME_GRID_CAP && l->grid[1] == (unsigned)ncomp && l->grid[2] == 1,
            "grid " + std::to_string(l->grid[0]) + " x " + std::to_string(l->grid[1]));
    REQUIRE(l->block[0] == 256 && l->block[1] == 1, "block");
    REQUIRE(l->lds == 0, "LDS bytes " + std::to_string(l->lds));
    REQUIRE(l->stream == (void*)c.h->stream, "not on the handle's stream");
    REQUIRE(l->ptrs.size() == 7 || l->ptrs.size() == 6, "device pointers among the arguments: " + std::to_string(l->ptrs.size()));
    for (const FakeHipPtr& p : l->ptrs) REQUIRE(p.ordinal >= 0, "a device pointer that is null or in no live allocation");
  }
  if (plan[4]) {
    REQUIRE(is.ready && c.h->frm.spec.get() != nullptr, "no tables cached behind a launch");
    // the same specification again: the cached tables, no allocation
    const bool cached = was.ready && same(was, is);
    REQUIRE(cached ? allocs == 0 : allocs == 6, std::to_string(allocs) + " allocations");
    fakehip_fail(FAKEHIP_ALLOC, -1);
    fakehip_fail(FAKEHIP_COPY, -1);
    REQUIRE(call.run(c) == SG_OK, "the repeated call failed");
    REQUIRE(fakehip_calls(FAKEHIP_COPY) == 0, "the repeated call copied");
    fakehip_fail(FAKEHIP_ALLOC, -1);
    REQUIRE(call.run(c) == SG_OK && fakehip_calls(FAKEHIP_ALLOC) == 0, "the repeated call allocated");
    REQUIRE(same(is, state_of(c)), "the repeated call changed the handle");
  } else {
    REQUIRE(same(was, is) && allocs == 0, "a frame of another block's layer touched the handle");
  }
  no_violations("in " + call.name);
}

// (b) what the call refuses
void refusals(Ctx& c) {
  const State was = state_of(c);
  const sg_frame ok = c.dim == 1 ? frame_of(2, 1, 1) : frame_of(2, 2, c.dim == 3 ? 2 : 1);
  int64_t plan[12];
  REQUIRE(sg_frame_plan(&c.cfg, &ok, plan) == SG_OK, "sg_frame_plan");
  const size_t nb = (size_t)c.dim * plan[0] * plan[1] * plan[2] * 8, all = buf_bytes(c);
  void* const buf = c.buf();
  sg_frame m9 = ok, m0 = ok, q65 = frame_of(8, c.dim > 1 ? 8 : 1, c.dim > 2 ? 2 : 1), none = ok, bad_fixed = ok, nan_at = ok;
  m9.m[0] = 9;
  m0.m[0] = 0;
  for (int a = 0; a < c.dim; ++a) none.fixed[a] = 1;
  bad_fixed.fixed[0] = 2;
  nan_at.fixed[0] = 1;
  nan_at.at[0] = std::nan("");
  const int64_t neg[4] = {plan[0] * plan[1] * plan[2], plan[0] * plan[1], plan[0], -1};
  const int64_t wide[4] = {plan[0] * plan[1] * plan[2], plan[0] * plan[1], plan[0], 2};
  watch_runtime();
  std::vector<int> rcs = {
      sg_get_frame_dev(nullptr, 0, &ok, buf, 0, nullptr, nb), sg_get_frame_dev(c.h, 0, nullptr, buf, 0, nullptr, nb),
      sg_get_frame_dev(c.h, 0, &ok, nullptr, 0, nullptr, nb), sg_get_frame_dev(c.h, 4, &ok, buf, 0, nullptr, nb),
      sg_get_frame_dev(c.h, -1, &ok, buf, 0, nullptr, nb),    sg_get_frame_dev(c.h, 0, &ok, buf, 2, nullptr, nb),
      sg_get_frame_dev(c.h, 0, &ok, buf, -1, nullptr, nb),    sg_get_frame_dev(c.h, 0, &ok, buf, 0, nullptr, nb - 8),
      sg_get_frame_dev(c.h, 0, &ok, buf, 0, nullptr, 0),      sg_get_frame_dev(c.h, 1, &ok, buf, 1, nullptr, nb / 2 - 4),
      sg_get_frame_dev(c.h, 0, &m9, buf, 0, nullptr, all),    sg_get_frame_dev(c.h, 0, &m0, buf, 0, nullptr, all),
      sg_get_frame_dev(c.h, 0, &none, buf, 0, nullptr, all),  sg_get_frame_dev(c.h, 0, &bad_fixed, buf, 0, nullptr, all),
      sg_get_frame_dev(c.h, 0, &nan_at, buf, 0, nullptr, all), sg_get_frame_dev(c.h, 0, &ok, buf, 0, neg, nb),
      sg_get_frame_dev(c.h, 0, &ok, buf, 0, wide, nb),
  };
  if (c.dim == 3) rcs.push_back(sg_get_frame_dev(c.h, 0, &q65, buf, 0, nullptr, all));
  // (a stress has dim^2 components: the bytes of a velocity do not hold it)
  if (c.dim > 1) rcs.push_back(sg_get_frame_dev(c.h, 2, &ok, buf, 0, nullptr, nb));
  all_refused(rcs);
  REQUIRE(same(was, state_of(c)), "a refused call changed the handle");
  // another block's layer: no error, no launch, no call of the runtime - but the bounds are still checked
  const sg_frame far = frame_of(2, 2, 2, c.dim - 1, 77.0);
  if (c.dim > 1) {
    watch_runtime();
    REQUIRE(sg_get_frame_dev(c.h, 0, &far, buf, 0, nullptr, all) == SG_OK, "a slice outside the block");
    REQUIRE(sg_get_frame_dev(c.h, 0, &far, buf, 0, nullptr, 8) == SG_ERR_ARG, "a slice outside the block, nbytes too small");
    REQUIRE(runtime_calls() == 0 && fakehip_log().empty() && same(was, state_of(c)), "a slice outside the block reached the runtime");
  }
  no_violations("in the refusals");
}

// (c) a failure in every runtime call of one frame, with the tables of `other` cached (a miss) or its own (a hit): the handle,
// its cached tables included, as it was
long sweep(Ctx& c, const Call& call, const Call* other) {
  return sweep_in_place(c, call.run, (other ? *other : call).run, [&]() { return state_of(c); },
                        [&](const State& was, const std::string& at) { REQUIRE(same(was, state_of(c)), at + ": the handle changed"); });
}

}  // namespace

long frame_block(const BlockDef& b) {
  g_where = b.name;
  Ctx c;
  REQUIRE(open_with_material(b, c) && dev_alloc(c, buf_bytes(c)), std::string("the block does not open: ") + sg_last_error(c.h));
  if (!c.h || c.bufs.empty()) return 0;
  REQUIRE((int)c.h->md.gw == b.gw, "the block's layout is not the family's");
  REQUIRE(!c.h->frm.ready, "a fresh handle has frame tables");
  const std::vector<Call> all = calls(c);
  for (const Call& call : all) {
    g_where = std::string(b.name) + " " + call.name;
    clean_call(c, call);
  }
  g_where = std::string(b.name) + " refusals";
  refusals(c);
  long injected = 0;
  for (size_t i = 0; i < all.size(); ++i) {
    g_where = std::string(b.name) + " " + all[i].name + " sweep, tables cached";
    injected += sweep(c, all[i], nullptr);
    // ... and with another specification's tables in the handle: the last call of the list before this frame's first
    const Call& other = all[(i + all.size() - 12) % all.size()];
    if (std::memcmp(&other.fr, &all[i].fr, sizeof(sg_frame)) != 0 && i % 12 < 2) {
      g_where = std::string(b.name) + " " + all[i].name + " sweep, another frame's tables cached";
      injected += sweep(c, all[i], &other);
    }
  }
  g_where = b.name;
  std::printf("%s: %zu frames\n", b.name, all.size());
  close_block(c);
  no_violations("during sg_destroy");
  return injected;
}
