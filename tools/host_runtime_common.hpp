// host_runtime_common.hpp - what the suites of host_runtime_driver share (host_runtime_driver.cpp: the life of a handle and the
// sweep over the C-ABI; host_runtime_xfer.cpp: the device transfers; host_runtime_frame.cpp: the frames): error reporting,
// the blocks and how one is opened and closed with nothing of the runtime left, snapshots of what a failed call must leave
// as it was, the refusal pattern, and the failure sweep on a live handle.  One program, so everything here is inline.
#pragma once
#include <functional>

#include "fake_hip.h"
#include "handle.hpp"

inline int g_errors = 0;
inline std::string g_where;
inline void error(const std::string& what) {
  g_errors += 1;
  std::printf("ERROR [%s] %s\n", g_where.c_str(), what.c_str());
  std::fflush(stdout);
}
#define REQUIRE(cond, msg)                                  \
  do {                                                      \
    if (!(cond)) error(std::string(msg) + "  (" #cond ")"); \
  } while (0)

// ---- the blocks ---------------------------------------------------------------------------------------------------------

struct BlockDef {
  const char* name;
  const char* path;   // SEIGEN_HIP_PATH, or null
  int dim, degree, n[3], diagonal, dtype, nbr_mask;
  bool own_stream;    // false: a stream of the caller's (sg_config::stream)
  Family family;
  int gw;             // the layout's group width (the feature suites check it)
};
// the blocks of the feature suites: 3-D MFMA, lane, tile f32, generic
inline const BlockDef kSuiteBlocks[] = {
    {"mfma-P4-f64", nullptr, 3, 4, {3, 2, 2}, 0, 0, 0, true, Family::Mfma, 16},
    {"lane-2d-P2", "lane", 2, 2, {9, 8, 1}, 0, 0, 0, true, Family::Lane, 64},
    {"tile-tri-P3-f32", nullptr, 2, 3, {7, 5, 1}, 0, 1, 0, true, Family::Tile2d, 16},
    {"generic-1d-P2", nullptr, 1, 2, {37, 1, 1}, 0, 0, 0, true, Family::Generic, 1},
};

struct Ctx {
  const BlockDef* b = nullptr;
  sg_handle* h = nullptr;
  sg_config cfg = {};            // what sg_create was handed
  hipStream_t user_stream = nullptr;
  std::vector<void*> bufs;       // the caller's device buffers: ghosts and send buffers; a feature suite's one buffer
  sg_info_t info = {};
  int dim = 0, nd = 0;
  int64_t ncells = 0;
  void* buf() const { return bufs.front(); }
  size_t words(int f) const { return (size_t)ncells * nd * (field_is_stress(f) ? dim * dim : dim); }
  size_t cell_words(int f) const { return words(f) / (size_t)ncells; }
};

inline sg_config config_of(const BlockDef& b, hipStream_t stream) {
  sg_config c;
  std::memset(&c, 0, sizeof(c));
  c.dim = b.dim;
  c.degree = b.degree;
  for (int a = 0; a < 3; ++a) {
    c.n[a] = b.n[a];
    c.h[a] = 0.5;
  }
  c.diagonal = b.diagonal;
  c.nbr_mask = b.nbr_mask;
  c.dtype = b.dtype;
  c.stream = (void*)stream;
  return c;
}

inline void* dev_alloc(Ctx& c, size_t nbytes) {
  void* p = nullptr;
  if (hipMalloc(&p, nbytes) != hipSuccess) return nullptr;
  std::memset(p, 0, nbytes);
  c.bufs.push_back(p);
  return p;
}

// sg_create (rc returned)
inline int create_block(const BlockDef& b, Ctx& c) {
  c.b = &b;
  if (b.path) setenv("SEIGEN_HIP_PATH", b.path, 1);
  else unsetenv("SEIGEN_HIP_PATH");
  if (!b.own_stream && !c.user_stream && hipStreamCreateWithPriority(&c.user_stream, hipStreamNonBlocking, 0) != hipSuccess) return SG_ERR_DEVICE;
  c.cfg = config_of(b, c.user_stream);
  const int rc = sg_create(&c.cfg, &c.h);
  if (rc != SG_OK) return rc;
  sg_get_info(c.h, &c.info);
  c.dim = c.info.dim;
  c.nd = c.info.nd;
  c.ncells = c.info.ncells;
  return SG_OK;
}
// ... then the caller's halo buffers on the sides with a neighbour
inline int open_block(const BlockDef& b, Ctx& c) {
  if (int rc = create_block(b, c)) return rc;
  for (int side = 0; side < 2 * b.dim; ++side)
    if ((b.nbr_mask >> side) & 1)
      for (int f = 0; f < 4; ++f) {
        size_t nb = 0;
        sg_halo_bytes(c.h, f, side, &nb);
        if (sg_halo_attach(c.h, f, side, dev_alloc(c, nb)) != SG_OK) return SG_ERR_ARG;
      }
  return SG_OK;
}
// ... and, in a feature suite, one material for all cells; the suite then takes its one device buffer (dev_alloc: c.buf())
inline bool open_with_material(const BlockDef& b, Ctx& c) {
  const double lam = 2.0, mu = 1.0;
  return open_block(b, c) == SG_OK && sg_set_params(c.h, 1.0, 1e-3, &lam, &mu, 0) == SG_OK;
}

// sg_destroy; last = false: another handle of the driver's is still alive, the counts are checked when that one goes
inline void close_block(Ctx& c, bool last = true) {
  if (c.h) sg_destroy(c.h);
  c.h = nullptr;
  for (void* p : c.bufs) (void)hipFree(p);
  c.bufs.clear();
  if (!last) {
    if (c.user_stream) (void)hipStreamDestroy(c.user_stream);
    c.user_stream = nullptr;
    return;
  }
  fakehip_counts n;
  fakehip_get_counts(&n);
  // a stream handed in through sg_config::stream stays the caller's: alive after sg_destroy, destroyed here
  REQUIRE(n.streams == (c.user_stream ? 1 : 0), "streams left after sg_destroy: " + std::to_string(n.streams));
  if (c.user_stream) (void)hipStreamDestroy(c.user_stream);
  c.user_stream = nullptr;
  REQUIRE(n.allocs == 0 && n.bytes == 0, "device allocations left after sg_destroy: " + std::to_string(n.allocs));
  REQUIRE(n.events == 0, "events left after sg_destroy: " + std::to_string(n.events));
  REQUIRE(n.graphs == 0 && n.execs == 0, "graphs left after sg_destroy");
  REQUIRE(n.pinned == 0, "pinned buffers left after sg_destroy");
  REQUIRE(n.capturing == 0, "a stream left capturing");
}

// ---- what the double saw ------------------------------------------------------------------------------------------------

inline void no_violations(const std::string& when) {
  for (size_t i = 0; i < fakehip_violations(); ++i) error("the runtime double objected " + when + ": " + fakehip_violation(i));
  fakehip_clear_violations();
}

inline bool same_counts(const fakehip_counts& a, const fakehip_counts& b) {
  return a.allocs == b.allocs && a.bytes == b.bytes && a.streams == b.streams && a.events == b.events && a.graphs == b.graphs &&
         a.execs == b.execs && a.pinned == b.pinned && a.capturing == b.capturing;
}
inline std::string show(const fakehip_counts& n) {
  return std::to_string(n.allocs) + " allocations, " + std::to_string(n.bytes) + " bytes, " + std::to_string(n.streams) + " streams, " +
         std::to_string(n.events) + " events, " + std::to_string(n.graphs) + "+" + std::to_string(n.execs) + " graphs, " +
         std::to_string(n.pinned) + " pinned, " + std::to_string(n.capturing) + " capturing";
}

// the kernel launches of the log whose name contains `part`
inline std::vector<const FakeHipLaunch*> launches_of(const char* part) {
  std::vector<const FakeHipLaunch*> r;
  for (const FakeHipLaunch& l : fakehip_log())
    if (l.op == 0 && l.name.find(part) != std::string::npos) r.push_back(&l);
  return r;
}

// the calls of the runtime, of every kind, since the injection was armed
inline long runtime_calls() {
  long reached = 0;
  for (int kind = 0; kind < FAKEHIP_NKINDS; ++kind) reached += fakehip_calls(kind);
  return reached;
}
// The refusal pattern: watch_runtime(), the calls, then all_refused(their return codes) - SG_ERR_ARG each, none reached the
// runtime; that the handle is as it was is the suite's to say, with its own snapshot.
inline void watch_runtime() {
  fakehip_fail(FAKEHIP_LAUNCH, -1);
  fakehip_log_clear();
}
inline void all_refused(const std::vector<int>& rcs) {
  for (size_t i = 0; i < rcs.size(); ++i) REQUIRE(rcs[i] == SG_ERR_ARG, "refusal " + std::to_string(i) + " returned " + std::to_string(rcs[i]));
  REQUIRE(runtime_calls() == 0 && fakehip_log().empty(), "a refused call reached the runtime");
}

// ---- what a transfer or a frame must leave as it was: storage mode, epoch, the fields' write counts ------------------------

struct FieldState {
  int sym = -1;
  uint64_t epoch = 0, ver[4] = {0, 0, 0, 0};
};
inline FieldState field_state_of(const Ctx& c) {
  FieldState s;
  sg_get_sym(c.h, &s.sym);
  s.epoch = c.h->epoch;
  for (int f = 0; f < 4; ++f) s.ver[f] = c.h->field.versions().v[f];
  return s;
}
inline bool same_but_versions(const FieldState& a, const FieldState& b) { return a.sym == b.sym && a.epoch == b.epoch; }
inline bool same_fields(const FieldState& a, const FieldState& b) {
  for (int f = 0; f < 4; ++f)
    if (a.ver[f] != b.ver[f]) return false;
  return same_but_versions(a, b);
}

// ---- the failure sweep on a live handle ---------------------------------------------------------------------------------

// For every kind of runtime call: count those of a clean `call`, then fail the k-th of them, every k.  `before` (may be
// empty) runs ahead of every counted or failed call and leaves the state the call is to find.  The failed call returns the
// kind's error code with a message and leaks nothing; `as_it_was(was, at)` is the suite's own check against
// `was = snapshot()`, taken before the call; the same call then succeeds.  Returns the number of failures injected.
template <class Snapshot, class AsItWas>
long sweep_in_place(Ctx& c, const std::function<int(Ctx&)>& call, const std::function<int(Ctx&)>& before, Snapshot snapshot, AsItWas as_it_was) {
  long injected = 0;
  for (int kind = 0; kind < FAKEHIP_NKINDS; ++kind) {
    if (before) REQUIRE(before(c) == SG_OK, "the call before failed");
    fakehip_fail(kind, -1);
    REQUIRE(call(c) == SG_OK, "the clean call failed");
    const long n = fakehip_calls(kind);
    for (long k = 0; k < n; ++k) {
      const std::string who = "kind " + std::to_string(kind) + ", k = " + std::to_string(k) + " of " + std::to_string(n);
      if (before) REQUIRE(before(c) == SG_OK, who + ": the call before failed");
      const auto was = snapshot();
      fakehip_counts before_it, after;
      fakehip_get_counts(&before_it);
      fakehip_log_clear();
      fakehip_fail(kind, k);
      const int rc = call(c);
      REQUIRE(fakehip_fired(), who + ": the failure was skipped");
      injected += 1;
      const std::string at = who + " (" + fakehip_fired_at() + ")";
      REQUIRE(rc == (kind == FAKEHIP_ALLOC ? SG_ERR_NOMEM : SG_ERR_DEVICE), at + ": returned " + std::to_string(rc));
      REQUIRE(sg_last_error(c.h)[0] != 0, at + ": no message");
      fakehip_get_counts(&after);
      REQUIRE(before_it.allocs == after.allocs && before_it.bytes == after.bytes && before_it.events == after.events &&
                  before_it.streams == after.streams && before_it.pinned == after.pinned && after.capturing == 0,
              at + ": something leaked");
      as_it_was(was, at);
      no_violations("in the failed call, " + at);
      fakehip_fail(kind, -1);
      REQUIRE(call(c) == SG_OK, at + ": the same call fails afterwards: " + sg_last_error(c.h));
    }
  }
  return injected;
}

// ---- the feature suites ---------------------------------------------------------------------------------------------------

long xfer_block(const BlockDef& b);    // host_runtime_xfer.cpp; the failures injected
long frame_block(const BlockDef& b);   // host_runtime_frame.cpp

// a suite over its blocks, with the library's defaults for storage mode and graph replay
inline void run_suite(const char* name, long (*block)(const BlockDef&)) {
  unsetenv("SEIGEN_HIP_SYM");
  unsetenv("SEIGEN_HIP_GRAPH");
  const int errors = g_errors;
  long injected = 0;
  for (const BlockDef& b : kSuiteBlocks) injected += block(b);
  std::printf("%s: %ld failures injected, %d errors\n", name, injected, g_errors - errors);
  std::fflush(stdout);
}
