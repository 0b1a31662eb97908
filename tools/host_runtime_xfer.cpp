// host_runtime_xfer.cpp - the suite of host_runtime_driver for the device transfers of libseigen_hip (devxfer.cpp and the host
// half of kernels_xfer.hip): `host_runtime_driver xfer`, tests/test_device_transfer_runtime.py.  On the four blocks of
// kSuiteBlocks (host_runtime_common.hpp)
//   (a) sg_get_field_dev, sg_set_field_dev and sg_get_spectrum_dev on whole fields and on ranges, both buffer types, a stress
//       into a block in symmetric storage, spectra armed and not armed: the return codes, the launches (kernel, grid within
//       its cap, LDS within a block's 64 KB - the plan of sg_xfer_plan), the write counts, the audit silent;
//   (b) what the calls refuse: SG_ERR_ARG without a call of the runtime and with the handle as it was;
//   (c) a failure injected into every runtime call of every one of those transfers: the error code, a message, nothing
//       leaked, storage mode and epoch as they were, a write counted only where the launch went out, and the same call
//       succeeding afterwards.
// (No kernel runs, so the word that reports an asymmetric stress stays zero: the second upload of that path is the GPU tests'.)
#include "host_runtime_common.hpp"

namespace {

int arm_spectra(Ctx& c, int nfreq) {
  const std::vector<double> w((size_t)8 * (nfreq > 0 ? nfreq : 1) * 2, 0.25);
  return sg_set_spectra(c.h, nfreq, nfreq > 0 ? 3 : 0, 1, 8, w.data(), w.data());
}

// the launches of namespace sg::xfer in the log
std::vector<const FakeHipLaunch*> xfer_launches() { return launches_of("sg::xfer::"); }

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
                         return set ? sg_set_field_dev(x.h, f, c0, k, x.buf(), dtype, nbytes) : sg_get_field_dev(x.h, f, c0, k, x.buf(), dtype, nbytes);
                       }});
        }
  for (int field = 0; field < 2; ++field)
    for (int dtype = 0; dtype < 2; ++dtype) {
      const int f = field ? SG_FIELD_S : SG_FIELD_U;
      const size_t nbytes = c.words(f) * (dtype ? 4 : 8);
      v.push_back({std::string("sg_get_spectrum_dev field ") + std::to_string(field) + (dtype ? " float" : " double"), -1, gw != 1 || dtype != 0, 0, n,
                   (int)(c.cell_words(f) / c.nd), 8, dtype ? 4 : 8, [=](Ctx& x) { return sg_get_spectrum_dev(x.h, field, 1, field, x.buf(), dtype, nbytes); }});
    }
  return v;
}

// (a) one clean call: return code, launches against the plan, write counts
void clean_call(Ctx& c, const Call& call) {
  const FieldState was = field_state_of(c);
  fakehip_log_clear();
  const int rc = call.run(c);
  REQUIRE(rc == SG_OK, "returned " + std::to_string(rc) + ": " + sg_last_error(c.h));
  const FieldState is = field_state_of(c);
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
  const FieldState was = field_state_of(c);
  const size_t nu = c.words(SG_FIELD_U) * 8, per = c.cell_words(SG_FIELD_U) * 8;
  void* const buf = c.buf();
  watch_runtime();
  all_refused({
      sg_get_field_dev(nullptr, 0, 0, c.ncells, buf, 0, nu),      sg_set_field_dev(nullptr, 0, 0, c.ncells, buf, 0, nu),
      sg_get_spectrum_dev(nullptr, 0, 0, 0, buf, 0, nu),          sg_get_field_dev(c.h, 0, 0, c.ncells, nullptr, 0, nu),
      sg_set_field_dev(c.h, 0, 0, c.ncells, nullptr, 0, nu),      sg_get_spectrum_dev(c.h, 0, 0, 0, nullptr, 0, nu),
      sg_get_field_dev(c.h, 4, 0, c.ncells, buf, 0, nu),          sg_set_field_dev(c.h, -1, 0, c.ncells, buf, 0, nu),
      sg_get_field_dev(c.h, 0, 0, c.ncells, buf, 2, nu),          sg_set_field_dev(c.h, 0, 0, c.ncells, buf, -1, nu),
      sg_get_field_dev(c.h, 0, 0, c.ncells, buf, 1, nu),          sg_set_field_dev(c.h, 0, 0, c.ncells, buf, 0, nu - 8),
      sg_get_field_dev(c.h, 0, 1, c.ncells, buf, 0, nu),          sg_set_field_dev(c.h, 0, -1, 2, buf, 0, 2 * per),
      sg_set_field_dev(c.h, 0, 0, -1, buf, 0, 0),                 sg_get_field_dev(c.h, 0, c.ncells, 1, buf, 0, per),
      sg_get_spectrum_dev(c.h, 2, 0, 0, buf, 0, nu),              sg_get_spectrum_dev(c.h, 0, 2, 0, buf, 0, nu),
      sg_get_spectrum_dev(c.h, 0, 0, 2, buf, 0, nu),              sg_get_spectrum_dev(c.h, 0, 0, 0, buf, 0, nu + 8),
      sg_get_spectrum_dev(c.h, 0, 0, 0, buf, 3, nu),
  });
  REQUIRE(same_fields(was, field_state_of(c)), "a refused call changed the handle");
  // an empty range moves nothing and is no error
  REQUIRE(sg_get_field_dev(c.h, 0, 3, 0, buf, 0, 0) == SG_OK && sg_set_field_dev(c.h, 0, 3, 0, buf, 1, 0) == SG_OK, "an empty range");
  REQUIRE(xfer_launches().empty() && same_fields(was, field_state_of(c)), "an empty range launched or counted a write");
  no_violations("in the refusals");
}

// (c) a failure in every runtime call of one transfer: storage mode and epoch as they were, and a write counted where, and
// only where, the launch that writes went out
long sweep(Ctx& c, const Call& call) {
  return sweep_in_place(c, call.run, nullptr, [&]() { return field_state_of(c); }, [&](const FieldState& was, const std::string& at) {
    const FieldState is = field_state_of(c);
    REQUIRE(same_but_versions(was, is), at + ": storage mode or epoch changed");
    const uint64_t out = call.writes >= 0 ? (call.kernel ? xfer_launches().size() : (is.ver[call.writes] - was.ver[call.writes])) : 0;
    for (int f = 0; f < 4; ++f) REQUIRE(is.ver[f] == was.ver[f] + (f == call.writes ? out : 0), at + ": write count of field " + std::to_string(f));
    REQUIRE(out <= 1, at + ": more than one write");
  });
}

}  // namespace

long xfer_block(const BlockDef& b) {
  g_where = b.name;
  Ctx c;
  REQUIRE(open_with_material(b, c) && dev_alloc(c, c.words(SG_FIELD_S) * sizeof(double)),   // (room for a stress field in double)
          std::string("the block does not open: ") + sg_last_error(c.h));
  if (!c.h || c.bufs.empty()) return 0;
  REQUIRE((int)c.h->md.gw == b.gw, "the block's layout is not the family's");
  int sym = -1;
  sg_get_sym(c.h, &sym);
  REQUIRE(sym == (b.gw != 1 ? 1 : 0), "storage mode of a fresh block");
  // spectra not armed: SG_ERR_STATE, nothing launched
  fakehip_log_clear();
  for (int field = 0; field < 2; ++field)
    REQUIRE(sg_get_spectrum_dev(c.h, field, 0, 0, c.buf(), 0, c.words(field ? SG_FIELD_S : SG_FIELD_U) * 8) == SG_ERR_STATE, "spectra not armed");
  REQUIRE(fakehip_log().empty(), "a launch without spectra");
  REQUIRE(arm_spectra(c, 2) == SG_OK, "sg_set_spectra");
  const std::vector<Call> all = calls(c);
  for (const Call& call : all) {
    g_where = std::string(b.name) + " " + call.name;
    clean_call(c, call);
  }
  g_where = std::string(b.name) + " refusals";
  refusals(c);
  long injected = 0;
  for (const Call& call : all) {
    g_where = std::string(b.name) + " " + call.name + " sweep";
    injected += sweep(c, call);
  }
  g_where = b.name;
  REQUIRE(arm_spectra(c, 0) == SG_OK, "disarming the spectra");
  REQUIRE(sg_get_spectrum_dev(c.h, 1, 0, 0, c.buf(), 0, c.words(SG_FIELD_S) * 8) == SG_ERR_STATE, "spectra disarmed");
  std::printf("%s: %zu transfers\n", b.name, all.size());
  close_block(c);
  no_violations("during sg_destroy");
  return injected;
}
