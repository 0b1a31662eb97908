// Gauges of the C-ABI (sg_set_gauges / sg_get_gauges / sg_probe_gradient): the broken gradient of the velocity - or its
// divergence, curl or symmetric part - at physical points, recorded on the device by the sixth end-of-step hook (stages.cpp
// hooks; kernels_gauge.hip has the arithmetic), or evaluated once behind everything queued.  The points are located and their
// derivative rows tabulated on the host (hostlogic.hpp plan_gauges: locate_point, the rule of sg_locate_points); the tables are
// built in locals and moved into the handle once nothing can fail any more, as the receivers' are.
#include <stdexcept>

#include "handle.hpp"

// the tables both entry points share: the owned points' cells and rows and the block's J, uploaded into `t`
static int build_tables(sg_handle* h, const char* who, int64_t npts, const double* pts, int kind, int64_t capacity, GaugeTables& t,
                        GaugePlan& pl) {
  NodeGeom G;
  if (!G.init(&h->cfg, h->cfg.degree)) return fail(h, SG_ERR_ARG, std::string(who) + ": cell type");
  try {
    pl = plan_gauges(G, layout(h), h->re.kind, npts, pts, kind, capacity);
  } catch (const std::exception& e) {
    return fail(h, SG_ERR_ARG, std::string(who) + ": " + e.what());
  }
  t.npts = npts;
  t.nown = (int64_t)pl.row.size();
  t.kind = kind;
  t.ncomp = pl.ncomp;
  std::vector<double> J((size_t)h->ncls * 9);
  for (int k = 0; k < h->ncls; ++k)
    for (int r = 0; r < 3; ++r)
      for (int j = 0; j < 3; ++j) J[((size_t)k * 3 + r) * 3 + j] = h->md.Jinv[k][r][j];
  HIPCHECK(h, t.item.upload(pl.item.data(), pl.item.size()));
  HIPCHECK(h, t.lane.upload(pl.lane.data(), pl.lane.size()));
  HIPCHECK(h, t.cls.upload(pl.cls.data(), pl.cls.size()));
  HIPCHECK(h, t.D.upload(pl.D.data(), pl.D.size()));
  HIPCHECK(h, t.J.upload(J.data(), J.size()));
  const size_t tlen = (size_t)(capacity * t.nown * t.ncomp);
  if (t.trace.alloc(tlen) != hipSuccess) {
    (void)hipGetLastError();
    return fail(h, SG_ERR_NOMEM, std::string(who) + ": hipMalloc of the trace failed");
  }
  // (on the handle's stream: arm_hook waits for it, and the one-shot's launch is queued behind it there - a fill on the null
  // stream is not ordered against a non-blocking stream)
  HIPCHECK(h, hipMemsetAsync(t.trace.get(), 0, std::max<size_t>(tlen, 1) * sizeof(double), h->stream));
  t.row = std::move(pl.row);
  return SG_OK;
}

// One launch of the gauge kernel on `stream`: velocity `field` as it stands there at the owned points of `t`, into sample
// step / every - 1 of its trace when the step (by value, or *ctr + 1) is a sample step.
static int queue_launch(sg_handle* h, hipStream_t stream, const GaugeTables& t, int field, const int64_t* ctr, int64_t step, int64_t every,
                        int64_t capacity) {
  gauge::Args a;
  std::memset(&a, 0, sizeof(a));
  a.ctr = ctr;
  a.step = step;
  a.every = every;
  a.capacity = capacity;
  a.item = t.item.get();
  a.lane = t.lane.get();
  a.cls = t.cls.get();
  a.D = t.D.get();
  a.J = t.J.get();
  a.out = t.trace.get();
  a.nown = t.nown;
  a.ncomp = t.ncomp;
  a.kind = t.kind;
  a.dim = h->cfg.dim;
  a.nd = h->re.nd;
  a.gw = (int32_t)h->md.gw;
  if (launch_gauges(h->field.read(field), a, h->f32, stream) != 0) return fail(h, SG_ERR_DEVICE, "gauge launch failed");
  return SG_OK;
}

// the armed gauges' launch: u1 of the step that just ended
static int queue_gauges(sg_handle* h, hipStream_t stream, const int64_t* ctr, int64_t step) {
  const GaugeTables& t = h->gge;
  return queue_launch(h, stream, t, SG_FIELD_U, ctr, step, t.clock.every, t.clock.count);
}

// what both entry points refuse about the points and the kind
static int check_points(sg_handle* h, const char* who, int64_t npts, const double* pts, int kind) {
  if (npts < 0) return fail(h, SG_ERR_ARG, std::string(who) + ": npts must be >= 0");
  if (npts > 0 && !pts) return fail(h, SG_ERR_ARG, std::string(who) + ": no points");
  if (npts > 0 && (kind < 0 || kind > 3))
    return fail(h, SG_ERR_ARG, std::string(who) + ": kind is 0 (gradient), 1 (divergence), 2 (curl) or 3 (strain rate)");
  if (npts > 0 && grad_ncomp(h->cfg.dim, kind) == 0) return fail(h, SG_ERR_ARG, std::string(who) + ": no curl in one dimension");
  return SG_OK;
}

extern "C" {

int sg_set_gauges(sg_handle* h, int64_t npts, const double* pts, int kind, int64_t every, int64_t capacity, int32_t* owned) {
  if (!h) return SG_ERR_ARG;
  if (int rc = check_points(h, "sg_set_gauges", npts, pts, kind)) return rc;
  if (npts > 0 && every < 1) return fail(h, SG_ERR_ARG, "sg_set_gauges: every must be >= 1");
  if (npts > 0 && capacity < 0) return fail(h, SG_ERR_ARG, "sg_set_gauges: capacity must be >= 0");
  HIPCHECK(h, hipSetDevice(h->cfg.device));
  GaugeTables t;
  GaugePlan pl;
  if (npts > 0) {
    if (int rc = build_tables(h, "sg_set_gauges", npts, pts, kind, capacity, t, pl)) return rc;
    t.clock.every = every;
    t.clock.count = capacity;
    t.queue = queue_gauges;
  }
  if (int rc = arm_hook(h, h->gge, t, npts > 0)) return rc;
  if (owned && npts > 0) std::memcpy(owned, pl.own.data(), pl.own.size() * sizeof(int32_t));
  return SG_OK;
}

int sg_get_gauges(sg_handle* h, double* out, size_t nbytes, int64_t* nsamples) {
  if (!h || !nsamples) return SG_ERR_ARG;
  const GaugeTables& t = h->gge;
  const size_t want = (size_t)(t.clock.count * t.npts * t.ncomp) * sizeof(double);
  if (nbytes != want || (want > 0 && !out))
    return fail(h, SG_ERR_ARG, "sg_get_gauges: the buffer must hold capacity x npts x ncomp doubles (" + std::to_string(want) + " bytes)");
  HIPCHECK(h, hipSetDevice(h->cfg.device));
  HIPCHECK(h, sync_all(h));
  const int64_t n = t.npts > 0 ? t.clock.samples() : 0;
  std::vector<double> tr((size_t)(n * t.nown * t.ncomp));
  if (!tr.empty()) HIPCHECK(h, hipMemcpy(tr.data(), t.trace.get(), tr.size() * sizeof(double), hipMemcpyDeviceToHost));
  if (want > 0) std::memset(out, 0, want);
  for (int64_t j = 0; j < n; ++j)
    for (int64_t r = 0; r < t.nown; ++r)
      std::memcpy(out + (j * t.npts + t.row[(size_t)r]) * t.ncomp, tr.data() + (j * t.nown + r) * t.ncomp, (size_t)t.ncomp * sizeof(double));
  *nsamples = n;
  return SG_OK;
}

// The one-shot: the tables of these points in locals (a temporary "trace" of one sample among them), one launch behind
// everything queued, one blocking copy.  Nothing of the handle changes.
int sg_probe_gradient(sg_handle* h, int field, int kind, int64_t npts, const double* pts, double* host_out, size_t nbytes, int32_t* owned) {
  if (!h) return SG_ERR_ARG;
  if (field != SG_FIELD_U && field != SG_FIELD_UH) return fail(h, SG_ERR_ARG, "sg_probe_gradient: field is SG_FIELD_U or SG_FIELD_UH");
  if (kind < 0 || kind > 3) return fail(h, SG_ERR_ARG, "sg_probe_gradient: kind is 0 (gradient), 1 (divergence), 2 (curl) or 3 (strain rate)");
  if (int rc = check_points(h, "sg_probe_gradient", npts, pts, kind)) return rc;
  const int ncomp = grad_ncomp(h->cfg.dim, kind);
  if (ncomp == 0) return fail(h, SG_ERR_ARG, "sg_probe_gradient: no curl in one dimension");
  if (nbytes != (size_t)npts * (size_t)ncomp * sizeof(double) || (nbytes > 0 && !host_out))
    return fail(h, SG_ERR_ARG, "sg_probe_gradient: the buffer must hold npts x ncomp doubles");
  if (npts == 0) return SG_OK;
  HIPCHECK(h, hipSetDevice(h->cfg.device));
  GaugeTables t;
  GaugePlan pl;
  if (int rc = build_tables(h, "sg_probe_gradient", npts, pts, kind, 1, t, pl)) return rc;
  std::vector<double> got((size_t)(t.nown * ncomp));
  if (t.nown > 0) {
    if (int rc = join_second(h)) return rc;
    if (int rc = queue_launch(h, h->stream, t, field, nullptr, 1, 1, 1)) return rc;
    HIPCHECK(h, sync_all(h));
    HIPCHECK(h, hipMemcpy(got.data(), t.trace.get(), got.size() * sizeof(double), hipMemcpyDeviceToHost));
  }
  std::memset(host_out, 0, nbytes);
  for (int64_t r = 0; r < t.nown; ++r)
    std::memcpy(host_out + t.row[(size_t)r] * ncomp, got.data() + r * ncomp, (size_t)ncomp * sizeof(double));
  if (owned) std::memcpy(owned, pl.own.data(), pl.own.size() * sizeof(int32_t));
  return SG_OK;
}

}  // extern "C"
