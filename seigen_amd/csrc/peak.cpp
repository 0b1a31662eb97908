// Peak maps of the C-ABI (sg_set_peaks / sg_get_peaks / sg_get_peaks_dev / sg_peaks_samples): per node the running maximum
// of |u|^2 and of s:s over the samples of a run and the sample that reached it, kept on the device by the fifth end-of-step
// hook (stages.cpp hooks; kernels_peak.hip has the arithmetic) and read out in the caller's [cell][node] order.
#include "handle.hpp"

static const int kPeakFields[2] = {SG_FIELD_U, SG_FIELD_S};

// node words of a map: the field's device layout with one component
static size_t peak_words(const sg_handle* h) { return (size_t)h->md.ncube_pad * h->ncls * h->re.nd; }
static int peak_grid(const sg_handle* h) { return 8 * std::max(h->ncu, 1); }

// One launch of the update kernel per selected field on `stream`: the fields as they stand there against the maps when the
// step (by value, or *ctr + 1) is a sample step of the series.  The storage mode is the one of the launch: a block that has
// left symmetric storage is read by the full-storage formula from that step on.
static int queue_peaks(sg_handle* h, hipStream_t stream, const int64_t* ctr, int64_t step) {
  const PeakTables& pk = h->pk;
  const int dim = h->cfg.dim;
  for (int k = 0; k < 2; ++k) {
    if (!pk.has(k)) continue;
    const int ncomp = k == 1 ? dim * dim : dim;
    if (launch_peak_update(h->field.read(kPeakFields[k]), pk.val[k].get(), pk.idx[k].get(), ctr, step, pk.clock.every, pk.clock.count,
                           (int64_t)peak_words(h), (int)h->md.gw, ncomp, dim, (k == 1 && h->sym) ? 1 : 0, h->f32, peak_grid(h), stream) != 0)
      return fail(h, SG_ERR_DEVICE, "peak map launch failed");
  }
  return SG_OK;
}

// the checks both getters share; SG_OK: the maps of `field` are armed and nvalues fits
static int peak_readable(sg_handle* h, int field, size_t nvalues, const char* who) {
  if (field < 0 || field > 1) return fail(h, SG_ERR_ARG, std::string(who) + ": field is 0 (velocity) or 1 (stress)");
  if (!h->pk.has(field)) return fail(h, SG_ERR_STATE, std::string(who) + ": no peak maps armed for this field (sg_set_peaks)");
  if (nvalues != (size_t)h->ncells * h->re.nd) return fail(h, SG_ERR_ARG, std::string(who) + ": size mismatch");
  return SG_OK;
}

// the maps of `field` into device buffers in the caller's order, behind everything the handle has queued
static int queue_gather(sg_handle* h, int field, void* dev_value, int c32, int32_t* dev_sample) {
  if (int rc = join_second(h)) return rc;
  if (launch_peak_gather(h->pk.val[field].get(), h->pk.idx[field].get(), dev_value, c32, dev_sample, (int64_t)peak_words(h), (int)h->md.gw,
                         h->re.nd, h->ncls, (int64_t)h->md.ncube, peak_grid(h), h->stream) != 0)
    return fail(h, SG_ERR_DEVICE, "peak map gather launch failed");
  return SG_OK;
}

extern "C" {

// The maps are built in locals - allocated, then filled on the handle's stream, which arm_hook waits for - and moved into the
// handle once nothing can fail any more, as the spectra's accumulators are.
int sg_set_peaks(sg_handle* h, int what, int64_t every, int64_t nsamples) {
  if (!h) return SG_ERR_ARG;
  if (what < 0 || what > 3) return fail(h, SG_ERR_ARG, "sg_set_peaks: what must be 0 (disarm), 1 (velocity), 2 (stress) or 3");
  PeakTables pk;
  if (what != 0) {
    if (every < 1) return fail(h, SG_ERR_ARG, "sg_set_peaks: every must be >= 1");
    if (nsamples < 1 || nsamples > (int64_t)INT32_MAX) return fail(h, SG_ERR_ARG, "sg_set_peaks: nsamples must be 1 .. 2^31 - 1");
  }
  HIPCHECK(h, hipSetDevice(h->cfg.device));
  if (what != 0) {
    pk.what = what;
    pk.queue = queue_peaks;
    pk.clock.every = every;
    pk.clock.count = nsamples;
    const size_t n = peak_words(h);
    for (int k = 0; k < 2; ++k) {
      if (!pk.has(k)) continue;
      if (pk.val[k].alloc(n) != hipSuccess || pk.idx[k].alloc(n) != hipSuccess) {
        (void)hipGetLastError();
        return fail(h, SG_ERR_NOMEM, "sg_set_peaks: hipMalloc of the maps (" + std::to_string(n * 12) + " bytes a field) failed");
      }
    }
    for (int k = 0; k < 2; ++k) {
      if (!pk.has(k)) continue;
      // (0.0 is all bits zero, -1 all bits one; on the handle's stream, which the host waits for below)
      HIPCHECK(h, hipMemsetAsync(pk.val[k].get(), 0, n * sizeof(double), h->stream));
      HIPCHECK(h, hipMemsetAsync(pk.idx[k].get(), 0xff, n * sizeof(int32_t), h->stream));
    }
  }
  return arm_hook(h, h->pk, pk, what != 0);
}

int sg_get_peaks(sg_handle* h, int field, double* value, int32_t* sample, size_t nvalues) {
  if (!h) return SG_ERR_ARG;
  if (int rc = peak_readable(h, field, nvalues, "sg_get_peaks")) return rc;
  if (!value && !sample) return SG_OK;
  HIPCHECK(h, hipSetDevice(h->cfg.device));
  DevBuf<double> dv;
  DevBuf<int32_t> ds;
  if ((value && dv.alloc(nvalues) != hipSuccess) || (sample && ds.alloc(nvalues) != hipSuccess)) {
    (void)hipGetLastError();
    return fail(h, SG_ERR_NOMEM, "sg_get_peaks: hipMalloc of the read-out buffers failed");
  }
  if (int rc = queue_gather(h, field, value ? dv.get() : nullptr, 0, sample ? ds.get() : nullptr)) return rc;
  HIPCHECK(h, hipStreamSynchronize(h->stream));
  if (value) HIPCHECK(h, hipMemcpy(value, dv.get(), nvalues * sizeof(double), hipMemcpyDeviceToHost));
  if (sample) HIPCHECK(h, hipMemcpy(sample, ds.get(), nvalues * sizeof(int32_t), hipMemcpyDeviceToHost));
  return SG_OK;
}

int sg_get_peaks_dev(sg_handle* h, int field, void* dev_value, int dtype, int32_t* dev_sample, size_t nvalues) {
  if (!h || dtype < 0 || dtype > 1) return SG_ERR_ARG;
  if (int rc = peak_readable(h, field, nvalues, "sg_get_peaks_dev")) return rc;
  if (!dev_value && !dev_sample) return SG_OK;
  HIPCHECK(h, hipSetDevice(h->cfg.device));
  return queue_gather(h, field, dev_value, dtype, dev_sample);
}

int sg_peaks_samples(sg_handle* h, int64_t* taken) {
  if (!h || !taken) return SG_ERR_ARG;
  *taken = h->pk.what != 0 ? h->pk.clock.capped_samples() : 0;   // the maps run out: no more than nsamples
  return SG_OK;
}

}  // extern "C"
