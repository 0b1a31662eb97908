// Device transfers of the C-ABI (sg_get_field_dev / sg_set_field_dev / sg_get_spectrum_dev): fields and spectra between the
// block's layout and a device buffer of the caller's in the host layout [cell][node][comp], queued on the handle's stream
// (kernels_xfer.hip; the plan of a launch is hostlogic.hpp xfer_plan).  Nothing here touches host memory but the one word
// that tells whether a stress handed to symmetric storage was symmetric.
#include "handle.hpp"

// One transfer of `ncells` cells from `cell0` between `layout_buf` - a buffer in the layout of field `field`, float where
// buf_f32 - and the caller's `dev` (float where c32); dir = 0: dev -> layout_buf, 1: layout_buf -> dev.
static int queue_xfer(sg_handle* h, int field, void* layout_buf, int buf_f32, int dir, int64_t cell0, int64_t ncells, void* dev, int c32,
                      int sym, int* flag) {
  if (ncells == 0) return SG_OK;
  const int64_t per_cell = (int64_t)(h->field_len[field] / (size_t)h->ncells);
  const int ncomp = (int)(per_cell / h->re.nd);
  const int gw = (int)h->md.gw;
  const size_t fb = buf_f32 ? sizeof(float) : sizeof(double);
  if (gw == 1 && buf_f32 == c32) {   // the layouts and the types coincide
    char* const own = (char*)layout_buf + (size_t)cell0 * per_cell * fb;
    const size_t nb = (size_t)ncells * per_cell * fb;
    HIPCHECK(h, hipMemcpyAsync(dir == 0 ? (void*)own : dev, dir == 0 ? (const void*)dev : own, nb, hipMemcpyDeviceToDevice, h->stream));
    return SG_OK;
  }
  const XferPlan p = xfer_plan(gw, h->ncls, h->re.nd, ncomp, (int)fb, cell0, ncells);
  if (launch_xfer(gw, h->ncls, h->re.nd, ncomp, h->cfg.dim, dir, layout_buf, dev, cell0, ncells, sym, flag, buf_f32, c32, p.item0, p.units,
                  (int)p.slices, (int)p.rows_per_slice, (int)p.pitch, (int)p.grid, (size_t)p.lds_bytes, h->stream) != 0)
    return fail(h, SG_ERR_DEVICE, "transfer kernel launch failed");
  return SG_OK;
}

// the checks of sg_get_field_range, for a buffer of `dtype`
static int dev_range(sg_handle* h, int field, int64_t cell0, int64_t ncells, const void* dev, int dtype, size_t nbytes, const char* who) {
  if (!h || !dev || field < 0 || field > 3 || dtype < 0 || dtype > 1) return SG_ERR_ARG;
  if (cell0 < 0 || ncells < 0 || cell0 + ncells > h->ncells) return fail(h, SG_ERR_ARG, std::string(who) + ": cell range out of bounds");
  const size_t per_cell = h->field_len[field] / (size_t)h->ncells;
  if (nbytes != (size_t)ncells * per_cell * (dtype ? sizeof(float) : sizeof(double))) return fail(h, SG_ERR_ARG, std::string(who) + ": size mismatch");
  return SG_OK;
}

extern "C" {

int sg_get_field_dev(sg_handle* h, int field, int64_t cell0, int64_t ncells, void* dev_out, int dtype, size_t nbytes) {
  if (int rc = dev_range(h, field, cell0, ncells, dev_out, dtype, nbytes, "sg_get_field_dev")) return rc;
  HIPCHECK(h, hipSetDevice(h->cfg.device));
  if (int rc = join_second(h)) return rc;
  const int sym = (h->sym && field_is_stress(field)) ? 1 : 0;
  return queue_xfer(h, field, const_cast<double*>(h->field.read(field)), h->f32, 1, cell0, ncells, dev_out, dtype, sym, nullptr);
}

int sg_set_field_dev(sg_handle* h, int field, int64_t cell0, int64_t ncells, const void* dev_in, int dtype, size_t nbytes) {
  if (int rc = dev_range(h, field, cell0, ncells, dev_in, dtype, nbytes, "sg_set_field_dev")) return rc;
  HIPCHECK(h, hipSetDevice(h->cfg.device));
  if (int rc = join_second(h)) return rc;
  if (ncells == 0) return SG_OK;
  // (the field counts as written - Fields::write - once a launch that writes it is on the stream: a call that fails before
  // leaves the write counts as they were)
  void* const own = const_cast<double*>(h->field.read(field));
  void* const in = const_cast<void*>(dev_in);
  if (!(h->sym && field_is_stress(field))) {
    if (int rc = queue_xfer(h, field, own, h->f32, 0, cell0, ncells, in, dtype, 0, nullptr)) return rc;
    (void)h->field.write(field);
    return SG_OK;
  }
  // A stress into symmetric storage - the rule of sg_set_field (transfer.cpp transfer_staged): the upload reports any
  // asymmetry of the caller's data, the host waits and reads the word, and a non-symmetric stress makes every (i > j) line
  // of both stress buffers valid (they are stale wherever kernels ran in symmetric mode) and the upload run again in full mode.
  // The word is zero while the block is symmetric; it is cleared all the same, behind a call that failed after its launch.
  HIPCHECK(h, hipMemsetAsync(h->sym_flag.get(), 0, sizeof(int), h->stream));
  if (int rc = queue_xfer(h, field, own, h->f32, 0, cell0, ncells, in, dtype, 0, h->sym_flag.get())) return rc;
  (void)h->field.write(field);
  HIPCHECK(h, sync_all(h));
  int flag = 0;
  HIPCHECK(h, hipMemcpy(&flag, h->sym_flag.get(), sizeof(int), hipMemcpyDeviceToHost));
  if (!flag) return SG_OK;
  if (int rc = leave_sym_mode(h)) return rc;
  if (int rc = queue_xfer(h, field, own, h->f32, 0, cell0, ncells, in, dtype, 0, nullptr)) return rc;
  (void)h->field.write(field);
  return SG_OK;
}

int sg_get_spectrum_dev(sg_handle* h, int field, int freq, int part, void* dev_out, int dtype, size_t nbytes) {
  if (!h || !dev_out || dtype < 0 || dtype > 1) return SG_ERR_ARG;
  if (field < 0 || field > 1) return fail(h, SG_ERR_ARG, "sg_get_spectrum_dev: field is 0 (velocity) or 1 (stress)");
  const SpectraTables& sp = h->spc;
  if (!sp.has(field)) return fail(h, SG_ERR_STATE, "sg_get_spectrum_dev: no spectra armed for this field (sg_set_spectra)");
  if (freq < 0 || freq >= sp.nfreq) return fail(h, SG_ERR_ARG, "sg_get_spectrum_dev: frequency outside 0 .. nfreq - 1");
  if (part < 0 || part > 1) return fail(h, SG_ERR_ARG, "sg_get_spectrum_dev: part is 0 (re) or 1 (im)");
  const int f = field == 0 ? SG_FIELD_U : SG_FIELD_S;
  if (nbytes != h->field_len[f] * (dtype ? sizeof(float) : sizeof(double))) return fail(h, SG_ERR_ARG, "sg_get_spectrum_dev: size mismatch");
  HIPCHECK(h, hipSetDevice(h->cfg.device));
  if (int rc = join_second(h)) return rc;
  // an accumulator is a buffer in the field's layout, double whatever the block's type
  double* const acc = sp.acc[field].get() + (size_t)(2 * freq + part) * h->field_alloc[f];
  const int sym = (h->sym && field == 1) ? 1 : 0;
  return queue_xfer(h, f, acc, 0, 1, 0, h->ncells, dev_out, dtype, sym, nullptr);
}

}  // extern "C"
