// The gradient of the C-ABI (sg_get_gradient_dev / sg_get_gradient): the broken gradient of a velocity field at the nodes - or
// its divergence, curl or symmetric part - into a device buffer of the caller's, queued on the handle's stream
// (kernels_grad.hip; the plan of a launch is hostlogic.hpp grad_plan, the tables grad_dense_tables and the block's Jinv).  The
// tables live on the device with the handle (handle.hpp GradTables): the first call builds them in locals and moves them in
// behind its launch, once nothing can fail any more.
#include "handle.hpp"

static int build_tables(sg_handle* h, GradTables& t) {
  const int d = h->cfg.dim, nd = h->re.nd;
  const std::vector<double> dense = grad_dense_tables(h->re.kind, d, h->cfg.degree, h->re.lattice);
  if (h->re.kind == KIND_TENSOR) {
    // the 1-D derivative matrix: the line of the first nodes along axis 0 (hostlogic.hpp grad_dense_tables)
    const int n1 = h->cfg.degree + 1;
    std::vector<double> c1((size_t)n1 * n1);
    for (int a = 0; a < n1; ++a)
      for (int b = 0; b < n1; ++b) c1[(size_t)a * n1 + b] = dense[(size_t)a * nd + b];
    HIPCHECK(h, t.C.upload(c1.data(), c1.size()));
    t.n1 = n1;
  } else {
    HIPCHECK(h, t.C.upload(dense.data(), dense.size()));
    t.n1 = 0;
  }
  std::vector<double> J((size_t)h->ncls * 9);
  for (int k = 0; k < h->ncls; ++k)
    for (int r = 0; r < 3; ++r)
      for (int j = 0; j < 3; ++j) J[((size_t)k * 3 + r) * 3 + j] = h->md.Jinv[k][r][j];
  HIPCHECK(h, t.J.upload(J.data(), J.size()));
  t.ready = true;
  return SG_OK;
}

// the checks of both getters; *ncomp: the kind's components
static int grad_range(sg_handle* h, int field, int kind, int64_t cell0, int64_t ncells, const void* buf, int dtype, size_t nbytes,
                      const char* who, int* ncomp) {
  if (!h || !buf || dtype < 0 || dtype > 1) return SG_ERR_ARG;
  if (field != SG_FIELD_U && field != SG_FIELD_UH) return fail(h, SG_ERR_ARG, std::string(who) + ": field is SG_FIELD_U or SG_FIELD_UH");
  if (kind < 0 || kind > 3) return fail(h, SG_ERR_ARG, std::string(who) + ": kind is 0 (gradient), 1 (divergence), 2 (curl) or 3 (strain rate)");
  *ncomp = grad_ncomp(h->cfg.dim, kind);
  if (*ncomp == 0) return fail(h, SG_ERR_ARG, std::string(who) + ": no curl in one dimension");
  if (cell0 < 0 || ncells < 0 || cell0 + ncells > h->ncells) return fail(h, SG_ERR_ARG, std::string(who) + ": cell range out of bounds");
  if (nbytes != (size_t)ncells * (size_t)h->re.nd * (size_t)*ncomp * (dtype ? sizeof(float) : sizeof(double)))
    return fail(h, SG_ERR_ARG, std::string(who) + ": size mismatch");
  return SG_OK;
}

extern "C" {

int sg_get_gradient_dev(sg_handle* h, int field, int kind, int64_t cell0, int64_t ncells, void* dev_out, int dtype, size_t nbytes) {
  int ncomp = 0;
  if (int rc = grad_range(h, field, kind, cell0, ncells, dev_out, dtype, nbytes, "sg_get_gradient_dev", &ncomp)) return rc;
  if (ncells == 0) return SG_OK;
  const int gw = (int)h->md.gw, d = h->cfg.dim;
  const GradPlan p = grad_plan(gw, h->ncls, h->re.nd, d, ncomp, cell0, ncells);
  if (!p.ok) return fail(h, SG_ERR_ARG, "sg_get_gradient_dev: the item's velocity block leaves no room for a node's values in the LDS budget");
  HIPCHECK(h, hipSetDevice(h->cfg.device));
  if (int rc = join_second(h)) return rc;
  GradTables fresh;
  if (!h->grd.ready)
    if (int rc = build_tables(h, fresh)) return rc;
  const GradTables& t = h->grd.ready ? h->grd : fresh;
  GradArgs a;
  std::memset(&a, 0, sizeof(a));
  a.item0 = p.item0;
  a.units = p.units;
  a.cell0 = cell0;
  a.ncells = ncells;
  a.slices = (int32_t)p.slices;
  a.nodes_per_slice = (int32_t)p.nodes_per_slice;
  a.pitch = (int32_t)p.pitch;
  a.out_offset = (int32_t)p.out_offset;
  a.gw = gw;
  a.ncls = h->ncls;
  a.nd = h->re.nd;
  a.dim = d;
  a.ncomp = ncomp;
  a.kind = kind;
  a.n1 = t.n1;
  if (launch_grad(h->field.read(field), dev_out, t.C.get(), t.J.get(), a, h->f32, dtype, (int)p.grid, (size_t)p.lds_bytes, h->stream) != 0)
    return fail(h, SG_ERR_DEVICE, "gradient kernel launch failed");
  if (!h->grd.ready) h->grd = std::move(fresh);
  return SG_OK;
}

int sg_get_gradient(sg_handle* h, int field, int kind, int64_t cell0, int64_t ncells, double* host_out, size_t nbytes) {
  int ncomp = 0;
  if (int rc = grad_range(h, field, kind, cell0, ncells, host_out, 0, nbytes, "sg_get_gradient", &ncomp)) return rc;
  HIPCHECK(h, hipSetDevice(h->cfg.device));
  DevBuf<double> tmp;
  HIPCHECK(h, tmp.alloc(nbytes / sizeof(double)));
  const bool had_tables = h->grd.ready;
  if (int rc = sg_get_gradient_dev(h, field, kind, cell0, ncells, tmp.get(), 0, nbytes)) return rc;
  hipError_t e = sync_all(h);
  if (e == hipSuccess && nbytes) e = hipMemcpy(host_out, tmp.get(), nbytes, hipMemcpyDeviceToHost);
  if (e != hipSuccess) {
    // a call that fails leaves the handle as it was: the tables this call built go again (hipFree waits for the launch)
    if (!had_tables) h->grd = GradTables();
    return fail(h, SG_ERR_DEVICE, std::string("sg_get_gradient: the copy to the host: ") + hipGetErrorString(e));
  }
  return SG_OK;
}

}  // extern "C"
