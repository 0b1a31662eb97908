// Frames of the C-ABI (sg_get_frame_dev): one field rastered on a pixel lattice aligned with the block's cubes into a device
// buffer of the caller's, queued on the handle's stream (kernels_frame.hip; the lattice, the listed groups and the launch are
// hostlogic.hpp frame_plan, the weights frame_weights).  The tables of a specification live on the device with the handle
// (handle.hpp FrameTables), which keeps the last one's: they are built in locals and moved in behind the launch, once nothing
// can fail any more.
#include "handle.hpp"

// the specification as the cache compares it: what frame_plan ignores is zeroed
static sg_frame frame_key(const sg_frame& fr, int dim) {
  sg_frame k;
  std::memset(&k, 0, sizeof(k));
  for (int a = 0; a < dim; ++a) {
    k.fixed[a] = fr.fixed[a];
    if (fr.fixed[a]) k.at[a] = fr.at[a];
    else k.m[a] = fr.m[a];
  }
  return k;
}

static bool same_key(const sg_frame& a, const sg_frame& b) {
  for (int k = 0; k < 3; ++k)
    if (a.m[k] != b.m[k] || a.fixed[k] != b.fixed[k] || !(a.at[k] == b.at[k])) return false;
  return true;
}

static int build_tables(sg_handle* h, const FramePlan& p, const sg_frame& key, FrameTables& t) {
  const int Q = p.Q, nd = h->re.nd, d = h->cfg.dim;
  std::vector<int32_t> cls((size_t)Q), order, cstart((size_t)h->ncls + 1, 0);
  std::vector<double> xi((size_t)Q * d), phi((size_t)Q * nd);
  std::string err;
  if (!frame_weights(h->cfg, h->cfg.degree, p, cls.data(), xi.data(), phi.data(), &err)) return fail(h, SG_ERR_ARG, "sg_get_frame_dev: " + err);
  for (int k = 0; k < h->ncls; ++k) {
    for (int q = 0; q < Q; ++q)
      if (cls[(size_t)q] == k) order.push_back(q);
    cstart[(size_t)k + 1] = (int32_t)order.size();
  }
  FrameSpec s;
  std::memset(&s, 0, sizeof(s));
  s.ngroups = (int64_t)p.groups.size();
  s.units = p.units;
  s.ncube = h->md.ncube;
  for (int k = 0; k < 3; ++k) {
    s.n[k] = k < d ? h->cfg.n[k] : 1;
    s.m[k] = p.m[k];
    s.fixed[k] = p.fixed[k];
    s.layer[k] = p.layer[k];
  }
  s.Q = Q;
  s.nd = nd;
  s.ncls = h->ncls;
  s.gw = p.gw;
  s.dim = d;
  HIPCHECK(h, t.spec.upload(&s, 1));
  HIPCHECK(h, t.cls.upload(cls.data(), cls.size()));
  HIPCHECK(h, t.order.upload(order.data(), order.size()));
  HIPCHECK(h, t.cstart.upload(cstart.data(), cstart.size()));
  HIPCHECK(h, t.phi.upload(phi.data(), phi.size()));
  HIPCHECK(h, t.groups.upload(p.groups.data(), p.groups.size()));
  t.key = key;
  t.plan = p;
  t.ready = true;
  return SG_OK;
}

extern "C" {

int sg_get_frame_dev(sg_handle* h, int field, const sg_frame* fr, void* dev_out, int dtype, const int64_t stride[4], size_t nbytes) {
  if (!h || !fr || !dev_out || field < 0 || field > 3 || dtype < 0 || dtype > 1) return SG_ERR_ARG;
  const int d = h->cfg.dim, gw = (int)h->md.gw;
  // the plan of the handle's last specification is kept with its tables: listing the groups walks the frame's cubes
  const sg_frame key = frame_key(*fr, d);
  const bool cached = h->frm.ready && same_key(h->frm.key, key);
  FramePlan planned;
  if (!cached) planned = frame_plan(h->cfg, gw, h->ncls, *fr);
  const FramePlan& p = cached ? h->frm.plan : planned;
  if (!p.err.empty()) return fail(h, SG_ERR_ARG, "sg_get_frame_dev: " + p.err);
  const int ncomp = (int)(h->field_len[field] / (size_t)h->ncells / (size_t)h->re.nd);
  // the largest index touched, whether or not this block holds the frame's layer: the extents are every block's
  const int64_t ext[4] = {ncomp, p.P[2], p.P[1], p.P[0]};
  int64_t st[4], last = 0, run = 1;
  for (int k = 3; k >= 0; --k) {
    st[k] = stride ? stride[k] : run;
    run *= ext[k];
    if (st[k] < 0) return fail(h, SG_ERR_ARG, "sg_get_frame_dev: negative stride");
    if (st[k] != 0 && (ext[k] - 1) > (((int64_t)1 << 60) - last) / st[k]) return fail(h, SG_ERR_ARG, "sg_get_frame_dev: stride too large");
    last += (ext[k] - 1) * st[k];
  }
  if ((uint64_t)last >= (uint64_t)(nbytes / (dtype ? sizeof(float) : sizeof(double)))) return fail(h, SG_ERR_ARG, "sg_get_frame_dev: nbytes does not cover the frame");
  if (!p.owns || p.grid == 0) return SG_OK;   // another block's layer: nothing to launch
  HIPCHECK(h, hipSetDevice(h->cfg.device));
  if (int rc = join_second(h)) return rc;
  FrameTables fresh;
  if (!cached) {
    // another specification: a set-up path, which waits for whatever still reads the tables that will be replaced
    if (h->frm.ready) HIPCHECK(h, sync_all(h));
    if (int rc = build_tables(h, p, key, fresh)) return rc;
  }
  const FrameTables& t = cached ? h->frm : fresh;
  const FrameTablePtrs a{t.spec.get(), t.cls.get(), t.order.get(), t.cstart.get(), t.phi.get(), t.groups.get()};
  const int sym = (h->sym && field_is_stress(field)) ? 1 : 0;
  if (launch_frame(h->field.read(field), dev_out, a, gw, p.units, ncomp, sym, st, h->f32, dtype, (int)p.grid, h->stream) != 0)
    return fail(h, SG_ERR_DEVICE, "frame kernel launch failed");
  if (!cached) h->frm = std::move(fresh);
  return SG_OK;
}

}  // extern "C"
