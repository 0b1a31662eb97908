// Stage launches of the C-ABI: the choice of a stage's kernel, regions of a split stage, the six fused launches of an LF4 step
// (seigen/elastic.py:283-313), hipGraph replay, un-fused operator applications, halo packs, timing.
#include <array>

#include "handle.hpp"

// ---- stage launches --------------------------------------------------------------------

// What a launch is queued with, as a value that its caller builds and every function below is handed: nothing on the handle
// says "a capture is under way", so nothing has to be put back afterwards.
struct LaunchCtx {
  hipStream_t stream;                 // the stream of this launch and of what belongs to it (pre-pass, source)
  bool capture_src = false;           // a capture: slice and weight of the source come from the device-side counter src_ctr_d ...
  bool capture = false;               // ... and the step of every armed end-of-step hook from its own counter (StepSeries::ctr)
};

// the source at the handle's step (hostlogic.hpp source_slice), with the device pointers of a capture's SrcStep
struct SourceNow {
  SourceSlice at;
  const double* values;
  SrcStep stepper;
};
static SourceSlice source_at(const sg_handle* h, bool capture) {
  const SourceTables& src = h->src;
  return source_slice({src.nnz, src.nsteps, src.is_static, src.weights.empty() ? nullptr : src.weights.data(), h->cfg.dim}, h->src_step,
                      capture);
}
static SourceNow source_now(const sg_handle* h, const LaunchCtx& ctx) {
  SourceNow sn;
  sn.at = source_at(h, ctx.capture_src);
  sn.values = h->src.values.get() + sn.at.offset;
  std::memset(&sn.stepper, 0, sizeof(sn.stepper));
  if (ctx.capture_src) {
    sn.stepper.ctr = h->src_ctr_d.get();
    sn.stepper.nsteps = sn.at.nsteps;
    sn.stepper.stride = sn.at.stride;
    sn.stepper.weights = sn.at.use_weights ? h->src.weights_d.get() : nullptr;
    sn.stepper.is_static = sn.at.is_static ? 1 : 0;
  }
  return sn;
}

// the arguments of a stage launch (kernels.hpp StageArgs) but for the region's boxes and items and the output (run_op)
static int stage_args(sg_handle* h, const LaunchCtx& ctx, StageArgs& a, const StageOp& op, int region) {
  const int kind = op.kind;
  if (kind != 0 && kind != 1) return fail(h, SG_ERR_ARG, "unknown stage");
  std::memset(&a, 0, sizeof(a));
  a.in = h->field.read(op.in);
  a.aux = op.aux >= 0 ? h->field.read(op.aux) : nullptr;
  a.uabs = h->field.read(op.uabs);
  for (int s = 0; s < 6; ++s) {
    a.ghost[s] = h->ghost[op.in][s];
    // required for interior launches too: masked boundary lanes still form (and load through) the pointer
    if (h->md.has_nbr[s] && !a.ghost[s])
      return fail(h, SG_ERR_STATE, "stage needs a halo buffer that was not attached (sg_halo_attach)");
  }
  a.Dt = h->Dt.get();
  a.Lt = h->Lt.get();
  a.md = h->md_dev.get();
  a.mk = h->mk_dev.get();
  a.ftab = h->ftab_dev.get();
  a.nbr_tab = h->nbr_tab.get();
  a.all_active = region == SG_REGION_ALL ? 1 : 0;
  a.tensor = h->re.kind == KIND_TENSOR ? 1 : 0;
  a.fragV = (kind == 0) ? h->fragF.get() : h->fragG.get();
  a.fragL = h->fragL.get();
  if (kind == 1 && h->fragQ.get()) {      // G stages with the factorised volume term
    a.fragV = h->fragP.get();
    a.fragQ = h->fragQ.get();
    a.gstash = h->gstash ? 1 : 0;
  }
  a.sym = h->sym ? 1 : 0;
  a.f32 = h->f32;
  const SpongeTables& sp = h->sponge;
  a.dbg = h->dbg.get() ? h->dbg.get() + 8 * (kind * 2 + (op.mode ? 1 : 0)) : nullptr;
  a.sponge_slot = (kind == 0) ? sp.slot.get() : nullptr;
  a.sponge_B = sp.B.get();
  a.sponge_sigma = (kind == 0) ? sp.sigma.get() : nullptr;
  a.sponge_pre = (kind == 0) ? sp.pre.get() : nullptr;
  a.lam = h->lam_d.get();
  a.mu = h->mu_d.get();
  a.lam0 = h->lam0;
  a.mu0 = h->mu0;
  a.per_cell = h->per_cell;
  a.rho2 = op.density ? h->rho2_d.get() : nullptr;   // stage U1 only
  a.src_coef = op.src_coef;
  a.mode = op.mode;
  a.c_self = op.c_self;
  a.c_aux = op.c_aux;
  a.c_new = op.c_new;
  if (!h->src.fused) return SG_OK;
  const SourceNow sn = source_now(h, ctx);
  if (kind == 0 && op.in == SG_FIELD_S && op.mode == 0 && ctx.capture_src) {
    // stage UH1 of a captured step on the tile path: the launch that opens the step also names it
    a.src_step = sn.stepper;
    a.src_bump = 1;
  }
  if (op.with_source && sn.at.due) {   // tile path: the G kernel adds the source values
    a.src_slot = h->src.slot.get();
    a.src_idx = h->src.idx.get();
    a.src_vals = sn.values;
    a.src_scale = sn.at.scale;
    a.src_step = sn.stepper;
  }
  return SG_OK;
}

// The sponge pre-pass of an F stage (SpongeTables::pre): B_e u_abs of the sponge cells, queued before anything of the stage
// writes, when the buffer does not hold it yet (hostlogic.hpp PrePass).
static int sponge_pre_pass(sg_handle* h, const LaunchCtx& ctx, const StageOp& op, int region) {
  SpongeTables& sp = h->sponge;
  if (!sp.pre.get() || !sp.pre_state.due(op, region, h->field.versions())) return SG_OK;
  const void* uabs = h->field.read(op.uabs);
  // the cells with a sponge matrix
  if (launch_sponge_pre(uabs, sp.B.get(), sp.cells.get(), sp.mat.get(), sp.mat_slots.get(), sp.pre.get(), sp.nmat_slots, h->re.nd,
                        h->cfg.dim, h->ncls, (int)h->md.gw, sp.pre_lines, h->f32, ctx.stream) != 0)
    return fail(h, SG_ERR_DEVICE, "sponge pre-pass launch failed");
  // ... and the cells whose sigma is affine in the reference coordinates: dim + 1 numbers per cell, element-constant matrices
  const int arc = sp.aff_frag.get()
                      ? launch_sponge_affine_mfma(h->cfg.degree, uabs, sp.aff_frag.get(), sp.aff_items.get(), sp.aff_slots.get(),
                                                  sp.aff_coef.get(), sp.pre.get(), sp.aff_nitems, sp.aff_grid, ctx.stream)
                      : launch_sponge_pre_affine(uabs, sp.aff_X.get(), sp.aff_col.get(), sp.aff_W, sp.aff_items.get(),
                                                 sp.aff_slots.get(), sp.aff_coef.get(), sp.pre.get(), sp.aff_nitems, h->re.nd,
                                                 h->cfg.dim, (int)h->md.gw, sp.pre_lines, h->f32, sp.aff_grid, ctx.stream);
  if (arc != 0) return fail(h, SG_ERR_DEVICE, "affine-sigma sponge pre-pass launch failed");
  // SECOND runs on its own stream after ev_stage - "everything before this stage's FIRST" - and reads the pre-pass too
  if (region == SG_REGION_FIRST && h->overlap && h->first_recorded_stage >= 0) HIPCHECK(h, hipEventRecord(h->ev_stage, ctx.stream));
  return SG_OK;
}

// The (cell group, class) items with an active cube of a region of a split stage, listed once per region (both regions
// are static).  The interior launch then splits ACTIVE items evenly over the XCDs (a shell is whole z-layers of groups,
// i.e. the first items of XCD 0 and the last of XCD 7: skipping them inside an even split of all items would leave the
// launch as long as before); the shell launch deals its few items round-robin over all waves.
static int region_items(sg_handle* h, int region, const std::vector<Box>& boxes) {
  if (h->region_nitems[region] >= 0) return SG_OK;
  const RegionItems r = region_items(boxes, h->cfg.n, layout(h), h->md.ncube, h->md.ncube_pad);
  DevBuf<int32_t> list;
  if (!r.items.empty()) HIPCHECK(h, list.upload(r.items.data(), r.items.size()));
  h->region_items[region] = std::move(list);
  h->region_nitems[region] = (int32_t)r.items.size();
  h->region_whole[region] = r.whole;
  return SG_OK;
}

// The kernel instantiation that a stage launch with these arguments runs (kernels.hpp stage_kernel_*): the one place that
// picks - launches, captures and sg_stage_kernel_name all take it from here.
static int pick_kernel(sg_handle* h, int kind, const StageArgs& a, const void*& kernel) {
  const int P = h->cfg.degree;
  switch (h->family) {
    case Family::Generic: kernel = stage_kernel_generic(kind, h->cfg.dim, P, a); break;
    case Family::Lane: kernel = stage_kernel_lane(kind, h->cfg.dim, P, a); break;
    case Family::Mfma: kernel = stage_kernel_mfma(kind, P, a); break;
    case Family::Tile2d: kernel = stage_kernel_tile2d(kind, P, a); break;
    case Family::Hexm: kernel = stage_kernel_hexm(kind, P, a); break;
  }
  return kernel ? SG_OK : fail(h, SG_ERR_DEVICE, std::string("kernel launch failed: ") + hipGetErrorString((hipError_t)-1));
}

// Blocks of four waves the handle's device holds of a 2-D tile instantiation (launch_stage_tile2d's `resident`): asked of the
// runtime the first time the handle meets the kernel and kept with the handle.  A capture must not ask: capture_steps asks first.
static int tile_resident(sg_handle* h, const void* kernel) {
  for (const auto& kr : h->tile_resident)
    if (kr.first == kernel) return kr.second;
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 256, 0) != hipSuccess || per_cu <= 0) per_cu = 2;
  h->tile_resident.emplace_back(kernel, per_cu * h->ncu);
  return h->tile_resident.back().second;
}

// one launch of the family's stage kernel
static int launch_family(sg_handle* h, const LaunchCtx& ctx, int kind, const StageArgs& a) {
  const void* kernel = nullptr;
  if (int rc = pick_kernel(h, kind, a, kernel)) return rc;
  const int P = h->cfg.degree;
  const long ngroups = (long)(h->md.ncube_pad / h->md.gw);
  int rc = 0;
  switch (h->family) {
    case Family::Generic: rc = launch_stage(kernel, h->cfg.dim, P, a, ctx.stream); break;
    case Family::Lane: rc = launch_stage_lane(kernel, a, ngroups * h->ncls, ctx.stream); break;
    case Family::Mfma: rc = launch_stage_mfma(kernel, a, ctx.stream); break;
    case Family::Tile2d: rc = launch_stage_tile2d(kernel, tile_resident(h, kernel), a, h->t2c, ngroups * h->ncls, ctx.stream); break;
    case Family::Hexm: rc = launch_stage_hexm(kernel, P, a, ngroups, ctx.stream); break;
  }
  return rc != 0 ? fail(h, SG_ERR_DEVICE, std::string("kernel launch failed: ") + hipGetErrorString((hipError_t)rc)) : SG_OK;
}

// the boxes of a region that hold cubes
static std::vector<Box> region_cubes(const sg_handle* h, int region) {
  std::vector<Box> boxes;
  region_boxes(h, region, boxes);
  boxes.erase(std::remove_if(boxes.begin(), boxes.end(), [](const Box& b) { return b.n[0] <= 0 || b.n[1] <= 0 || b.n[2] <= 0; }), boxes.end());
  return boxes;
}

// the launches of a region: one per box for the generic kernels; the other families scan all cell groups and mask lanes
// by box in one launch
static int launch_region(sg_handle* h, const LaunchCtx& ctx, int kind, int region, StageArgs& a) {
  const std::vector<Box> boxes = region_cubes(h, region);
  if (!family_interleaved(h->family)) {
    for (const Box& b : boxes) {
      std::memcpy(a.box_o, b.o, sizeof(a.box_o));
      std::memcpy(a.box_n, b.n, sizeof(a.box_n));
      if (int rc = launch_family(h, ctx, kind, a)) return rc;
    }
    return SG_OK;
  }
  a.nbox = 0;
  for (const Box& b : boxes) {
    if (a.nbox >= SG_MAX_BOXES) return fail(h, SG_ERR_STATE, "region has more boxes than a launch can carry");
    for (int k = 0; k < 3; ++k) {
      a.boxes_o[a.nbox][k] = b.o[k];
      a.boxes_n[a.nbox][k] = b.n[k];
    }
    a.nbox += 1;
  }
  if (a.nbox == 0) return SG_OK;
  a.spread = (region == SG_REGION_BOUNDARY) ? 1 : 0;
  // only launches that run while an exchange is in flight leave block slots to RCCL
  a.grid_blocks = (region == SG_REGION_INTERIOR || region == SG_REGION_SECOND) ? h->grid_blocks : h->grid_full;
  // (the sponge is part of F only, and only cells with a matrix of their own make items differ in cost: then one item per
  // wave on the prime-strided grid)
  if (h->family == Family::Tile2d) a.grid_blocks = (h->sponge.nslots > 0 && kind == 0) ? h->tile_grid_sponge : h->tile_grid;
  a.item_list = nullptr;
  a.nlist = 0;
  a.order_chunk = (h->family == Family::Mfma && !a.spread && kind == 0) ? h->order_chunk : 0;
  if (region != SG_REGION_ALL) {
    if (int rc = region_items(h, region, boxes)) return rc;
    a.item_list = h->region_items[region].get();
    a.nlist = h->region_nitems[region];
    if (family_whole_groups(h->family) && h->region_whole[region] && !h->no_whole) a.all_active = 1;
  }
  a.nitems = a.item_list ? a.nlist : (int32_t)std::min<int64_t>((h->md.ncube_pad / h->md.gw) * h->ncls, INT32_MAX);
  return launch_family(h, ctx, kind, a);
}

// the source lives on single nodes: added to each part of a split stage right after the launch
// that wrote it (INTERIOR + BOUNDARY: all of it after the second launch)
static int add_source(sg_handle* h, const LaunchCtx& ctx, int field, double coef, int region) {
  if (h->src.fused) return SG_OK;  // added by the stage kernel (stage_args)
  const SourceNow sn = source_now(h, ctx);
  if (!sn.at.due || region == SG_REGION_INTERIOR) return SG_OK;
  const int d = h->cfg.dim;
  int64_t off = 0, cnt = h->src.nnz;
  if (region == SG_REGION_FIRST) cnt = h->src.nfirst;
  if (region == SG_REGION_SECOND) {
    off = h->src.nfirst;
    cnt = h->src.nnz - h->src.nfirst;
  }
  if (cnt == 0) return SG_OK;
  int rc = launch_source(h->field.write(field), d * d, h->md.gw, cnt, h->src.nodes.get() + off, sn.values + off * d * d, coef, sn.at.scale,
                         sn.stepper, h->f32, ctx.stream);
  return rc != 0 ? fail(h, SG_ERR_DEVICE, "source kernel launch failed") : SG_OK;
}

// Everything one stage launch queues, in this order: the sponge pre-pass, the region's kernels, and the source of a G
// stage that has one - inside those kernels (2-D tile family, stage_args) or by add_source: chosen here, for every caller.
static int run_op(sg_handle* h, const LaunchCtx& ctx, const StageOp& op, int region) {
  StageArgs a;
  if (int rc = stage_args(h, ctx, a, op, region)) return rc;
  if (int rc = sponge_pre_pass(h, ctx, op, region)) return rc;
  // the output counts as written from here on, i.e. after the pre-pass was decided (hostlogic.hpp PrePass::due)
  a.out = h->field.write(op.out);
  if (int rc = launch_region(h, ctx, op.kind, region, a)) return rc;
  return op.with_source ? add_source(h, ctx, op.out, op.src_coef, region) : SG_OK;
}

static StageOp stage_op(const sg_handle* h, int stage) {
  return lf4_stage(stage, h->dt, h->rho, h->rho_physical != 0, h->rho2_d.get() != nullptr);
}
static int run_stage_impl(sg_handle* h, const LaunchCtx& ctx, int stage, int region) { return run_op(h, ctx, stage_op(h, stage), region); }

// The kernel of an LF4 stage as a launch of `region` would choose it, without launching, allocating or counting anything;
// null (and SG_OK) for a region that has no box with cubes: it launches nothing.
static int stage_kernel(sg_handle* h, int stage, int region, const void*& kernel) {
  const StageOp op = stage_op(h, stage);
  StageArgs a;
  kernel = nullptr;
  if (int rc = stage_args(h, LaunchCtx{h->stream}, a, op, region)) return rc;
  return region_cubes(h, region).empty() ? SG_OK : pick_kernel(h, op.kind, a, kernel);
}

int resolve_timing(sg_handle* h) {
  if (h->ev_stage_ids.empty()) return SG_OK;
  if (int rc = join_second(h)) return rc;
  HIPCHECK(h, sync_all(h));
  for (size_t k = 0; k < h->ev_stage_ids.size(); ++k) {
    float ms = 0;
    HIPCHECK(h, hipEventElapsedTime(&ms, h->ev_pool[2 * k], h->ev_pool[2 * k + 1]));
    const int id = h->ev_stage_ids[k], st = id & 15;
    if (st == 6) {
      h->counters.halo_pack_ms += ms;
    } else if (id & 16) {
      // FIRST of a stage whose SECOND runs beside it on the other stream: both pairs start at (about) the same
      // point and overlap, so the stage's device time is the LONGER of the two, not their sum
      if (h->first_ms_pending[st] >= 0) h->counters.kernel_ms[st] += h->first_ms_pending[st];  // a FIRST without SECOND
      h->first_ms_pending[st] = ms;
    } else if (id & 32) {
      // (a SECOND whose FIRST was not timed - timing switched on between the two - counts with its own time)
      const double f = h->first_ms_pending[st];
      h->counters.kernel_ms[st] += (f >= 0 && f > ms) ? f : (double)ms;
      h->first_ms_pending[st] = -1;
    } else {
      h->counters.kernel_ms[st] += ms;
    }
  }
  h->ev_stage_ids.clear();
  return SG_OK;
}

// the wall clock of a stepping call (sg_last_step_ms): from ev0, which the caller recorded, to the end of what is queued
int finish_step_call(sg_handle* h) {
  HIPCHECK(h, hipEventRecord(h->ev1, h->stream));
  HIPCHECK(h, hipEventSynchronize(h->ev1));
  float ms = 0;
  HIPCHECK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
  h->last_ms = ms;
  return SG_OK;
}

// One launch of the injector kernel (kernels_inject.hip) on `stream`: entry step - 1 (by value, or *ctr) of `it`'s series.  The
// fields are taken for writing: whatever remembers a field state (the sponge pre-pass of the F stages, hostlogic.hpp PrePass)
// sees that the velocity has moved on - UTEMP's pre-pass of u1 is stale once an entry has been added to u1.
int queue_inject(sg_handle* h, hipStream_t stream, const InjectTables& it, const int64_t* ctr, int64_t step, int sym) {
  inject::Args a;
  std::memset(&a, 0, sizeof(a));
  a.ctr = ctr;
  a.step = step;
  a.nsteps = it.clock.count;
  a.item = it.item.get();
  a.lane = it.lane.get();
  a.start = it.start.get();
  a.psi = it.psi.get();
  a.amp = it.amp.get();
  a.ngroups = it.ngroups;
  a.nown = it.nown;
  a.ncomp = it.ncomp;
  a.nu = (it.what & 1) ? h->cfg.dim : 0;
  a.dim = h->cfg.dim;
  a.nd = h->re.nd;
  a.gw = (int32_t)h->md.gw;
  a.sym = sym >= 0 ? sym : (h->sym ? 1 : 0);
  void* u = (it.what & 1) ? (void*)h->field.write(SG_FIELD_U) : nullptr;
  void* s = (it.what & 2) ? (void*)h->field.write(SG_FIELD_S) : nullptr;
  if (launch_inject(u, s, a, h->f32, stream) != 0) return fail(h, SG_ERR_DEVICE, "injector launch failed");
  return SG_OK;
}

// Per-launch timing (sg_enable_timing): an event pair around a stage launch or a halo pack on stream s, resolved lazily by
// resolve_timing (8192 pending pairs at once, on the main stream); id as in sg_handle::ev_stage_ids.
static int timing_begin(sg_handle* h, hipStream_t s, size_t& k) {
  k = h->ev_stage_ids.size();
  if (!h->timing) return SG_OK;
  if (k >= 8192) {
    if (int rc = resolve_timing(h)) return rc;
    k = 0;
  }
  while (h->ev_pool.size() < 2 * k + 2) {
    hipEvent_t e;
    HIPCHECK(h, hipEventCreate(&e));
    h->ev_pool.push_back(e);
  }
  HIPCHECK(h, hipEventRecord(h->ev_pool[2 * k], s));
  return SG_OK;
}

static int timing_end(sg_handle* h, hipStream_t s, size_t k, int id) {
  if (!h->timing) return SG_OK;
  HIPCHECK(h, hipEventRecord(h->ev_pool[2 * k + 1], s));
  h->ev_stage_ids.push_back(id);
  return SG_OK;
}

extern "C" {

int sg_run_stage(sg_handle* h, int stage, int region) {
  if (!h) return SG_ERR_ARG;
  if (!h->params_set) return fail(h, SG_ERR_STATE, "sg_set_params must be called before stepping");
  if (region < 0 || region > 4) return fail(h, SG_ERR_ARG, "unknown region");
  if (stage < 0 || stage > 5) return fail(h, SG_ERR_ARG, "unknown stage");
  HIPCHECK(h, hipSetDevice(h->cfg.device));
  const bool second = h->overlap && region == SG_REGION_SECOND;
  if (second) {
    // depends on everything before this stage's FIRST (ev_stage), not on FIRST itself - so FIRST of the SAME stage
    // must have been issued (it records ev_stage); anything else would wait on a stale event and race
    if (h->first_recorded_stage != stage)
      return fail(h, SG_ERR_STATE, "sg_run_stage(stage, SG_REGION_SECOND) must follow sg_run_stage(stage, SG_REGION_FIRST) of the same stage");
    h->first_recorded_stage = -1;
    HIPCHECK(h, hipStreamWaitEvent(h->stream2, h->ev_stage, 0));
  } else {
    if (int rc = join_second(h)) return rc;
    if (h->overlap && region == SG_REGION_FIRST) {
      HIPCHECK(h, hipEventRecord(h->ev_stage, h->stream));
      h->first_recorded_stage = stage;
    }
  }
  const LaunchCtx ctx{second ? h->stream2 : h->stream};
  size_t k = 0;
  int rc = timing_begin(h, ctx.stream, k);
  if (rc != SG_OK) return rc;
  rc = run_stage_impl(h, ctx, stage, region);
  if (rc == SG_OK) rc = timing_end(h, ctx.stream, k, stage + ((h->overlap && region == SG_REGION_FIRST) ? 16 : (second ? 32 : 0)));
  if (second) {
    if (rc == SG_OK && hipEventRecord(h->ev_second, h->stream2) != hipSuccess) rc = fail(h, SG_ERR_DEVICE, "hipEventRecord failed");
    h->second_pending = rc == SG_OK;
  }
  if (rc != SG_OK) return rc;
  h->counters.launches[stage] += 1;
  return SG_OK;
}

// One launch of the recorder (kernels_recv.hip) on `stream`: u1 and s1 as they stand there at the owned receivers, into the
// trace's sample of the step (by value, or *ctr + 1) when that is a sample step.
static int queue_receivers(sg_handle* h, hipStream_t stream, const int64_t* ctr, int64_t step) {
  const ReceiverTables& rt = h->rec;
  RecvArgs a;
  std::memset(&a, 0, sizeof(a));
  a.ctr = ctr;
  a.step = step;
  a.every = rt.clock.every;
  a.capacity = rt.clock.count;
  a.item = rt.item.get();
  a.lane = rt.lane.get();
  a.phi = rt.phi.get();
  a.trace = rt.trace.get();
  a.nown = rt.nown;
  a.ncomp = rt.ncomp;
  a.nu = (rt.what & 1) ? h->cfg.dim : 0;
  a.dim = h->cfg.dim;
  a.nd = h->re.nd;
  a.gw = (int32_t)h->md.gw;
  a.sym = h->sym ? 1 : 0;
  if (launch_receivers(h->field.read(SG_FIELD_U), h->field.read(SG_FIELD_S), a, h->f32, stream) != 0)
    return fail(h, SG_ERR_DEVICE, "receiver launch failed");
  return SG_OK;
}

// The two passes of a monitor sample (kernels_measure.hip) on `stream`: of the fields as they stand there, with these weights,
// into out[step / every - 1] when the step (by value, or *ctr + 1) is a sample step.
static int queue_measure(sg_handle* h, hipStream_t stream, const double* w_cells, const double w0[3], const int64_t* ctr, int64_t step,
                         int64_t every, int64_t capacity, double* out) {
  const MeasureScratch& ms = h->msr;
  measure::Args a;
  std::memset(&a, 0, sizeof(a));
  a.ctr = ctr;
  a.step = step;
  a.every = every;
  a.capacity = capacity;
  a.Mtri = ms.Mtri.get();
  a.w = w_cells;
  for (int k = 0; k < 3; ++k) a.w0[k] = w0[k];
  a.detj = 1.0;
  for (int k = 0; k < h->cfg.dim; ++k) a.detj *= h->cfg.h[k];
  a.partial = ms.partial.get();
  a.out = out;
  a.nitems = ms.nitems;
  a.ncube = h->md.ncube;
  a.nchunks = ms.nchunks;
  a.nd = h->re.nd;
  a.dim = h->cfg.dim;
  a.gw = (int32_t)h->md.gw;
  a.ncls = h->ncls;
  a.ips = ms.ips;
  const std::vector<MonitorComp> comps = monitor_components(h->cfg.dim, h->sym);
  a.ncomp = (int32_t)comps.size();
  for (size_t k = 0; k < comps.size(); ++k) {
    a.comp[k] = comps[k].comp;
    a.diag[k] = comps[k].diag ? 1 : 0;
    a.mult[k] = comps[k].mult;
  }
  if (launch_measure(h->field.read(SG_FIELD_U), h->field.read(SG_FIELD_S), a, h->f32, stream) != 0)
    return fail(h, SG_ERR_DEVICE, "monitor launch failed");
  return SG_OK;
}

// ... of the armed monitor (sg_set_monitor), into its trace
static int queue_monitor(sg_handle* h, hipStream_t stream, const int64_t* ctr, int64_t step) {
  const MonitorTables& mt = h->mon;
  return queue_measure(h, stream, mt.w.get(), mt.w0, ctr, step, mt.clock.every, mt.clock.count, mt.trace.get());
}
// the armed injectors' launch (sg_set_injectors): entry step - 1 of their series, which belongs to the step that follows
static int queue_injectors(sg_handle* h, hipStream_t stream, const int64_t* ctr, int64_t step) {
  return queue_inject(h, stream, h->inj, ctr, step);
}

// One launch of the spectra kernel per selected field (kernels_spectra.hip) on `stream`: the fields as they stand there enter
// the accumulators when the step (by value, or *ctr + 1) is a sample step of the series.
static int queue_spectra(sg_handle* h, hipStream_t stream, const int64_t* ctr, int64_t step) {
  const SpectraTables& sp = h->spc;
  const int fields[2] = {SG_FIELD_U, SG_FIELD_S};
  for (int k = 0; k < 2; ++k) {
    if (!sp.has(k)) continue;
    spectra::Args a;
    std::memset(&a, 0, sizeof(a));
    a.ctr = ctr;
    a.step = step;
    a.every = sp.clock.every;
    a.nsamples = sp.clock.count;
    a.w = sp.w[k].get();
    a.acc = sp.acc[k].get();
    a.n = (int64_t)h->field_alloc[fields[k]];
    a.nfreq = sp.nfreq;
    a.gw = (int32_t)h->md.gw;
    a.dim = h->cfg.dim;
    a.ncomp = k == 1 ? h->cfg.dim * h->cfg.dim : h->cfg.dim;
    a.sym = (k == 1 && h->sym) ? 1 : 0;
    a.vec_line = a.gw % (h->f32 ? 4 : 2) == 0 ? 1 : 0;
    if (launch_spectra(h->field.read(fields[k]), a, h->f32, 8 * std::max(h->ncu, 1), stream) != 0)
      return fail(h, SG_ERR_DEVICE, "spectra launch failed");
  }
  return SG_OK;
}

// What runs at the end of every step, on the main stream behind stage S1's SECOND launch, as values: the hooks in the order
// they run.  The receivers' recorder, the gauges (gauge.cpp) and the monitor sample u1 and s1 of the step that just ended, and so
// do the spectra and the peak maps (peak.cpp) - before the injectors add the entry that belongs to the step that follows.  All six keep one protocol
// (hook_step, and the callers that walk this table); they differ in what stands here.
struct Hook {
  StepSeries* series;   // the clock and the device-side step counter
  bool armed;           // a disarmed hook does nothing and counts nothing
  bool has_launches;    // on this block (the points of the receivers and the injectors have one owner); steps count on every block
  // a full series - true: refuses the step (end_of_step, check_room), and the hook launches at every step: its kernel tells
  // the sample steps; false: has run out silently, and the hook launches at the due steps only
  bool refuses;
  const char* name;     // ... and what a refusal calls the trace and
  const char* getter;   // ... the call that reads it out
  int (*queue)(sg_handle* h, hipStream_t stream, const int64_t* ctr, int64_t step);   // the step by value, or *ctr + 1
  uint32_t bit;         // in sg_handle::in_graphs
};
using Hooks = std::array<Hook, 6>;
static Hooks hooks(sg_handle* h) {
  return {{{&h->rec, h->rec.nrec > 0, h->rec.nown > 0, true, "receiver", "sg_get_receivers", queue_receivers, 2u << 0},
           {&h->gge, h->gge.npts > 0, h->gge.nown > 0, true, "gauge", "sg_get_gauges", h->gge.queue, 2u << 5},
           {&h->mon, h->mon.armed, true, true, "monitor", "sg_get_monitor", queue_monitor, 2u << 1},
           {&h->spc, h->spc.nfreq > 0, true, false, "", "", queue_spectra, 2u << 2},
           {&h->pk, h->pk.what != 0, true, false, "", "", h->pk.queue, 2u << 4},
           {&h->inj, h->inj.npts > 0, h->inj.nown > 0, false, "", "", queue_injectors, 2u << 3}}};
}

// The end of a step for one hook.  Eager launches name the step by value and count it here; the launches of a capture read
// it from the hook's counter and bump that, and a capture counts nothing (sg_step sets the counter before it replays and
// counts the replayed steps) - so active() holds for all of a capture's steps: the graphs have a run-out hook's launches, the
// kernel's threads exiting at once beyond the series, or have none (ensure_graphs).
static int hook_step(sg_handle* h, const LaunchCtx& ctx, const Hook& k) {
  if (!k.armed) return SG_OK;
  StepClock& c = k.series->clock;
  const int64_t step = c.steps + 1;
  const bool launch = k.refuses || (ctx.capture ? c.active() : c.due_at(step));
  if (k.has_launches && launch) {
    if (int rc = join_second(h)) return rc;
    if (int rc = k.queue(h, ctx.stream, ctx.capture ? k.series->ctr.get() : nullptr, step)) return rc;
    if (ctx.capture && launch_step_counter(k.series->ctr.get(), 1, 1, ctx.stream) != 0)
      return fail(h, SG_ERR_DEVICE, "step counter launch failed");
  }
  if (!ctx.capture) c.steps = step;
  return SG_OK;
}

// What ends a step on the stream: the hooks in their order.  A refusal (no room for the step's sample) is found before
// anything is queued or counted - where two traces are full the later hook's, the monitor's, is reported; a launch error of
// a later hook leaves the earlier ones' step counted.  A capture refuses nothing: sg_step has checked its steps (check_room).
static int end_of_step(sg_handle* h, const LaunchCtx& ctx) {
  const Hooks hs = hooks(h);
  for (auto it = hs.rbegin(); it != hs.rend() && !ctx.capture; ++it) {
    const Hook& k = *it;
    if (k.armed && k.refuses && k.series->clock.no_room_at(k.series->clock.steps + 1))
      return fail(h, SG_ERR_STATE, std::string(k.name) + " trace full: read it out (" + k.getter + ") and re-arm before stepping on");
  }
  for (const Hook& k : hs)
    if (int rc = hook_step(h, ctx, k)) return rc;
  return SG_OK;
}

// The bookkeeping of n finished steps.  Eager stage launches and hook_step have counted themselves; replayed steps
// count here, and what a replay wrote is new to everything that remembers a field state.
static void steps_done(sg_handle* h, int64_t n, bool replayed) {
  h->src_step += n;
  h->counters.steps += n;
  if (!replayed) return;
  for (int st = 0; st < 6; ++st) h->counters.launches[st] += n;
  for (const Hook& k : hooks(h))
    if (k.armed) k.series->clock.steps += n;
  h->field.replayed();
  h->sponge.pre_state.forget();
}

int sg_end_step(sg_handle* h) {
  if (!h) return SG_ERR_ARG;
  HIPCHECK(h, hipSetDevice(h->cfg.device));
  if (int rc = end_of_step(h, LaunchCtx{h->stream})) return rc;
  steps_done(h, 1, false);
  return SG_OK;
}

// one LF4 step = six whole-block launches on the handle's stream (elastic.py:291-304).  counted: the eager steps of
// sg_step, which count their launches, through sg_run_stage (an event pair per launch) when timing is on.
static int run_stages(sg_handle* h, const LaunchCtx& ctx, bool counted) {
  for (int st = 0; st < 6; ++st) {
    const bool timed = counted && h->timing;
    if (int rc = timed ? sg_run_stage(h, st, SG_REGION_ALL) : run_stage_impl(h, ctx, st, SG_REGION_ALL)) return rc;
    if (counted && !timed) h->counters.launches[st] += 1;
  }
  return SG_OK;
}

// ... and what ends it on the stream; counted = false: a step of a capture
static int enqueue_step(sg_handle* h, const LaunchCtx& ctx, bool counted) {
  if (int rc = run_stages(h, ctx, counted)) return rc;
  // the next step's slice (tile path: stage UH1 bumps the counter itself, stage_args)
  if (ctx.capture_src && !h->src.fused && launch_step_counter(h->src_ctr_d.get(), 1, 1, ctx.stream) != 0)
    return fail(h, SG_ERR_DEVICE, "step counter launch failed");
  return end_of_step(h, ctx);
}

// capture `steps` steps into an executable graph; on any failure graphs are switched off for the handle
static hipGraphExec_t capture_steps(sg_handle* h, int steps, bool with_src) {
  hipGraph_t g = nullptr;
  hipGraphExec_t ge = nullptr;
  // what a launch asks the runtime once per kernel instantiation - the resident blocks of the 2-D tile kernels - is
  // asked here, outside the capture, of the six stages' kernels (a failure shows again, and is reported, in the capture)
  for (int st = 0; st < 6 && h->family == Family::Tile2d; ++st) {
    const void* kernel = nullptr;
    if (stage_kernel(h, st, SG_REGION_ALL, kernel) == SG_OK && kernel) (void)tile_resident(h, kernel);
  }
  if (hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) return nullptr;
  int rc = SG_OK;
  const LaunchCtx ctx{h->stream, with_src, true};
  h->sponge.pre_state.forget();      // a replay starts from whatever the buffer holds: the captured step computes its own
  for (int k = 0; k < steps && rc == SG_OK; ++k) rc = enqueue_step(h, ctx, false);
  h->sponge.pre_state.forget();      // nothing was launched: the buffer does not hold what the capture asked for
  hipError_t e = hipStreamEndCapture(h->stream, &g);
  if (rc == SG_OK && e == hipSuccess && g) {
    if (hipGraphInstantiate(&ge, g, nullptr, nullptr, 0) != hipSuccess) ge = nullptr;
  }
  if (g) (void)hipGraphDestroy(g);
  (void)hipGetLastError();
  return ge;
}

// The samples of all nsteps steps must fit the trace of every hook that refuses: checked before anything is queued (native
// exchange too).
static int check_room(sg_handle* h, int64_t nsteps) {
  for (const Hook& k : hooks(h)) {
    const StepClock& c = k.series->clock;
    if (!k.armed || !k.refuses || c.fits(nsteps)) continue;
    return fail(h, SG_ERR_STATE, std::string("sg_step: the ") + k.name + " trace has room for " + std::to_string(c.count - c.samples()) +
                                     " more samples, these steps take " + std::to_string(c.samples_after(nsteps) - c.samples()));
  }
  return SG_OK;
}

// The graphs of one and of eight steps, captured again when a setter changed kernel arguments (epoch) or the source or a hook
// came or went.  A source that is still active is part of them: its launches take the step's slice and weight from a
// device-side counter (kernels.hpp SrcStep); one that has run out, or none: no source launches.  An armed hook likewise,
// while its series has a step to come (a hook that refuses always has: a full trace stops the stepping).
static int ensure_graphs(sg_handle* h) {
  const bool with_src = source_at(h, false).active;
  if (with_src && !h->src_ctr_d.get()) return fail(h, SG_ERR_STATE, "source without a device-side step counter");
  uint32_t with = with_src ? 1u : 0u;
  for (const Hook& k : hooks(h))
    if (k.armed && (k.refuses || k.series->clock.active())) with |= k.bit;
  if (h->graph_epoch == h->epoch && h->in_graphs == with) return SG_OK;
  if (h->graph1) (void)hipGraphExecDestroy(h->graph1);
  if (h->graph8) (void)hipGraphExecDestroy(h->graph8);
  h->graph1 = capture_steps(h, 1, with_src);
  h->graph8 = h->graph1 ? capture_steps(h, 8, with_src) : nullptr;
  h->graph_epoch = h->epoch;
  h->in_graphs = with;
  if (!h->graph1 || !h->graph8) h->graph_ok = false;  // same kernels, launched one by one (eager_steps)
  return SG_OK;
}

// nsteps steps as graph replays; the device-side counters start from the step the replay starts from
static int replay_steps(sg_handle* h, int64_t nsteps) {
  // (tile path: the counter is bumped by the launch that OPENS a step, so it starts one short)
  if ((h->in_graphs & 1u) && launch_step_counter(h->src_ctr_d.get(), h->src_step - (h->src.fused ? 1 : 0), 0, h->stream) != 0)
    return fail(h, SG_ERR_DEVICE, "step counter launch failed");
  // a hook that is in the graphs and has launches there (each a word of its own: the order of these launches is the table's)
  for (const Hook& k : hooks(h))
    if ((h->in_graphs & k.bit) && k.has_launches && launch_step_counter(k.series->ctr.get(), k.series->clock.steps, 0, h->stream) != 0)
      return fail(h, SG_ERR_DEVICE, "step counter launch failed");
  int64_t k = 0;
  for (; k + 8 <= nsteps; k += 8) HIPCHECK(h, hipGraphLaunch(h->graph8, h->stream));
  for (; k < nsteps; ++k) HIPCHECK(h, hipGraphLaunch(h->graph1, h->stream));
  steps_done(h, nsteps, true);
  return SG_OK;
}

static int eager_steps(sg_handle* h, int64_t nsteps) {
  for (int64_t k = 0; k < nsteps; ++k) {
    if (int rc = enqueue_step(h, LaunchCtx{h->stream}, true)) return rc;
    steps_done(h, 1, false);
  }
  return SG_OK;
}

int sg_step(sg_handle* h, int64_t nsteps) {
  if (!h || nsteps < 0) return SG_ERR_ARG;
  if (!h->params_set) return fail(h, SG_ERR_STATE, "sg_set_params must be called before stepping");
  if (int rc = check_room(h, nsteps)) return rc;
  HIPCHECK(h, hipSetDevice(h->cfg.device));
  for (int s = 0; s < 6; ++s)
    if (h->md.has_nbr[s]) {
      if (h->comm) return comm_step(h, nsteps);     // the native exchange (comm.cpp)
      return fail(h, SG_ERR_STATE, "sg_step on a block with neighbours: attach a communicator (sg_comm_init) or drive "
                                   "stages + halo from the host");
    }
  // launch-bound blocks: replay captured graphs (no per-stage timing)
  const bool graphs = h->graph_ok && !h->timing && nsteps >= 2;
  if (graphs)
    if (int rc = ensure_graphs(h)) return rc;
  HIPCHECK(h, hipEventRecord(h->ev0, h->stream));
  if (int rc = (graphs && h->graph_ok) ? replay_steps(h, nsteps) : eager_steps(h, nsteps)) return rc;
  return finish_step_call(h);
}

// One sample of the fields as they stand behind everything the handle has queued, with the caller's weights.
int sg_measure(sg_handle* h, const double* w, int per_cell, double out[5]) {
  if (!h || !out) return SG_ERR_ARG;
  if (per_cell && !w) return fail(h, SG_ERR_ARG, "sg_measure: per-cell weights without weights");
  HIPCHECK(h, hipSetDevice(h->cfg.device));
  if (int rc = measure_prepare(h)) return rc;
  DevBuf<double> w_cells;
  double w0[3] = {0.0, 0.0, 0.0};
  if (w && per_cell) HIPCHECK(h, w_cells.upload(w, (size_t)h->ncells * 3));
  if (w && !per_cell) std::memcpy(w0, w, sizeof(w0));
  if (int rc = join_second(h)) return rc;
  if (int rc = queue_measure(h, h->stream, w && per_cell ? w_cells.get() : nullptr, w0, nullptr, 1, 1, 1, h->msr.out.get())) return rc;
  HIPCHECK(h, hipStreamSynchronize(h->stream));
  HIPCHECK(h, hipMemcpy(out, h->msr.out.get(), 5 * sizeof(double), hipMemcpyDeviceToHost));
  return SG_OK;
}

int sg_last_step_ms(sg_handle* h, double* ms) {
  if (!h || !ms) return SG_ERR_ARG;
  *ms = h->last_ms;
  return SG_OK;
}

int sg_apply_F(sg_handle* h, int s_in, int u_abs, int u_out) {
  if (!h) return SG_ERR_ARG;
  if (!field_is_stress(s_in) || field_is_stress(u_out) || field_is_stress(u_abs) || u_abs == u_out)
    return fail(h, SG_ERR_ARG, "sg_apply_F: s_in must be a stress field, u_abs/u_out distinct velocity fields");
  HIPCHECK(h, hipSetDevice(h->cfg.device));
  return run_op(h, LaunchCtx{h->stream}, StageOp{0, s_in, u_out, -1, u_abs}, SG_REGION_ALL);
}

int sg_apply_G(sg_handle* h, int u_in, int s_out, int use_source) {
  if (!h) return SG_ERR_ARG;
  if (field_is_stress(u_in) || !field_is_stress(s_out))
    return fail(h, SG_ERR_ARG, "sg_apply_G: u_in must be a velocity field, s_out a stress field");
  if (!h->params_set) return fail(h, SG_ERR_STATE, "sg_set_params must be called first");
  HIPCHECK(h, hipSetDevice(h->cfg.device));
  StageOp op{1, u_in, s_out};
  op.with_source = use_source != 0;
  return run_op(h, LaunchCtx{h->stream}, op, SG_REGION_ALL);
}

// ---- halo ---------------------------------------------------------------------------------

int sg_halo_bytes(const sg_handle* h, int field, int side, size_t* nbytes) {
  if (!h || !nbytes || field < 0 || field > 3 || side < 0 || side >= 2 * h->cfg.dim) return SG_ERR_ARG;
  const int d = h->cfg.dim;
  int axis = side >> 1;
  size_t n2 = 1;
  for (int a = 0; a < 3; ++a)
    if (a != axis) n2 *= (size_t)h->cfg.n[a];
  // dim components per facet node for every field: a stress trace travels as T_i,axis (kernels.hip pack_one)
  *nbytes = n2 * h->md.halo_per_cube * h->re.nf * (size_t)d * (h->f32 ? sizeof(float) : sizeof(double));
  (void)field;
  return SG_OK;
}

int sg_halo_pack(sg_handle* h, int field, int side, void* dev_out) {
  if (!h || !dev_out || field < 0 || field > 3 || side < 0 || side >= 2 * h->cfg.dim) return SG_ERR_ARG;
  void* outs[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  outs[side] = dev_out;
  return sg_halo_pack_sides(h, field, outs);
}

int sg_halo_pack_sides(sg_handle* h, int field, void* const* dev_out) {
  if (!h || !dev_out || field < 0 || field > 3) return SG_ERR_ARG;
  HIPCHECK(h, hipSetDevice(h->cfg.device));
  const int d = h->cfg.dim;
  int comps = field_is_stress(field) ? d * d : d;
  int sides[6], n = 0;
  void* outs[6];
  for (int s = 0; s < 2 * d; ++s)
    if (dev_out[s]) {
      sides[n] = s;
      outs[n] = dev_out[s];
      n += 1;
    }
  if (int rc = join_second(h)) return rc;
  size_t k = 0, total = 0;
  int rc = timing_begin(h, h->stream, k);     // pack launches are timed like stage launches (stage id 6)
  if (rc != SG_OK) return rc;
  rc = launch_pack(h->md_dev.get(), h->md, h->field.read(field), comps, n, sides, outs,
                   (h->sym && field_is_stress(field)) ? 1 : 0, h->f32, h->stream);
  if (rc != 0) return fail(h, SG_ERR_DEVICE, "pack kernel launch failed");
  for (int i = 0; i < n; ++i) {
    size_t nb = 0;
    (void)sg_halo_bytes(h, field, sides[i], &nb);
    total += nb;
  }
  if (int rc = timing_end(h, h->stream, k, 6)) return rc;
  h->counters.halo_pack_launches += 1;
  h->counters.halo_bytes_packed += (int64_t)total;
  return SG_OK;
}

// ---- instrumentation ----------------------------------------------------------------------------

int sg_enable_timing(sg_handle* h, int on) {
  if (!h) return SG_ERR_ARG;
  if (!on) {
    int rc = resolve_timing(h);
    if (rc != SG_OK) return rc;
  }
  h->timing = on != 0;
  return SG_OK;
}

int sg_get_counters(sg_handle* h, sg_counters_t* out) {
  if (!h || !out) return SG_ERR_ARG;
  HIPCHECK(h, hipSetDevice(h->cfg.device));
  int rc = resolve_timing(h);
  if (rc != SG_OK) return rc;
  for (int st = 0; st < 6; ++st)      // a FIRST launch whose SECOND was never issued
    if (h->first_ms_pending[st] >= 0 && !h->second_pending) {
      h->counters.kernel_ms[st] += h->first_ms_pending[st];
      h->first_ms_pending[st] = -1;
    }
  *out = h->counters;
  return SG_OK;
}

int sg_stage_kernel_name(sg_handle* h, int stage, int region, char* buf, size_t n) {
  if (!h || !buf || n == 0) return SG_ERR_ARG;
  if (region < 0 || region > 4) return fail(h, SG_ERR_ARG, "unknown region");
  if (stage < 0 || stage > 5) return fail(h, SG_ERR_ARG, "unknown stage");
  HIPCHECK(h, hipSetDevice(h->cfg.device));
  // the choice that a launch makes (pick_kernel), named from the handle that a launch would pass to the runtime
  const void* kernel = nullptr;
  if (int rc = stage_kernel(h, stage, region, kernel)) return rc;
  std::snprintf(buf, n, "%s", kernel ? kernel_name_of(kernel).c_str() : "");
  return SG_OK;
}

}  // extern "C"
