// C-ABI of libseigen_hip.so (see include/seigen_hip.h): handle life cycle (device memory, operator tables, kernel
// family choice), parameters, sponge, source and the table exports.  Field transfers: transfer.cpp; stage launches,
// the fused six-launch LF4 step (seigen/elastic.py:283-313) and halo packs: stages.cpp.
#include <limits>
#include <stdexcept>
#include <string>

#include "handle.hpp"
#include "source_tables.hpp"
#include "sponge_tables.hpp"

// the configuration, the reference element and the mesh tables
static int init_element(const sg_config* cfg, sg_handle* h) {
  if (cfg->dim < 1 || cfg->dim > 3) return fail(h, SG_ERR_ARG, "dim must be 1, 2 or 3");
  if (cfg->degree < 1 || cfg->degree > 4) return fail(h, SG_ERR_ARG, "degree must be 1..4");
  for (int a = 0; a < cfg->dim; ++a) {
    if (cfg->n[a] < 1) return fail(h, SG_ERR_ARG, "n[axis] must be >= 1");
    if (!(cfg->h[a] > 0.0)) return fail(h, SG_ERR_ARG, "h[axis] must be > 0");
  }
  h->cfg = *cfg;
  for (int a = cfg->dim; a < 3; ++a) {
    h->cfg.n[a] = 1;
    h->cfg.h[a] = 1.0;
    h->cfg.origin[a] = 0.0;
    h->cfg.cube0[a] = 0;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(h, SG_ERR_DEVICE, "no HIP device available (libseigen_hip has no CPU fallback)");
  if (cfg->device < 0 || cfg->device >= ndev) return fail(h, SG_ERR_ARG, "device ordinal out of range");
  HIPCHECK(h, hipSetDevice(cfg->device));

  if (cfg->diagonal == SG_DIAGONAL_QUAD && cfg->dim == 1) return fail(h, SG_ERR_ARG, "tensor-product cells need dim 2 or 3");
  try {
    h->re = make_refelem(cfg->dim, cfg->degree, cfg->diagonal == SG_DIAGONAL_QUAD ? KIND_TENSOR : KIND_SIMPLEX);
    std::memset(&h->md, 0, sizeof(MeshDev));
    h->md.nd = h->re.nd;
    h->md.nf = h->re.nf;
    build_mesh_tables(cfg->dim, cfg->degree, cfg->diagonal, h->cfg.h, h->re.fnode.data(), h->re.lattice.data(), h->md);
  } catch (const std::exception& e) {
    return fail(h, SG_ERR_ARG, e.what());
  }
  for (int a = 0; a < 3; ++a) h->md.n[a] = h->cfg.n[a];
  for (int s = 0; s < 6; ++s) h->md.has_nbr[s] = (s < 2 * cfg->dim) ? ((cfg->nbr_mask >> s) & 1) : 0;
  h->ncls = h->md.ncls;
  h->ncells = (int64_t)h->cfg.n[0] * h->cfg.n[1] * h->cfg.n[2] * h->ncls;
  return SG_OK;
}

// the kernel family, and with it the precision and the layout
static int init_family(sg_handle* h) {
  h->family = choose_kernel_path(h->cfg);
  if (h->cfg.dtype != 0 && h->cfg.dtype != 1) return fail(h, SG_ERR_ARG, "dtype must be 0 (f64) or 1 (f32)");
  h->f32 = h->cfg.dtype;
  if (h->f32 && !family_f32(h->family))
    return fail(h, SG_ERR_ARG, "dtype f32 is implemented on the MFMA paths (3-D blocks: degree 1 from 65536 cells; 2-D "
                               "blocks on the tile kernels)");
  h->md.gw = family_gw(h->family);
  h->md.ncube = (int64_t)h->cfg.n[0] * h->cfg.n[1] * h->cfg.n[2];
  h->md.ncube_pad = (h->md.ncube + h->md.gw - 1) / h->md.gw * h->md.gw;
  return SG_OK;
}

// hexahedra, every family (kernels_lane.hip hex_stage, kernels_hexm.hip, kernels.hip stage_kernel TP = 2): the 1-D
// factors D1 [n1][n1] and lift1 [2][n1], read off the full tables along the first axis and checked against ALL of D_r, L_f
static int hex_factors(sg_handle* h, std::vector<double>& Dt) {
  const RefElem& re = h->re;
  const int nd = re.nd, nf = re.nf, n1 = h->cfg.degree + 1;
  auto node = [&](int a0, int a1, int a2) { return a0 + n1 * (a1 + n1 * a2); };
  Dt.assign((size_t)n1 * n1 + 2 * n1, 0.0);
  for (int m = 0; m < n1; ++m) {
    for (int n = 0; n < n1; ++n) Dt[(size_t)m * n1 + n] = re.D[((size_t)0 * nd + node(m, 0, 0)) * nd + node(n, 0, 0)];
    for (int s = 0; s < 2; ++s) Dt[(size_t)n1 * n1 + s * n1 + m] = re.L[((size_t)s * nd + node(m, 0, 0)) * nf + 0];
  }
  double worst = 0.0;
  for (int a = 0; a < nd; ++a) {
    const int ai[3] = {a % n1, (a / n1) % n1, a / (n1 * n1)};
    for (int r = 0; r < 3; ++r) {
      for (int b = 0; b < nd; ++b) {
        const int bi[3] = {b % n1, (b / n1) % n1, b / (n1 * n1)};
        const bool line = ai[(r + 1) % 3] == bi[(r + 1) % 3] && ai[(r + 2) % 3] == bi[(r + 2) % 3];
        const double want = line ? Dt[(size_t)ai[r] * n1 + bi[r]] : 0.0;
        worst = std::max(worst, std::fabs(re.D[((size_t)r * nd + a) * nd + b] - want));
      }
      for (int s = 0; s < 2; ++s)
        for (int bp = 0; bp < nf; ++bp) {
          const int b = re.fnode[(size_t)(2 * r + s) * nf + bp];
          const int bi[3] = {b % n1, (b / n1) % n1, b / (n1 * n1)};
          // facet nodes in ascending order: bp = lower transverse index + n1 * the upper one
          const int lo = r == 0 ? 1 : 0, hi = r == 2 ? 1 : 2;
          // ... and the neighbour's matching node is the one across the cube, at the same place of its facet list
          int ni[3] = {bi[0], bi[1], bi[2]};
          ni[r] = s ? 0 : n1 - 1;
          if (bp != bi[lo] + n1 * bi[hi] || bi[r] != (s ? n1 - 1 : 0) || h->md.fnode[2 * r + s][bp] != b ||
              h->md.nb_node[0][2 * r + s][bp] != node(ni[0], ni[1], ni[2]) || h->md.nb_fnode[0][2 * r + s][bp] != bp ||
              h->md.nb_face[0][2 * r + s] != 2 * r + (1 - s) || h->md.nb_axis[0][2 * r + s] != r)
            return fail(h, SG_ERR_ARG, "hexahedral element: unexpected facet node order");
          const bool same = ai[lo] == bi[lo] && ai[hi] == bi[hi];
          const double want = same ? Dt[(size_t)n1 * n1 + s * n1 + ai[r]] : 0.0;
          worst = std::max(worst, std::fabs(re.L[((size_t)(2 * r + s) * nd + a) * nf + bp] - want));
        }
    }
  }
  if (worst > 1e-11) return fail(h, SG_ERR_ARG, "hexahedral element: the operator tables do not factorise");
  return SG_OK;
}

// The operator fragments of the matrix-pipe families, F, G, L (and Q, P: the factorised G volume), as the device holds
// them: float tables two values to a double where f32 (StageArgs::fragV / fragL are double pointers, as the fields are)
using Frags = std::vector<double>[5];
template <typename T>
static void set_frags(Frags& fr, const std::vector<T>& fF, const std::vector<T>& fG, const std::vector<T>& fL) {
  for (auto [i, v] : {std::make_pair(0, &fF), std::make_pair(1, &fG), std::make_pair(2, &fL)}) {
    fr[i].assign((v->size() * sizeof(T) + sizeof(double) - 1) / sizeof(double), 0.0);
    std::memcpy(fr[i].data(), v->data(), v->size() * sizeof(T));
  }
}

// The tables of the family: StageArgs::Dt / Lt and the mesh tables on the device, the MFMA constants on the device, the
// fragments in `fr` (uploaded after the fields, init_fields: the device allocations keep their order)
static int family_tables(sg_handle* h, Frags& fr) {
  const sg_config* cfg = &h->cfg;
  const RefElem& re = h->re;
  const int d = cfg->dim, nd = re.nd, nf = re.nf, nfaces = re.nfaces;
  // transposed operators: Dt[r][b][a], Lt[f][b'][a]
  std::vector<double> Dt((size_t)d * nd * nd), Lt((size_t)nfaces * nf * nd);
  for (int r = 0; r < d; ++r)
    for (int a = 0; a < nd; ++a)
      for (int b = 0; b < nd; ++b) Dt[((size_t)r * nd + b) * nd + a] = re.D[((size_t)r * nd + a) * nd + b];
  for (int f = 0; f < nfaces; ++f)
    for (int a = 0; a < nd; ++a)
      for (int b = 0; b < nf; ++b) Lt[((size_t)f * nf + b) * nd + a] = re.L[((size_t)f * nd + a) * nf + b];
  const bool hex = re.kind == KIND_TENSOR && d == 3;
  if (int rc = hex ? hex_factors(h, Dt) : SG_OK) return rc;
  switch (h->family) {
    case Family::Generic: break;
    case Family::Hexm: {   // kernels_hexm.hip: line operators with the own-trace half folded in, x-pass A operands
      Dt = hexm_table(cfg->degree, Dt.data(), Dt.data() + (size_t)(cfg->degree + 1) * (cfg->degree + 1), h->md);
      break;
    }
    case Family::Lane: {
      if (hex) break;
      // E_r = D_r - (L_0 R_0 - L_{r+1} R_{r+1}) / (2 (d-1)!) row-major (own-trace half of the central flux folded into the
      // volume operator, see mfma_tables.cpp), and L_f row-major
      double fact = 1.0;
      for (int i = 2; i <= d - 1; ++i) fact *= i;
      const double cfold = 1.0 / (2.0 * fact);
      for (int r = 0; r < d; ++r)
        for (int a = 0; a < nd; ++a)
          for (int b = 0; b < nd; ++b) {
            double v = re.D[((size_t)r * nd + a) * nd + b];
            for (int bf = 0; bf < nf; ++bf) {
              if (re.fnode[(size_t)0 * nf + bf] == b) v -= cfold * re.L[((size_t)0 * nd + a) * nf + bf];
              if (re.fnode[(size_t)(r + 1) * nf + bf] == b) v += cfold * re.L[((size_t)(r + 1) * nd + a) * nf + bf];
            }
            Dt[((size_t)r * nd + a) * nd + b] = v;
          }
      Lt = re.L;
      break;
    }
    case Family::Mfma: {
      if (h->f32) set_frags(fr, mfma32_frags_F(re), mfma32_frags_G(re), mfma32_frags_L(re));
      else set_frags(fr, mfma_frags_F(re), mfma_frags_G(re), mfma_frags_L(re));
      // factorised G volume (mfma_tables.hpp): D_r = P_r Q
      const char* gq = std::getenv("SEIGEN_HIP_GQ");
      // default: degree 4 only (G<4,0> -2 %, step -0.7 .. -1 %; at degree 3, rank 10 of 20 on 4-row tiles, it is 12 % slower:
      // profiles/r04/kernel_experiments.txt); SEIGEN_HIP_GQ=0 / 1 forces it off / on for degrees 3 and 4
      if (!h->f32 && cfg->degree >= 3 && (gq ? std::atoi(gq) != 0 : cfg->degree >= SG_GQ_FROM_DEGREE)) {
        try {
          fr[3] = mfma_frags_Q(re);
          fr[4] = mfma_frags_P(re);
        } catch (const std::exception& e) {
          return fail(h, SG_ERR_ARG, e.what());
        }
      }
      // degree 4: the lifts take their own traces from a wave-private LDS stash (kernels_mfma.hip g_stash); 0 = from memory
      const char* gs = std::getenv("SEIGEN_HIP_GSTASH");
      h->gstash = !(gs && std::atoi(gs) == 0);
      break;
    }
    case Family::Tile2d: {
      h->t2c = tile2d_const(h->md);
      if (h->f32) set_frags(fr, tile2d_frags32_V(re, -1.0), tile2d_frags32_V(re, 1.0), tile2d_frags32_L(re));
      else set_frags(fr, tile2d_frags_V(re, -1.0), tile2d_frags_V(re, 1.0), tile2d_frags_L(re));
      break;
    }
  }
  HIPCHECK(h, h->Dt.upload(Dt.data(), Dt.size()));
  HIPCHECK(h, h->Lt.upload(Lt.data(), Lt.size()));
  HIPCHECK(h, h->md_dev.upload(&h->md, 1));
  if (h->family == Family::Mfma) {
    MfmaConst mk;
    try {
      mk = mfma_const(h->md);      // (checks the facet rule the F kernels' trace loads are written to: mfma_trace_lines)
    } catch (const std::exception& e) {
      return fail(h, SG_ERR_ARG, e.what());
    }
    HIPCHECK(h, h->mk_dev.upload(&mk, 1));
    std::vector<int32_t> ft, tab;
    mfma_trace_offsets(h->md, 9, ft);
    HIPCHECK(h, h->ftab_dev.upload(ft.data(), ft.size()));
    if ((h->md.ncube_pad / 16) * 6 * 16 >= ((int64_t)1 << 31))     // cell slots are int32 (288 GB hold far fewer cells)
      return fail(h, SG_ERR_ARG, "block too large for the MFMA path's neighbour table");
    build_nbr_table(h->md, tab);
    HIPCHECK(h, h->nbr_tab.upload(tab.data(), tab.size()));
  }
  return SG_OK;
}

// the four fields (zero), the operator fragments, the symmetric-stress flag, the diagnostic stamps
static int init_fields(sg_handle* h, const Frags& fr) {
  const int d = h->cfg.dim, nd = h->re.nd;
  for (int f = 0; f < 4; ++f) {
    size_t comps = field_is_stress(f) ? (size_t)d * d : (size_t)d;
    h->field_len[f] = (size_t)h->ncells * nd * comps;
    h->field_alloc[f] = (size_t)h->md.ncube_pad * h->ncls * nd * comps;
    const size_t n = h->f32 ? (h->field_alloc[f] + 1) / 2 : h->field_alloc[f];   // in doubles
    if (h->field.alloc(f, n) != hipSuccess) return fail(h, SG_ERR_NOMEM, "hipMalloc of a field buffer failed");
    HIPCHECK(h, hipMemset(h->field.write(f), 0, n * sizeof(double)));
  }
  DevBuf<double>* frag[5] = {&h->fragF, &h->fragG, &h->fragL, &h->fragQ, &h->fragP};
  for (int i = 0; i < 5; ++i)
    if (!fr[i].empty()) HIPCHECK(h, frag[i]->upload(fr[i].data(), fr[i].size()));
  if (family_interleaved(h->family)) {
    // symmetric-stress mode: fields start at zero, g only produces symmetric tensors;
    // left for good as soon as the user uploads a non-symmetric stress or source (SEIGEN_HIP_SYM=0: never entered)
    const char* sym_env = std::getenv("SEIGEN_HIP_SYM");
    h->sym = !(sym_env && std::strcmp(sym_env, "0") == 0);
    const int zero = 0;
    HIPCHECK(h, h->sym_flag.upload(&zero, 1));
  }
  if (std::getenv("SEIGEN_HIP_STAMPS")) {
    const std::vector<unsigned long long> zeros(32, 0);
    HIPCHECK(h, h->dbg.upload(zeros.data(), zeros.size()));
  }
  return SG_OK;
}

// block slots per CU of the family's stage kernels (registers and LDS)
static int blocks_per_cu(const sg_handle* h) {
  const int P = h->cfg.degree;
  return h->family == Family::Mfma ? mfma_blocks_per_cu(P, h->f32) : (h->family == Family::Hexm ? hexm_blocks_per_cu(P) : 2);
}

// persistent grids, graph replay, the streams and events
static int init_launch(sg_handle* h) {
  const sg_config* cfg = &h->cfg;
  // Persistent grid of the MFMA stage kernels: two blocks per CU fill every CU (registers and
  // LDS allow exactly two).  A block with halo neighbours leaves 1/16 of those slots empty, so
  // that RCCL's send/receive kernels can start WHILE an interior launch runs: behind a full
  // grid they only start when it drains (tools/overlap_probe.py), and a stage kernel that found
  // some of its own slots taken would run the late blocks' static shares one after the other.
  hipDeviceProp_t prop;
  HIPCHECK(h, hipGetDeviceProperties(&prop, cfg->device));
  h->ncu = prop.multiProcessorCount;
  const int slots = blocks_per_cu(h) * prop.multiProcessorCount;
  h->grid_full = slots / 8 * 8;
  h->grid_blocks = (cfg->nbr_mask != 0 ? slots - slots / 16 : slots) / 8 * 8;
  if (const char* gb = std::getenv("SEIGEN_HIP_GRID_BLOCKS")) h->grid_blocks = grid_blocks_override(std::atoi(gb));
  if (cfg->nbr_mask == 0) h->grid_full = h->grid_blocks;
  // F stages of a whole 3-D block: items dealt to the XCDs in chunks of 1/8 of a z-layer of cubes, so that all XCDs
  // sweep the block layer by layer together (the z-neighbour traces then meet the own rows of the next layer in the
  // Infinity Cache: F stages -3 %, profiles/r03/order_chunk_sweep.txt; the G stages do not gain and keep one
  // contiguous range per XCD).  SEIGEN_HIP_ORDER_CHUNK overrides (0 = off).
  h->order_chunk = 0;
  if (h->family == Family::Mfma && prepare_stage_mfma() != 0) return fail(h, SG_ERR_DEVICE, "the G stage kernels' dynamic LDS was refused");
  if (h->family == Family::Mfma) {
    const int64_t per_layer = ((int64_t)cfg->n[0] * cfg->n[1] + 15) / 16 * 6;
    if (cfg->n[2] >= 16) h->order_chunk = (int)std::max<int64_t>(6, (per_layer + 7) / 8);
  }
  if (const char* oc = std::getenv("SEIGEN_HIP_ORDER_CHUNK")) h->order_chunk = std::max(0, std::atoi(oc));
  h->no_whole = std::getenv("SEIGEN_HIP_NO_WHOLE") != nullptr;
  // 2-D tile kernels: a persistent grid of exactly the blocks the device holds of the stage's kernel (0 = asked of
  // the runtime per instantiation, stages.cpp tile_resident) - a wave sets up once and works through its share of the
  // items: 2-D P4 at N = 256 (the reference's benchmark protocol) 84.5 -> 93.4 G DoF-updates/s against one item per
  // wave, P3 +8 %, level elsewhere (profiles/r05/tile_grid_sweep.txt).  With a sponge the items differ in cost and a
  // static share can collect the expensive ones: then 251 blocks per XCD label - with an odd (prime) stride of 4 * 251
  // items a wave's items do not keep falling on the same column of the mesh, i.e. on the sponge strips at both ends of
  // every row (config 2: 0.228 ms per step with 768 blocks, 0.213 with 2008).
  h->tile_grid = 0;
  h->tile_grid_sponge = 2008;
  if (const char* tg = std::getenv("SEIGEN_HIP_TILE_GRID")) h->tile_grid = h->tile_grid_sponge = std::max(8, std::atoi(tg) / 8 * 8);
  const char* ge = std::getenv("SEIGEN_HIP_GRAPH");  // 0/1 overrides (measurements)
  const int64_t dofs = h->ncells * (int64_t)h->re.nd * (cfg->dim + cfg->dim * cfg->dim);
  h->graph_ok = ge ? (std::strcmp(ge, "0") != 0) : (dofs <= (int64_t)1 << 23);
  const char* ov = std::getenv("SEIGEN_HIP_OVERLAP");
  h->overlap = cfg->nbr_mask != 0 && !(ov && std::strcmp(ov, "0") == 0);
  int prio_lo = 0, prio_hi = 0;
  HIPCHECK(h, hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
  if (cfg->stream) {
    h->stream = (hipStream_t)cfg->stream;
  } else {
    HIPCHECK(h, hipStreamCreateWithPriority(&h->stream, hipStreamNonBlocking, h->overlap ? prio_hi : 0));
    h->own_stream = true;
  }
  if (h->overlap) {
    HIPCHECK(h, hipStreamCreateWithPriority(&h->stream2, hipStreamNonBlocking, prio_lo));
    HIPCHECK(h, hipEventCreateWithFlags(&h->ev_stage, hipEventDisableTiming));
    HIPCHECK(h, hipEventCreateWithFlags(&h->ev_second, hipEventDisableTiming));
  }
  HIPCHECK(h, hipEventCreate(&h->ev0));
  HIPCHECK(h, hipEventCreate(&h->ev1));
  HIPCHECK(h, hipDeviceSynchronize());
  return SG_OK;
}

extern "C" {

const char* sg_last_error(const sg_handle* h) { return h ? h->err.c_str() : g_create_err.c_str(); }

// device memory is released by the owners (DevBuf) when `delete h` runs; streams, events and graphs here, in order
void sg_destroy(sg_handle* h) {
  if (!h) return;
  (void)hipSetDevice(h->cfg.device);
  if (h->stream) (void)sync_all(h);
  if (h->dbg.get()) {
    unsigned long long v[32];
    if (hipMemcpy(v, h->dbg.get(), sizeof(v), hipMemcpyDeviceToHost) == hipSuccess)
      for (int k = 0; k < 4; ++k)
        std::fprintf(stderr, "[seigen_hip stamps] %s mode %d: items %llu  cycles/item: setup %.0f volume %.0f lifts %.0f epilogue %.0f"
                             "   (lifts: neighbour set-up %.0f, facet 0 %.0f, facets 1-3 %.0f)\n",
                     k < 2 ? "F" : "G", k & 1, v[8 * k + 4], v[8 * k + 4] ? (double)v[8 * k + 0] / v[8 * k + 4] : 0.0,
                     v[8 * k + 4] ? (double)v[8 * k + 1] / v[8 * k + 4] : 0.0, v[8 * k + 4] ? (double)v[8 * k + 2] / v[8 * k + 4] : 0.0,
                     v[8 * k + 4] ? (double)v[8 * k + 3] / v[8 * k + 4] : 0.0, v[8 * k + 4] ? (double)v[8 * k + 5] / v[8 * k + 4] : 0.0,
                     v[8 * k + 4] ? (double)v[8 * k + 6] / v[8 * k + 4] : 0.0, v[8 * k + 4] ? (double)v[8 * k + 7] / v[8 * k + 4] : 0.0);
  }
  comm_release(h);
  if (h->graph1) (void)hipGraphExecDestroy(h->graph1);
  if (h->graph8) (void)hipGraphExecDestroy(h->graph8);
  for (int i = 0; i < 2; ++i) {
    if (h->pin[i]) (void)hipHostFree(h->pin[i]);
    if (h->xfer_ev[i]) (void)hipEventDestroy(h->xfer_ev[i]);
  }
  if (h->ev0) (void)hipEventDestroy(h->ev0);
  if (h->ev1) (void)hipEventDestroy(h->ev1);
  for (hipEvent_t e : h->ev_pool) (void)hipEventDestroy(e);
  if (h->ev_stage) (void)hipEventDestroy(h->ev_stage);
  if (h->ev_second) (void)hipEventDestroy(h->ev_second);
  if (h->stream2) {
    (void)hipStreamSynchronize(h->stream2);
    (void)hipStreamDestroy(h->stream2);
  }
  if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

int sg_create(const sg_config* cfg, sg_handle** out) {
  if (!cfg || !out) {
    g_create_err = "null argument";
    return SG_ERR_ARG;
  }
  *out = nullptr;
  sg_handle* h = new sg_handle();
  Frags fr;
  int rc = init_element(cfg, h);
  if (rc == SG_OK) rc = init_family(h);
  if (rc == SG_OK) rc = family_tables(h, fr);
  if (rc == SG_OK) rc = init_fields(h, fr);
  if (rc == SG_OK) rc = init_launch(h);
  if (rc != SG_OK) {
    g_create_err = h->err;
    sg_destroy(h);
    return rc;
  }
  *out = h;
  return SG_OK;
}

int sg_get_stream(const sg_handle* h, void** stream) {
  if (!h || !stream) return SG_ERR_ARG;
  *stream = (void*)h->stream;
  return SG_OK;
}

int sg_get_second_stream(const sg_handle* h, void** stream) {
  if (!h || !stream) return SG_ERR_ARG;
  *stream = (void*)h->stream2;
  return SG_OK;
}

int sg_get_info(const sg_handle* h, sg_info_t* out) {
  if (!h || !out) return SG_ERR_ARG;
  const int d = h->cfg.dim;
  out->dim = d;
  out->degree = h->cfg.degree;
  out->nd = h->re.nd;
  out->nf = h->re.nf;
  out->nfaces = h->re.nfaces;
  out->nclasses = h->ncls;
  out->ncells = h->ncells;
  out->u_dofs = (int64_t)d * h->re.nd * h->ncells;
  out->s_dofs = (int64_t)d * d * h->re.nd * h->ncells;
  for (int s = 0; s < 6; ++s) {
    int axis = s >> 1;
    if (axis >= d) {
      out->halo_faces[s] = 0;
      continue;
    }
    int64_t n2 = 1;
    for (int a = 0; a < 3; ++a)
      if (a != axis) n2 *= h->cfg.n[a];
    out->halo_faces[s] = (int32_t)(n2 * h->md.halo_per_cube);
  }
  return SG_OK;
}

int sg_sync(sg_handle* h) {
  if (!h) return SG_ERR_ARG;
  HIPCHECK(h, hipSetDevice(h->cfg.device));
  if (int rc = join_second(h)) return rc;
  HIPCHECK(h, sync_all(h));
  return SG_OK;
}

int sg_node_coords(const sg_handle* h, int degree, double* out, size_t nbytes) {
  if (!h) return SG_ERR_ARG;
  return sg_block_node_coords(&h->cfg, degree, out, nbytes);
}

// Every setter below computes and uploads into locals first and assigns to the handle only once nothing can fail any more:
// a call that fails leaves the handle as it was.  (The handle's old tables may still be read by queued work: sync_all
// before they are replaced.)

int sg_set_params(sg_handle* h, double density, double dt, const double* lambda, const double* mu, int per_cell) {
  if (!h || !lambda || !mu) return SG_ERR_ARG;
  HIPCHECK(h, hipSetDevice(h->cfg.device));
  DevBuf<double> lam_d, mu_d;
  if (per_cell) {
    HIPCHECK(h, lam_d.upload(lambda, (size_t)h->ncells));
    HIPCHECK(h, mu_d.upload(mu, (size_t)h->ncells));
  }
  HIPCHECK(h, sync_all(h));
  h->rho = density;
  h->rho_physical = 0;
  h->rho2_d.reset();
  h->dt = dt;
  h->per_cell = per_cell ? 1 : 0;
  if (per_cell) {
    h->lam_d = std::move(lam_d);
    h->mu_d = std::move(mu_d);
  }
  h->lam0 = lambda[0];
  h->mu0 = mu[0];
  h->params_set = true;
  h->epoch += 1;
  return SG_OK;
}

int sg_set_density(sg_handle* h, const double* rho, int per_cell, int physical) {
  if (!h || !rho) return SG_ERR_ARG;
  HIPCHECK(h, hipSetDevice(h->cfg.device));
  DevBuf<double> rho2_d;
  const int64_t n = per_cell ? h->ncells : 1;
  std::vector<double> r2((size_t)n * 2);
  for (int64_t e = 0; e < n; ++e) {
    if (physical && rho[e] == 0.0) return fail(h, SG_ERR_ARG, "sg_set_density: zero density");
    r2[2 * (size_t)e] = physical ? 1.0 : rho[e];
    r2[2 * (size_t)e + 1] = physical ? 1.0 / rho[e] : 1.0;
  }
  if (per_cell) HIPCHECK(h, rho2_d.upload(r2.data(), r2.size()));
  HIPCHECK(h, sync_all(h));
  h->rho2_d = std::move(rho2_d);
  h->rho_physical = physical ? 1 : 0;
  h->rho = rho[0];
  h->epoch += 1;
  return SG_OK;
}

// What each cell gets - nothing, a scalar, dim + 1 numbers, a matrix - is decided by plan_sponge (sponge_tables.cpp: plain
// C++, under the CPU sanitizers); this function checks the plan against the device, uploads it and puts it in place.
int sg_set_absorption(sg_handle* h, const double* sigma_nodes, int sigma_degree) {
  if (!h) return SG_ERR_ARG;
  if (sigma_nodes && (sigma_degree < 1 || sigma_degree > 6)) return fail(h, SG_ERR_ARG, "sigma_degree must be 1..6");
  HIPCHECK(h, hipSetDevice(h->cfg.device));
  SpongeTables sp;
  if (sigma_nodes) {
    const int d = h->cfg.dim, nd = h->re.nd;
    SpongeRequest rq;
    rq.dim = d;
    rq.degree = h->cfg.degree;
    rq.kind = h->re.kind;
    rq.sigma_degree = sigma_degree;
    rq.ncells = h->ncells;
    rq.ncls = h->ncls;
    rq.gw = (int)h->md.gw;
    // a sigma that is one value on all nodes of a cell (the piecewise-constant sponges of the reference's problem scripts,
    // explosive_source_lf4.py:42-45) is applied as sigma u at the node
    rq.want_scalar = family_interleaved(h->family);
    rq.pre_family = family_sponge_pre(h->family);
    // Affine cells take dim + 1 numbers (kernels.hip sponge_pre_affine_kernel, kernels_mfma.hip sponge_affine_mfma);
    // SEIGEN_HIP_SPONGE_AFFINE=0 sends them through their matrices (tests: the two must agree).  The lane kernels' cells -
    // hexahedra DQ_1 / DQ_2, gw = 64 - have matrices of at most 27 x 27 shared through the caches: there the matrix pre-pass
    // is the faster one (64.5 against 61.9 G at 96^3 DQ_2, profiles/r06/affine_sponge.txt); '1' forces the affine path
    const char* aff_env = std::getenv("SEIGEN_HIP_SPONGE_AFFINE");
    rq.try_affine = rq.pre_family && !(aff_env && aff_env[0] == '0') && (h->family != Family::Lane || (aff_env && aff_env[0] == '1'));
    rq.line_layout = family_pre_lines(h->family);
    SpongePlan pl;
    try {
      pl = plan_sponge(rq, sigma_nodes);
    } catch (const std::exception& e) {
      return fail(h, SG_ERR_ARG, std::string("sg_set_absorption: ") + e.what());
    }
    const bool pre = rq.pre_family && pl.nslots > 0, affine = rq.pre_family && pl.naffine > 0;
    const bool aff_mfma = affine && h->family == Family::Mfma && !h->f32;   // on the matrix pipe (kernels_mfma.hip sponge_affine_mfma)
    if (affine) {
      if (rq.gw * nd > SG_SPONGE_AFFINE_MAX_ROWS)
        return fail(h, SG_ERR_STATE, "sg_set_absorption: the affine-sigma pre-pass takes at most " +
                                         std::to_string(SG_SPONGE_AFFINE_MAX_ROWS) + " (cell, node) rows per item (set SEIGEN_HIP_SPONGE_AFFINE=0)");
      const size_t lds = sponge_pre_affine_lds(pl.W, !pl.dense, nd, d, rq.gw);
      if (lds > ((size_t)150 << 10))
        return fail(h, SG_ERR_STATE, "sg_set_absorption: the affine-sigma tables of this element do not fit the LDS (set SEIGEN_HIP_SPONGE_AFFINE=0)");
      int ncu = 0;
      HIPCHECK(h, hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, h->cfg.device));
      sp.aff_grid = aff_mfma ? prepare_sponge_affine_mfma(h->cfg.degree, ncu) : prepare_sponge_pre_affine(d, h->f32, lds, ncu);
      if (sp.aff_grid <= 0) return fail(h, SG_ERR_DEVICE, "sg_set_absorption: the affine-sigma pre-pass cannot be set up on this device");
      // SEIGEN_HIP_GRID_BLOCKS also caps this grid (hostlogic.hpp affine_grid_cap): tests make the pre-pass loop on small meshes
      if (const char* gb = std::getenv("SEIGEN_HIP_GRID_BLOCKS")) sp.aff_grid = affine_grid_cap(sp.aff_grid, std::atoi(gb));
    }
    hipError_t e = hipSuccess;
    auto up = [&e](auto& buf, const auto& v) {
      if (e == hipSuccess) e = buf.upload(v.data(), v.size());
    };
    up(sp.slot, pl.slot);
    sp.nslots = pl.nslots;
    sp.pre_lines = (rq.line_layout && pl.nslots > 0) ? 1 : 0;
    if (pre) {
      const size_t pre_bytes = (size_t)pl.nslots * nd * d * (h->f32 ? sizeof(float) : sizeof(double));
      up(sp.cells, pl.cells);
      up(sp.mat, pl.mat_of);
      if (e == hipSuccess) e = sp.pre.alloc(pre_bytes);
      if (e == hipSuccess) e = hipMemset(sp.pre.get(), 0, pre_bytes);
      // the cells with a matrix: every slot in order, or - line layout, affine cells among them - a list
      sp.nmat_slots = (int32_t)pl.mat_slots.size();
      if (sp.pre_lines || pl.naffine > 0) up(sp.mat_slots, pl.mat_slots);
    }
    if (affine) {
      up(sp.aff_items, pl.items);
      up(sp.aff_slots, pl.item_slots);
      up(sp.aff_coef, pl.aff_coef);
      up(sp.aff_X, pl.X);
      if (!pl.dense) up(sp.aff_col, pl.col);
      if (aff_mfma) up(sp.aff_frag, mfma_frags_dense(h->re, pl.Xd.data(), 3));
      sp.aff_nitems = (int32_t)pl.items.size();
      sp.aff_W = pl.W;
    }
    if (!pl.sig.empty()) up(sp.sigma, pl.sig);
    up(sp.B, pl.B);
    if (e != hipSuccess)
      return fail(h, e == hipErrorOutOfMemory ? SG_ERR_NOMEM : SG_ERR_DEVICE,
                  std::string("sg_set_absorption: hipMalloc / upload of the sponge tables failed: ") + hipGetErrorString(e));
  }
  HIPCHECK(h, sync_all(h));
  h->sponge = std::move(sp);
  h->epoch += 1;
  return SG_OK;
}

// sg_set_source and sg_set_source_separable: nsteps slices of values (-1: one that holds at every step), or - weights
// given - one slice scaled by weights[k] at step k < nsteps.  Which nodes are merged, their order (SG_REGION_FIRST first),
// their device offsets, the fused table of the 2-D tile family and whether the values are symmetric is decided by
// plan_source (source_tables.cpp: plain C++, under the CPU sanitizers); this function uploads the plan and puts it in place.
static int set_source(sg_handle* h, int64_t nnz, const int64_t* nodes, int64_t nsteps, const double* values, const double* weights) {
  HIPCHECK(h, hipSetDevice(h->cfg.device));
  SourceTables src;
  DevBuf<int64_t> ctr;        // the device-side step counter, where the handle has none yet
  bool leave_sym = false;
  if (nnz != 0 && nsteps != 0) {
    if (!nodes || !values || nsteps < -1) return SG_ERR_ARG;
    SourceRequest rq;
    rq.dim = h->cfg.dim;
    rq.L = layout(h);
    rq.ncells = h->ncells;
    rq.ncube_pad = h->md.ncube_pad;
    std::copy_n(h->cfg.n, 3, rq.n);
    region_boxes(h, SG_REGION_FIRST, rq.first);
    rq.want_fused = family_fused_source(h->family) && !std::getenv("SEIGEN_HIP_SOURCE_LAUNCH");
    rq.sym = h->sym;
    SourcePlan pl;
    try {
      pl = plan_source(rq, nnz, nodes, nsteps, values, weights);
    } catch (const std::exception& e) {
      return fail(h, SG_ERR_ARG, std::string("sg_set_source: ") + e.what());
    }
    src.nnz = pl.nnz;
    src.nfirst = pl.nfirst;
    src.is_static = pl.is_static;
    src.nsteps = pl.nsteps;
    HIPCHECK(h, src.nodes.upload(pl.offs.data(), pl.offs.size()));
    HIPCHECK(h, src.values.upload(pl.vals.data(), pl.vals.size()));
    if (weights) {
      HIPCHECK(h, src.weights_d.upload(pl.weights.data(), pl.weights.size()));
      src.weights = std::move(pl.weights);
    }
    if (!pl.slot.empty()) {   // the G stage kernels add the source themselves (StageArgs::src_slot / src_idx)
      HIPCHECK(h, src.slot.upload(pl.slot.data(), pl.slot.size()));
      HIPCHECK(h, src.idx.upload(pl.idx.data(), pl.idx.size()));
      src.fused = true;
    }
    if (!h->src_ctr_d.get()) {   // device-side step counter for graph replay (stages.cpp sg_step), kept across sources
      const int64_t zero = 0;
      HIPCHECK(h, ctr.upload(&zero, 1));
    }
    leave_sym = h->sym && !pl.symmetric;
  }
  HIPCHECK(h, sync_all(h));
  // (the last step that can fail, and it fails before the storage mode changes)
  if (leave_sym)
    if (int rc = leave_sym_mode(h)) return rc;
  if (ctr.get()) h->src_ctr_d = std::move(ctr);
  h->src = std::move(src);
  h->src_step = 0;
  h->epoch += 1;
  return SG_OK;
}

int sg_set_source(sg_handle* h, int64_t nnz, const int64_t* nodes, int64_t nsteps, const double* values) {
  if (!h || nnz < 0) return SG_ERR_ARG;
  return set_source(h, nnz, nodes, nsteps, values, nullptr);
}

int sg_set_source_separable(sg_handle* h, int64_t nnz, const int64_t* nodes, const double* pattern, int64_t nsteps,
                            const double* weights) {
  if (!h || nnz < 0 || nsteps < 0) return SG_ERR_ARG;
  if (nnz != 0 && nsteps != 0 && !weights) return SG_ERR_ARG;
  return set_source(h, nnz, nodes, nsteps, pattern, weights);
}

int sg_set_source_box_ricker(sg_handle* h, const double* lo, const double* hi, double a, double t0, double t_first,
                             double dt_step, int64_t nsteps) {
  if (!h || !lo || !hi || nsteps < 0) return SG_ERR_ARG;
  const int d = h->cfg.dim;
  NodeGeom G;
  if (!G.init(&h->cfg, h->cfg.degree)) return SG_ERR_ARG;
  std::vector<int64_t> nodes;
  try {
    nodes = box_nodes(G, lo, hi);
  } catch (const std::exception& e) {
    return fail(h, SG_ERR_ARG, std::string("source box: ") + e.what());
  }
  if (nodes.empty() || nsteps == 0) return sg_set_source(h, 0, nullptr, 0, nullptr);
  std::vector<double> pattern(nodes.size() * (size_t)d * d, 0.0);
  for (size_t j = 0; j < nodes.size(); ++j)
    for (int i = 0; i < d; ++i) pattern[(j * d + i) * d + i] = 1.0;
  const std::vector<double> w = ricker_weights(a, t0, t_first, dt_step, nsteps);
  return sg_set_source_separable(h, (int64_t)nodes.size(), nodes.data(), pattern.data(), nsteps, w.data());
}

// The receivers: located on the host and tabulated with the element's basis (hostlogic.hpp plan_receivers: locate_point,
// the rule of sg_locate_points), uploaded into locals, and moved into the handle once nothing can fail any more.
int sg_set_receivers(sg_handle* h, int64_t nrec, const double* pts, int what, int64_t every, int64_t capacity,
                     int32_t* owned) {
  if (!h) return SG_ERR_ARG;
  if (nrec < 0) return fail(h, SG_ERR_ARG, "sg_set_receivers: nrec must be >= 0");
  if (nrec > 0 && !pts) return fail(h, SG_ERR_ARG, "sg_set_receivers: no points");
  if (nrec > 0 && (what < 1 || what > 3)) return fail(h, SG_ERR_ARG, "sg_set_receivers: what must be 1 (velocity), 2 (stress) or 3");
  if (nrec > 0 && every < 1) return fail(h, SG_ERR_ARG, "sg_set_receivers: every must be >= 1");
  if (nrec > 0 && capacity < 0) return fail(h, SG_ERR_ARG, "sg_set_receivers: capacity must be >= 0");
  HIPCHECK(h, hipSetDevice(h->cfg.device));
  ReceiverTables rt;
  ReceiverPlan pl;
  if (nrec > 0) {
    NodeGeom G;
    if (!G.init(&h->cfg, h->cfg.degree)) return fail(h, SG_ERR_ARG, "sg_set_receivers: cell type");
    try {
      pl = plan_receivers(G, layout(h), h->re.kind, nrec, pts, what, capacity);
    } catch (const std::exception& e) {
      return fail(h, SG_ERR_ARG, std::string("sg_set_receivers: ") + e.what());
    }
    rt.nrec = nrec;
    rt.nown = (int64_t)pl.row.size();
    rt.what = what;
    rt.ncomp = pl.ncomp;
    rt.clock.every = every;
    rt.clock.count = capacity;
    const size_t tlen = (size_t)(capacity * rt.nown * rt.ncomp);
    HIPCHECK(h, rt.item.upload(pl.item.data(), pl.item.size()));
    HIPCHECK(h, rt.lane.upload(pl.lane.data(), pl.lane.size()));
    HIPCHECK(h, rt.phi.upload(pl.phi.data(), pl.phi.size()));
    if (rt.trace.alloc(tlen) != hipSuccess) return fail(h, SG_ERR_NOMEM, "sg_set_receivers: hipMalloc of the trace failed");
    HIPCHECK(h, hipMemset(rt.trace.get(), 0, std::max<size_t>(tlen, 1) * sizeof(double)));
    rt.row = std::move(pl.row);
  }
  if (int rc = arm_hook(h, h->rec, rt, nrec > 0)) return rc;
  if (owned) std::memcpy(owned, pl.own.data(), pl.own.size() * sizeof(int32_t));
  return SG_OK;
}

int sg_get_receivers(sg_handle* h, double* out, size_t nbytes, int64_t* nsamples) {
  if (!h || !nsamples) return SG_ERR_ARG;
  const ReceiverTables& rt = h->rec;
  const size_t want = (size_t)(rt.clock.count * rt.nrec * rt.ncomp) * sizeof(double);
  if (nbytes != want || (want > 0 && !out))
    return fail(h, SG_ERR_ARG, "sg_get_receivers: the buffer must hold capacity x nrec x ncomp doubles (" + std::to_string(want) + " bytes)");
  HIPCHECK(h, hipSetDevice(h->cfg.device));
  HIPCHECK(h, sync_all(h));
  const int64_t n = rt.clock.samples();
  std::vector<double> t((size_t)(n * rt.nown * rt.ncomp));
  if (!t.empty()) HIPCHECK(h, hipMemcpy(t.data(), rt.trace.get(), t.size() * sizeof(double), hipMemcpyDeviceToHost));
  if (want > 0) std::memset(out, 0, want);
  for (int64_t j = 0; j < n; ++j)
    for (int64_t r = 0; r < rt.nown; ++r)
      std::memcpy(out + (j * rt.nrec + rt.row[(size_t)r]) * rt.ncomp, t.data() + (j * rt.nown + r) * rt.ncomp,
                  (size_t)rt.ncomp * sizeof(double));
  *nsamples = n;
  return SG_OK;
}

// The injectors: located, weighted and grouped by cell on the host (hostlogic.hpp injector_plan: locate_point, the rule of
// sg_locate_points; psi from the element's Mhat^-1), uploaded into a local InjectTables.  Nothing of the handle changes here:
// leave_sym tells the caller that the stress table is not symmetric and the block has to leave symmetric storage - which the
// caller does once nothing else of its own can fail (a failed call leaves the handle as it was, the storage mode included).
static int build_injectors(sg_handle* h, const char* who, int64_t npts, const double* pts, int what, int64_t nsteps, const double* amp,
                           InjectTables& it, std::vector<int32_t>& own, bool& leave_sym) {
  if (npts < 0 || nsteps < 0) return fail(h, SG_ERR_ARG, std::string(who) + ": npts and nsteps must be >= 0");
  if (what < 1 || what > 3) return fail(h, SG_ERR_ARG, std::string(who) + ": what must be 1 (velocity), 2 (stress) or 3");
  if (!pts || !amp) return fail(h, SG_ERR_ARG, std::string(who) + ": no points or no amplitudes");
  NodeGeom G;
  if (!G.init(&h->cfg, h->cfg.degree)) return fail(h, SG_ERR_ARG, std::string(who) + ": cell type");
  InjectorPlan pl;
  std::vector<double> table;
  try {
    pl = injector_plan(G, layout(h), h->re, npts, pts, what);
    table = injector_gather(pl, npts, nsteps, amp);
  } catch (const std::exception& e) {
    return fail(h, SG_ERR_ARG, std::string(who) + ": " + e.what());
  }
  it.npts = npts;
  it.nown = (int64_t)pl.row.size();
  it.ngroups = (int64_t)pl.cell.size();
  it.what = what;
  it.ncomp = pl.ncomp;
  it.clock.count = nsteps;
  HIPCHECK(h, it.item.upload(pl.item.data(), pl.item.size()));
  HIPCHECK(h, it.lane.upload(pl.lane.data(), pl.lane.size()));
  HIPCHECK(h, it.start.upload(pl.start.data(), pl.start.size()));
  HIPCHECK(h, it.psi.upload(pl.psi.data(), pl.psi.size()));
  HIPCHECK(h, it.amp.upload(table.data(), table.size()));
  own = std::move(pl.own);
  leave_sym = h->sym && !injector_symmetric(pl, h->cfg.dim, what, nsteps, table);
  return SG_OK;
}

int sg_set_injectors(sg_handle* h, int64_t npts, const double* pts, int what, int64_t nsteps, const double* amp, int32_t* owned) {
  if (!h) return SG_ERR_ARG;
  HIPCHECK(h, hipSetDevice(h->cfg.device));
  InjectTables it;
  std::vector<int32_t> own;
  bool leave_sym = false;
  if (npts != 0 && nsteps != 0) {
    if (int rc = build_injectors(h, "sg_set_injectors", npts, pts, what, nsteps, amp, it, own, leave_sym)) return rc;
  } else if (npts < 0 || nsteps < 0) {
    return fail(h, SG_ERR_ARG, "sg_set_injectors: npts and nsteps must be >= 0");
  }
  if (int rc = arm_hook(h, h->inj, it, it.npts > 0, leave_sym)) return rc;
  if (owned && !own.empty()) std::memcpy(owned, own.data(), own.size() * sizeof(int32_t));
  return SG_OK;
}

int sg_inject(sg_handle* h, int64_t npts, const double* pts, int what, const double* amp) {
  if (!h) return SG_ERR_ARG;
  if (npts == 0) return SG_OK;
  HIPCHECK(h, hipSetDevice(h->cfg.device));
  InjectTables it;
  std::vector<int32_t> own;
  bool leave_sym = false;
  if (int rc = build_injectors(h, "sg_inject", npts, pts, what, 1, amp, it, own, leave_sym)) return rc;
  if (it.nown == 0) return SG_OK;   // (no point of this block's: its table is symmetric)
  if (int rc = join_second(h)) return rc;
  // A table that is not symmetric: the mirrors, then the launch in full storage; the block leaves symmetric storage once
  // both are queued and done - a call that fails before leaves the handle as it was.
  if (leave_sym)
    if (int rc = queue_sym_mirrors(h)) return rc;
  if (int rc = queue_inject(h, h->stream, it, nullptr, 1, leave_sym ? 0 : -1)) return rc;
  HIPCHECK(h, sync_all(h));   // the tables are this call's: they go when it returns
  if (leave_sym) {
    h->sym = false;
    h->epoch += 1;
  }
  return SG_OK;
}

// The monitor (kernels_measure.hip): tables and trace are built in locals and moved into the handle once nothing can fail
// any more, as the receivers' are.
int sg_set_monitor(sg_handle* h, int64_t every, int64_t capacity, const double* w, int per_cell) {
  if (!h) return SG_ERR_ARG;
  if (every < 0) return fail(h, SG_ERR_ARG, "sg_set_monitor: every must be >= 0 (0 disarms)");
  if (every > 0 && capacity < 1) return fail(h, SG_ERR_ARG, "sg_set_monitor: capacity must be >= 1");
  if (every > 0 && per_cell && !w) return fail(h, SG_ERR_ARG, "sg_set_monitor: per-cell weights without weights");
  if (every > 0 && capacity > ((int64_t)1 << 32)) return fail(h, SG_ERR_ARG, "sg_set_monitor: more than 2^32 samples");
  HIPCHECK(h, hipSetDevice(h->cfg.device));
  MonitorTables mt;
  if (every > 0) {
    if (int rc = measure_prepare(h)) return rc;
    mt.armed = true;
    mt.clock.every = every;
    mt.clock.count = capacity;
    if (w && per_cell) HIPCHECK(h, mt.w.upload(w, (size_t)h->ncells * 3));
    if (w && !per_cell) std::memcpy(mt.w0, w, sizeof(mt.w0));
    if (mt.trace.alloc((size_t)capacity * 5) != hipSuccess) return fail(h, SG_ERR_NOMEM, "sg_set_monitor: hipMalloc of the trace failed");
    HIPCHECK(h, hipMemset(mt.trace.get(), 0, (size_t)capacity * 5 * sizeof(double)));
  }
  return arm_hook(h, h->mon, mt, every > 0);
}

int sg_get_monitor(sg_handle* h, double* out, size_t nbytes, int64_t* nsamples) {
  if (!h || !nsamples) return SG_ERR_ARG;
  const MonitorTables& mt = h->mon;
  const size_t want = mt.armed ? (size_t)mt.clock.count * 5 * sizeof(double) : 0;
  if (nbytes != want || (want > 0 && !out))
    return fail(h, SG_ERR_ARG, "sg_get_monitor: the buffer must hold capacity x 5 doubles (" + std::to_string(want) + " bytes)");
  HIPCHECK(h, hipSetDevice(h->cfg.device));
  HIPCHECK(h, sync_all(h));
  const int64_t n = mt.armed ? mt.clock.samples() : 0;
  if (want > 0) std::memset(out, 0, want);
  if (n > 0) HIPCHECK(h, hipMemcpy(out, mt.trace.get(), (size_t)n * 5 * sizeof(double), hipMemcpyDeviceToHost));
  *nsamples = n;
  return SG_OK;
}

// The correlation (kernels_xcorr.hip).  The first successful call builds the handle's tables - the operator in the form the
// kernel takes, the zeroed accumulator, the two events - in locals and moves them into the handle after the launch is queued;
// every refusal comes before anything is queued.
static int correlation_prepare(sg_handle* a, CorrelationTables& ct) {
  const int gw = (int)a->md.gw, nd = a->re.nd;
  const int tensor = a->cfg.diagonal == SG_DIAGONAL_QUAD ? 1 : 0;
  const char* form = std::getenv("SEIGEN_HIP_XCORR");
  ct.mfma = xcorr_has_mfma(a->cfg.dim, nd, gw, tensor) && !(form && std::strcmp(form, "lds") == 0);
  ct.nitems = (a->md.ncube_pad / gw) * a->ncls;
  ct.ipw = ct.mfma ? 0 : xcorr_items_per_group(nd, gw);
  ct.grid = (ct.mfma || ct.ipw > 0) ? prepare_xcorr(nd, gw, ct.ipw, ct.mfma ? 1 : 0, a->f32, a->ncu) : -1;
  if (ct.grid <= 0) return fail(a, SG_ERR_DEVICE, "sg_correlate: no kernel for this element");
  const std::vector<double> op = ct.mfma ? xcorr_mass_tiles(a->re.Mhat, nd) : a->re.Mhat;
  HIPCHECK(a, ct.M.upload(op.data(), op.size()));
  if (ct.acc.alloc((size_t)a->ncells * 3) != hipSuccess) return fail(a, SG_ERR_NOMEM, "sg_correlate: hipMalloc of the accumulator failed");
  // (on a's stream, ahead of the launch that adds to it: the legacy stream is not ordered against a non-blocking one)
  HIPCHECK(a, hipMemsetAsync(ct.acc.get(), 0, (size_t)a->ncells * 3 * sizeof(double), a->stream));
  HIPCHECK(a, ct.ev_in.create());
  HIPCHECK(a, ct.ev_out.create());
  ct.ready = true;
  return SG_OK;
}

int sg_correlate(sg_handle* a, sg_handle* b, const double w[3]) {
  if (!a) return SG_ERR_ARG;
  if (!b) return fail(a, SG_ERR_ARG, "sg_correlate: no second handle");
  if (b != a) {
    const std::string diff = xcorr_first_difference(a->cfg, (int)a->md.gw, b->cfg, (int)b->md.gw);
    if (!diff.empty()) return fail(a, SG_ERR_ARG, "sg_correlate: the handles differ in " + diff);
  }
  HIPCHECK(a, hipSetDevice(a->cfg.device));
  CorrelationTables fresh;
  if (!a->cor.ready)
    if (int rc = correlation_prepare(a, fresh)) return rc;
  const CorrelationTables& ct = a->cor.ready ? a->cor : fresh;
  xcorr::Args x;
  std::memset(&x, 0, sizeof(x));
  x.ua = a->field.read(SG_FIELD_U);
  x.sa = a->field.read(SG_FIELD_S);
  x.ub = b->field.read(SG_FIELD_U);
  x.sb = b->field.read(SG_FIELD_S);
  x.M = ct.M.get();
  x.acc = ct.acc.get();
  double detj = 1.0;
  for (int k = 0; k < a->cfg.dim; ++k) detj *= a->cfg.h[k];
  for (int k = 0; k < 3; ++k) x.wd[k] = (w ? w[k] : 1.0) * detj;
  x.nitems = ct.nitems;
  x.ncube = a->md.ncube;
  x.nd = a->re.nd;
  x.dim = a->cfg.dim;
  x.gw = (int32_t)a->md.gw;
  x.ncls = a->ncls;
  x.ipw = ct.ipw;
  const std::vector<XcorrComp> comps = xcorr_components(a->cfg.dim, a->sym, b->sym);
  x.ncomp = (int32_t)comps.size();
  for (size_t k = 0; k < comps.size(); ++k) {
    x.comp_a[k] = comps[k].comp_a;
    x.comp_b[k] = comps[k].comp_b;
    x.diag[k] = comps[k].diag ? 1 : 0;
    x.mult[k] = comps[k].mult;
  }
  // behind everything both handles have queued; b's later work behind the launch
  if (int rc = join_second(a)) return rc;
  if (b != a) {
    if (join_second(b) != SG_OK) return fail(a, SG_ERR_DEVICE, std::string("sg_correlate: second handle: ") + b->err);
    HIPCHECK(a, hipEventRecord(ct.ev_in.get(), b->stream));
    HIPCHECK(a, hipStreamWaitEvent(a->stream, ct.ev_in.get(), 0));
  }
  if (launch_xcorr(x, ct.mfma ? 1 : 0, a->f32, ct.grid, a->stream) != 0) return fail(a, SG_ERR_DEVICE, "correlation launch failed");
  if (b != a) {
    HIPCHECK(a, hipEventRecord(ct.ev_out.get(), a->stream));
    HIPCHECK(a, hipStreamWaitEvent(b->stream, ct.ev_out.get(), 0));
  }
  if (!a->cor.ready) a->cor = std::move(fresh);
  return SG_OK;
}

int sg_get_correlation(sg_handle* a, double* out, size_t nbytes) {
  if (!a) return SG_ERR_ARG;
  if (!a->cor.ready) return fail(a, SG_ERR_STATE, "sg_get_correlation: no correlation yet (sg_correlate)");
  const size_t want = (size_t)a->ncells * 3 * sizeof(double);
  if (nbytes != want || !out)
    return fail(a, SG_ERR_ARG, "sg_get_correlation: the buffer must hold ncells x 3 doubles (" + std::to_string(want) + " bytes)");
  HIPCHECK(a, hipSetDevice(a->cfg.device));
  HIPCHECK(a, sync_all(a));
  HIPCHECK(a, hipMemcpy(out, a->cor.acc.get(), want, hipMemcpyDeviceToHost));
  return SG_OK;
}

int sg_reset_correlation(sg_handle* a, int release) {
  if (!a) return SG_ERR_ARG;
  if (!a->cor.ready) return SG_OK;
  HIPCHECK(a, hipSetDevice(a->cfg.device));
  if (release) {
    HIPCHECK(a, sync_all(a));
    a->cor = CorrelationTables();
    return SG_OK;
  }
  HIPCHECK(a, hipMemsetAsync(a->cor.acc.get(), 0, (size_t)a->ncells * 3 * sizeof(double), a->stream));
  return SG_OK;
}

// The spectra (kernels_spectra.hip): weight tables and zeroed accumulators are built in locals and moved into the handle once
// nothing can fail any more, as the receivers' and the monitor's are.
int sg_set_spectra(sg_handle* h, int nfreq, int what, int64_t every, int64_t nsamples, const double* wu, const double* ws) {
  if (!h) return SG_ERR_ARG;
  if (nfreq < 0 || nfreq > SG_SPECTRA_MAX_FREQ)
    return fail(h, SG_ERR_ARG, "sg_set_spectra: nfreq must be 0 (disarm) .. " + std::to_string(SG_SPECTRA_MAX_FREQ));
  SpectraTables sp;
  HIPCHECK(h, hipSetDevice(h->cfg.device));
  if (nfreq > 0) {
    if (what < 1 || what > 3) return fail(h, SG_ERR_ARG, "sg_set_spectra: what must be 1 (velocity), 2 (stress) or 3");
    if (every < 1) return fail(h, SG_ERR_ARG, "sg_set_spectra: every must be >= 1");
    if (nsamples < 1) return fail(h, SG_ERR_ARG, "sg_set_spectra: nsamples must be >= 1");
    if (nsamples > ((int64_t)1 << 32)) return fail(h, SG_ERR_ARG, "sg_set_spectra: more than 2^32 samples");
    const double* tables[2] = {wu, ws};
    const int fields[2] = {SG_FIELD_U, SG_FIELD_S};
    for (int k = 0; k < 2; ++k)
      if ((what & (1 << k)) && !tables[k]) return fail(h, SG_ERR_ARG, "sg_set_spectra: no weight table for a selected field");
    sp.nfreq = nfreq;
    sp.what = what;
    sp.clock.every = every;
    sp.clock.count = nsamples;
    for (int k = 0; k < 2; ++k) {
      if (!(what & (1 << k))) continue;
      const size_t n = (size_t)2 * nfreq * h->field_alloc[fields[k]];
      if (sp.acc[k].alloc(n) != hipSuccess || sp.w[k].alloc((size_t)nsamples * nfreq * 2) != hipSuccess) {
        (void)hipGetLastError();
        return fail(h, SG_ERR_NOMEM, "sg_set_spectra: hipMalloc of the accumulators (" + std::to_string(n * sizeof(double)) +
                                         " bytes) or of the weight table failed");
      }
    }
    for (int k = 0; k < 2; ++k) {
      if (!(what & (1 << k))) continue;
      HIPCHECK(h, hipMemcpy(sp.w[k].get(), tables[k], (size_t)nsamples * nfreq * 2 * sizeof(double), hipMemcpyHostToDevice));
      // (on the handle's stream, which the host waits for below: the legacy stream is not ordered against a non-blocking one)
      HIPCHECK(h, hipMemsetAsync(sp.acc[k].get(), 0, (size_t)2 * nfreq * h->field_alloc[fields[k]] * sizeof(double), h->stream));
    }
  }
  return arm_hook(h, h->spc, sp, nfreq > 0);
}

int sg_get_spectrum(sg_handle* h, int field, int freq, int part, double* host, size_t nbytes) {
  if (!h) return SG_ERR_ARG;
  if (field < 0 || field > 1) return fail(h, SG_ERR_ARG, "sg_get_spectrum: field is 0 (velocity) or 1 (stress)");
  const SpectraTables& sp = h->spc;
  if (!sp.has(field)) return fail(h, SG_ERR_STATE, "sg_get_spectrum: no spectra armed for this field (sg_set_spectra)");
  if (freq < 0 || freq >= sp.nfreq) return fail(h, SG_ERR_ARG, "sg_get_spectrum: frequency outside 0 .. nfreq - 1");
  if (part < 0 || part > 1) return fail(h, SG_ERR_ARG, "sg_get_spectrum: part is 0 (re) or 1 (im)");
  const int f = field == 0 ? SG_FIELD_U : SG_FIELD_S;
  if (!host || nbytes != h->field_len[f] * sizeof(double)) return fail(h, SG_ERR_ARG, "sg_get_spectrum: size mismatch");
  HIPCHECK(h, hipSetDevice(h->cfg.device));
  return download_layout(h, f, sp.acc[field].get() + (size_t)(2 * freq + part) * h->field_alloc[f], host);
}

int sg_spectra_samples(sg_handle* h, int64_t* taken) {
  if (!h || !taken) return SG_ERR_ARG;
  *taken = h->spc.nfreq > 0 ? h->spc.clock.capped_samples() : 0;   // the spectra run out: no more than nsamples
  return SG_OK;
}

// By bilinearity up to four launches of sg_correlate's kernel, double instantiation, on the accumulators of the two handles.
int sg_correlate_spectra(sg_handle* a, int fa, sg_handle* b, int fb, const double w[3], const double z[2]) {
  if (!a) return SG_ERR_ARG;
  if (!b) return fail(a, SG_ERR_ARG, "sg_correlate_spectra: no second handle");
  if (b != a) {
    const std::string diff = xcorr_first_difference(a->cfg, (int)a->md.gw, b->cfg, (int)b->md.gw);
    if (!diff.empty()) return fail(a, SG_ERR_ARG, "sg_correlate_spectra: the handles differ in " + diff);
  }
  double wk[3];
  for (int k = 0; k < 3; ++k) wk[k] = w ? w[k] : 1.0;
  const bool need_u = wk[0] != 0.0, need_s = wk[1] != 0.0 || wk[2] != 0.0;
  for (const sg_handle* x : {(const sg_handle*)a, (const sg_handle*)b}) {
    if (x->spc.nfreq == 0) return fail(a, SG_ERR_STATE, "sg_correlate_spectra: a handle has no spectra armed (sg_set_spectra)");
    if ((need_u && !x->spc.has(0)) || (need_s && !x->spc.has(1)))
      return fail(a, SG_ERR_STATE, "sg_correlate_spectra: a weight asks for a field whose spectra a handle has not armed");
  }
  if (fa < 0 || fa >= a->spc.nfreq || fb < 0 || fb >= b->spc.nfreq)
    return fail(a, SG_ERR_ARG, "sg_correlate_spectra: frequency outside 0 .. nfreq - 1");
  if (!need_u && !need_s) return SG_OK;
  HIPCHECK(a, hipSetDevice(a->cfg.device));
  CorrelationTables fresh;
  if (!a->cor.ready)
    if (int rc = correlation_prepare(a, fresh)) return rc;
  CorrelationTables& ct = a->cor.ready ? a->cor : fresh;
  if (ct.grid64 == 0) {   // the double instantiation: the handle's own unless the block is FP32
    ct.grid64 = a->f32 ? prepare_xcorr(a->re.nd, (int)a->md.gw, ct.ipw, ct.mfma ? 1 : 0, 0, a->ncu) : ct.grid;
    if (ct.grid64 <= 0) {
      ct.grid64 = 0;
      return fail(a, SG_ERR_DEVICE, "sg_correlate_spectra: no kernel for this element");
    }
  }
  const int dim = a->cfg.dim;
  xcorr::Args x;
  std::memset(&x, 0, sizeof(x));
  x.M = ct.M.get();
  x.acc = ct.acc.get();
  double detj = 1.0;
  for (int k = 0; k < dim; ++k) detj *= a->cfg.h[k];
  x.nitems = ct.nitems;
  x.ncube = a->md.ncube;
  x.nd = a->re.nd;
  x.dim = dim;
  x.gw = (int32_t)a->md.gw;
  x.ncls = a->ncls;
  x.ipw = ct.ipw;
  // the kernel reads the velocity's components and then the listed ones of the stress: a stress no weight asks for is not
  // listed, a velocity no weight asks for is read from a's and b's own buffers of something finite - the stress accumulators,
  // which are longer - and its form enters with the weight 0
  const std::vector<XcorrComp> comps = xcorr_components(dim, a->sym, b->sym);
  x.ncomp = need_s ? (int32_t)comps.size() : dim;
  for (int k = 0; k < x.ncomp; ++k) {
    x.comp_a[k] = comps[k].comp_a;
    x.comp_b[k] = comps[k].comp_b;
    x.diag[k] = comps[k].diag ? 1 : 0;
    x.mult[k] = comps[k].mult;
  }
  const size_t nu = a->field_alloc[SG_FIELD_U], ns = a->field_alloc[SG_FIELD_S];
  auto part_of = [&](const sg_handle* h, int freq, int part, const void*& u, const void*& s) {
    const double* su = h->spc.has(1) ? h->spc.acc[1].get() + (size_t)(2 * freq + part) * ns : nullptr;
    s = su;
    u = h->spc.has(0) ? h->spc.acc[0].get() + (size_t)(2 * freq + part) * nu : su;
  };
  // behind everything both handles have queued; b's later work behind the launches
  if (int rc = join_second(a)) return rc;
  if (b != a) {
    if (join_second(b) != SG_OK) return fail(a, SG_ERR_DEVICE, std::string("sg_correlate_spectra: second handle: ") + b->err);
    HIPCHECK(a, hipEventRecord(ct.ev_in.get(), b->stream));
    HIPCHECK(a, hipStreamWaitEvent(a->stream, ct.ev_in.get(), 0));
  }
  const double zr = z ? z[0] : 1.0, zi = z ? z[1] : 0.0;
  const struct {
    int pa, pb;
    double zw;
  } terms[4] = {{0, 0, zr}, {1, 1, zr}, {0, 1, -zi}, {1, 0, zi}};
  for (int t = 0; t < (zi != 0.0 ? 4 : 2); ++t) {
    part_of(a, fa, terms[t].pa, x.ua, x.sa);
    part_of(b, fb, terms[t].pb, x.ub, x.sb);
    for (int k = 0; k < 3; ++k) x.wd[k] = terms[t].zw * wk[k] * detj;
    if (launch_xcorr(x, ct.mfma ? 1 : 0, 0, ct.grid64, a->stream) != 0) return fail(a, SG_ERR_DEVICE, "correlation launch failed");
  }
  if (b != a) {
    HIPCHECK(a, hipEventRecord(ct.ev_out.get(), a->stream));
    HIPCHECK(a, hipStreamWaitEvent(b->stream, ct.ev_out.get(), 0));
  }
  if (!a->cor.ready) a->cor = std::move(fresh);
  return SG_OK;
}

int sg_get_sym(const sg_handle* h, int* sym) {
  if (!h || !sym) return SG_ERR_ARG;
  *sym = h->sym ? 1 : 0;
  return SG_OK;
}

int sg_leave_sym(sg_handle* h) {
  if (!h) return SG_ERR_ARG;
  HIPCHECK(h, hipSetDevice(h->cfg.device));
  return leave_sym_mode(h);
}

int sg_halo_attach(sg_handle* h, int field, int side, const void* dev_in) {
  if (!h || field < 0 || field > 3 || side < 0 || side >= 2 * h->cfg.dim) return SG_ERR_ARG;
  h->ghost[field][side] = (const double*)dev_in;
  return SG_OK;
}

}  // extern "C"

// what every sample of the handle needs (handle.hpp MeasureScratch): built once, outside any capture
int measure_prepare(sg_handle* h) {
  if (h->msr.ready) return SG_OK;
  MeasureScratch ms;
  const int gw = (int)h->md.gw, nd = h->re.nd;
  ms.nitems = (h->md.ncube_pad / gw) * h->ncls;
  ms.nchunks = (ms.nitems + SG_MONITOR_CHUNK_ITEMS - 1) / SG_MONITOR_CHUNK_ITEMS;
  ms.ips = measure_items_per_sweep(nd, gw);
  if (ms.ips <= 0 || prepare_measure(nd, gw, ms.ips, h->f32) != 0) return fail(h, SG_ERR_DEVICE, "monitor: no kernel for this element");
  const std::vector<double> tri = mass_lower_rows(h->re.Mhat, nd);
  HIPCHECK(h, ms.Mtri.upload(tri.data(), tri.size()));
  if (ms.partial.alloc((size_t)ms.nchunks * 5) != hipSuccess || ms.out.alloc(5) != hipSuccess)
    return fail(h, SG_ERR_NOMEM, "monitor: hipMalloc of the partial sums failed");
  ms.ready = true;
  h->msr = std::move(ms);
  return SG_OK;
}
