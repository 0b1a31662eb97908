// The device-free part of the C-ABI (include/seigen_hip.h "device-free setup queries") and the host logic behind
// sg_create that involves no device: kernel-family choice, regions of a split stage and their items, node coordinates,
// point location, the receiver and the injector plan, the exports of the reference-element operators and mesh tables.  No HIP header,
// no HIP call: this file, refelem.cpp, mesh_tables.cpp, mfma_tables.cpp, sponge_tables.cpp and source_tables.cpp are what
// `make host-asan` builds with -fsanitize=address,undefined and runs on the CPU.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <stdexcept>

#include "hostlogic.hpp"
#include "kernels.hpp"
#include "mfma_tables.hpp"

using namespace sg;

std::string g_create_err;

// which (dim, degree) each kernel family is instantiated for (kernels_mfma.hip, kernels_lane.hip, kernels_tile2d.hip,
// kernels_hexm.hip)
static bool mfma_supported(int dim, int P) { return dim == 3 && P >= 1 && P <= 4; }
// 3-D: only P1/P2 fit a lane's registers (P3/P4 take the MFMA path)
static bool lane_supported(int dim, int P) { return ((dim == 1 || dim == 2) && P >= 1 && P <= 4) || (dim == 3 && (P == 1 || P == 2)); }
// hexahedra: DQ_1 and DQ_2 (27 nodes) fit a lane's registers one component at a time
static bool lane_supported_hex(int dim, int P) { return dim == 3 && (P == 1 || P == 2); }
static bool hexm_supported(int dim, int P) { return dim == 3 && (P == 3 || P == 4); }
static bool tile2d_supported(int dim, int P) { return dim == 2 && P >= 1 && P <= 4; }   // DQ_4 has 25 rows: two row tiles

// SEIGEN_HIP_PATH=generic: the generic kernels everywhere; =lane / =mfma / =tile: that family below its size threshold
// where it exists (an unknown value: as unset)
Family choose_kernel_path(const sg_config& cfg) {
  const char* pe = std::getenv("SEIGEN_HIP_PATH");
  const std::string path = pe ? pe : "";
  if (path == "generic") return Family::Generic;
  const bool force_lane = path == "lane";
  const int d = cfg.dim, P = cfg.degree;
  const int64_t ncube = (int64_t)cfg.n[0] * (d > 1 ? cfg.n[1] : 1) * (d > 2 ? cfg.n[2] : 1);
  if (cfg.diagonal == SG_DIAGONAL_QUAD) {
    // quadrilaterals: the MFMA tile kernels (DQ_4: two 16-row tiles) at every size, SEIGEN_HIP_PATH=lane included
    if (tile2d_supported(d, P)) return Family::Tile2d;
    // hexahedra DQ_3 / DQ_4: lines in registers, x lines on the matrix pipe (kernels_hexm.hip) at every size
    if (hexm_supported(d, P)) return Family::Hexm;
    // hexahedra DQ_1 / DQ_2: the sum-factorised lane-per-cell kernels (kernels_lane.hip hex_stage) from
    // SG_HEX_LANE_MIN_CELLS(degree) cubes up (below that the thread-per-node generic kernel has more parallelism)
    if (lane_supported_hex(d, P) && (force_lane || ncube >= SG_HEX_LANE_MIN_CELLS(P))) return Family::Lane;
    return Family::Generic;
  }
  const int64_t ncells = ncube * (d == 1 ? 1 : (d == 2 ? 2 : 6));
  // 3-D: the MFMA kernels at every degree (degrees 1 and 2 use 4x4x4 tiles only); measured with tools/path_sweep.py they
  // beat the lane and generic kernels everywhere except degree 1 on blocks under 65536 cells
  if (mfma_supported(d, P) && !force_lane && (P >= 2 || ncells >= 65536 || path == "mfma")) return Family::Mfma;
  // 2-D: the MFMA tile kernels (16 cells per wave, operators in registers) at every size: they win at every size measured,
  // 40 x 40 squares included (tools/path_sweep2d.py, profiles/r02/path_sweep2d_tile_v2.txt)
  if (tile2d_supported(d, P) && !force_lane) return Family::Tile2d;
  // lane-per-cell kernels need enough 64-cell groups to fill the chip; below that the thread-per-node generic kernel has
  // more parallelism (crossovers measured: tools/path_sweep.py, profiles/r02/small_2d_configs_negative_results.txt)
  if (lane_supported(d, P) && (force_lane || ncells >= (P == 1 ? 196608 : 120000))) return Family::Lane;
  return Family::Generic;
}

StageOp lf4_stage(int stage, double dt, double rho, bool rho_physical, bool per_cell_density) {
  const double c3 = dt * dt * dt / 24.0;
  const int U = SG_FIELD_U, UH = SG_FIELD_UH, S = SG_FIELD_S, SH = SG_FIELD_SH;
  switch (stage) {   // {kind, in, out, aux, uabs, mode, c_self, c_aux, c_new, with_source, src_coef, density}
    case SG_STAGE_UH1: return {0, S, UH};
    case SG_STAGE_STEMP: return {1, UH, SH, -1, U, 0, 0.0, 0.0, 0.0, true, 1.0, false};
    case SG_STAGE_U1:
      // explicit mode keeps only rhs(form_u1): u1 = rho*u0 + dt*uh1 + dt^3/24*uh2 (elastic.py:341-345, :354-356);
      // sg_set_density(physical = 1): u1 = u0 + (dt*uh1 + dt^3/24*uh2)/rho; per-cell density: factors in rho2
      if (per_cell_density) return {0, SH, U, UH, U, 1, 1.0, dt, c3, false, 1.0, true};
      if (rho_physical) return {0, SH, U, UH, U, 1, 1.0, dt / rho, c3 / rho, false, 1.0, false};
      return {0, SH, U, UH, U, 1, rho, dt, c3, false, 1.0, false};
    case SG_STAGE_SH1: return {1, U, SH, -1, U, 0, 0.0, 0.0, 0.0, true, 1.0, false};
    case SG_STAGE_UTEMP:
      // utemp = F(sh1; u1) has one consumer, sh2 = G(utemp) in the stress update s1 = s0 + dt sh1 + dt^3/24 sh2 with
      // sh1 = G(u1) + S (elastic.py:300-303, :348-352) - and g is LINEAR in the velocity: dt G(u1) + dt^3/24 G(utemp) =
      // G(dt u1 + dt^3/24 utemp).  So this stage leaves w = dt u1 + dt^3/24 utemp in UH (one more operand in its fused
      // epilogue, on a stage that waits for the matrix pipe, not for memory) and stage S1 reads w and s0 ONLY: no sh1, no
      // second right-hand side - 6 of its 21 words per node gone (the halo exchanged after this stage is w's).
      // (mode 2: the fused form without the self term, out = c_aux aux + c_new rhs; kernel families without an instantiation
      // of their own run their mode-1 kernels with c_self = 0)
      return {0, SH, UH, U, U, 2, 0.0, dt, c3, false, 1.0, false};
    case SG_STAGE_S1:
      // s1 = s0 + G(w) + (dt + dt^3/24) S   (G stage kernels, fused form: out = c_self out + c_new rhs, no second operand)
      return {1, UH, S, -1, U, 1, 1.0, 0.0, 1.0, true, dt + c3, false};
  }
  return {};
}

void region_boxes(int d, const int32_t n[3], const int32_t has_nbr[6], int region, std::vector<Box>& out, int xw) {
  out.clear();
  int lo[3] = {0, 0, 0}, hi[3];
  for (int a = 0; a < 3; ++a) hi[a] = n[a];
  if (region == SG_REGION_ALL) {
    out.push_back(Box{{0, 0, 0}, {hi[0], hi[1], hi[2]}});
    return;
  }
  // interior: peel one cube (along x: one layout group of xw cubes, handle.hpp shell_width_x) off every side
  // that has a neighbour block
  int ilo[3] = {0, 0, 0}, ihi[3] = {hi[0], hi[1], hi[2]};
  for (int a = 0; a < d; ++a) {
    const int w = (a == 0 && xw > 1) ? xw : 1;
    if (has_nbr[2 * a]) ilo[a] = w < hi[a] ? w : hi[a];
    if (has_nbr[2 * a + 1]) ihi[a] = hi[a] - w > 0 ? hi[a] - w : 0;
    if (ihi[a] < ilo[a]) ihi[a] = ilo[a];
  }
  if (region == SG_REGION_INTERIOR) {
    out.push_back(Box{{ilo[0], ilo[1], ilo[2]}, {ihi[0] - ilo[0], ihi[1] - ilo[1], ihi[2] - ilo[2]}});
    return;
  }
  // FIRST / SECOND: the interior cut in two along the slowest axis (whole runs of the layout)
  const int ax = d - 1, mid = ilo[ax] + (ihi[ax] - ilo[ax]) / 2;
  if (region == SG_REGION_SECOND) {
    Box b{{ilo[0], ilo[1], ilo[2]}, {ihi[0] - ilo[0], ihi[1] - ilo[1], ihi[2] - ilo[2]}};
    b.o[ax] = mid;
    b.n[ax] = ihi[ax] - mid;
    out.push_back(b);
    return;
  }
  if (region == SG_REGION_FIRST) {
    Box b{{ilo[0], ilo[1], ilo[2]}, {ihi[0] - ilo[0], ihi[1] - ilo[1], ihi[2] - ilo[2]}};
    b.n[ax] = mid - ilo[ax];
    out.push_back(b);
  }
  // boundary shell = all \ interior, as disjoint slabs: peel axis by axis
  int clo[3] = {lo[0], lo[1], lo[2]}, chi[3] = {hi[0], hi[1], hi[2]};
  for (int a = 0; a < d; ++a) {
    if (ilo[a] > clo[a]) {
      Box b;
      for (int k = 0; k < 3; ++k) {
        b.o[k] = clo[k];
        b.n[k] = chi[k] - clo[k];
      }
      b.n[a] = ilo[a] - clo[a];
      out.push_back(b);
      clo[a] = ilo[a];
    }
    if (ihi[a] < chi[a] && ihi[a] >= clo[a]) {
      Box b;
      for (int k = 0; k < 3; ++k) {
        b.o[k] = clo[k];
        b.n[k] = chi[k] - clo[k];
      }
      b.o[a] = ihi[a];
      b.n[a] = chi[a] - ihi[a];
      out.push_back(b);
      chi[a] = ihi[a];
    }
  }
}

RegionItems region_items(const std::vector<Box>& boxes, const int32_t n[3], const Layout& L, int64_t ncube, int64_t ncube_pad) {
  const int64_t ngroups = L.group(ncube_pad);
  std::vector<int32_t> cnt((size_t)ngroups, 0);
  for (const Box& b : boxes)
    for (int ck = b.o[2]; ck < b.o[2] + b.n[2]; ++ck)
      for (int cj = b.o[1]; cj < b.o[1] + b.n[1]; ++cj)
        for (int ci = b.o[0]; ci < b.o[0] + b.n[0]; ++ci) cnt[(size_t)L.group(ci + (int64_t)n[0] * (cj + (int64_t)n[1] * ck))] += 1;
  // Whole groups only (always, on meshes whose rows are a multiple of the group width: a shell in x is one
  // group thick): the kernels then skip the cube coordinates and the box tests, as in a whole-block launch.
  // (The boxes of a region are disjoint, so the count of a group tells.)
  RegionItems r;
  for (int64_t g = 0; g < ngroups; ++g) {
    if (cnt[(size_t)g] == 0) continue;
    if (cnt[(size_t)g] != std::min<int64_t>(L.gw, ncube - g * L.gw)) r.whole = false;
    for (int64_t k = 0; k < L.ncls; ++k) r.items.push_back((int32_t)(g * L.ncls + k));
  }
  return r;
}

// J xi = r for a dim x dim system, Gaussian elimination with partial pivoting (what np.linalg.solve does in
// functionspace.py locate); false if J is singular
static bool solve_small(int d, double J[3][3], double r[3], double xi[3]) {
  for (int j = 0; j < d; ++j) {
    int pv = j;
    for (int i = j + 1; i < d; ++i)
      if (std::fabs(J[i][j]) > std::fabs(J[pv][j])) pv = i;
    if (J[pv][j] == 0.0) return false;
    if (pv != j) {
      for (int k = 0; k < d; ++k) std::swap(J[j][k], J[pv][k]);
      std::swap(r[j], r[pv]);
    }
    for (int i = j + 1; i < d; ++i) {
      const double l = J[i][j] / J[j][j];
      for (int k = j; k < d; ++k) J[i][k] -= l * J[j][k];
      r[i] -= l * r[j];
    }
  }
  for (int i = d - 1; i >= 0; --i) {
    double v = r[i];
    for (int k = i + 1; k < d; ++k) v -= J[i][k] * xi[k];
    xi[i] = v / J[i][i];
  }
  return true;
}

int64_t locate_point(const NodeGeom& G, const double* p, double* xi) {
  const sg_config& cfg = *G.cfg;
  const int d = G.d;
  // the cell's vertices are lattice corners: node 0 and the nodes P steps along each reference axis
  int corner[4] = {0, 0, 0, 0};
  for (int v = 0; v <= d; ++v)
    for (int a = 0; a < G.nq; ++a) {
      bool hit = true;
      for (int m = 0; m < d; ++m) hit = hit && G.lat[(size_t)a * d + m] == (m == v - 1 ? G.degree : 0);
      if (hit) {
        corner[v] = a;
        break;
      }
    }
  int64_t opt[3][2] = {{0, 0}, {0, 0}, {0, 0}};
  int nopt[3] = {1, 1, 1};
  for (int a = 0; a < d; ++a) {
    const double t = (p[a] - cfg.origin[a]) / cfg.h[a];
    if (!(std::fabs(t) < 1e15)) return -1;     // NaN, or far outside any mesh
    const int64_t i = (int64_t)std::floor(t);
    nopt[a] = 0;
    if (std::fabs(t - std::nearbyint(t)) < 1e-9 && i - 1 >= 0) opt[a][nopt[a]++] = i - 1;
    if (i >= 0) opt[a][nopt[a]++] = i;
    if (nopt[a] == 0) return -1;
  }
  for (int oz = 0; oz < nopt[2]; ++oz)
    for (int oy = 0; oy < nopt[1]; ++oy)
      for (int ox = 0; ox < nopt[0]; ++ox) {
        const int64_t g[3] = {opt[0][ox], opt[1][oy], opt[2][oz]};
        // block-local cube (NodeGeom adds cube0 back first: the same coordinates on every block)
        int c[3] = {0, 0, 0};
        bool mine = true;
        for (int a = 0; a < d; ++a) {
          const int64_t l = g[a] - cfg.cube0[a];
          // the candidates of an axis are at most one apart: none of them lies in this block
          if (l < -1 || l > cfg.n[a]) return -1;
          c[a] = (int)l;
          mine = mine && l >= 0 && l < cfg.n[a];
        }
        for (int k = 0; k < G.ncls; ++k) {
          double V[4][3];
          for (int v = 0; v <= d; ++v) G.node(c, k, corner[v], V[v]);
          double J[3][3], r[3], x[3] = {0, 0, 0};
          for (int i = 0; i < d; ++i) {
            for (int m = 0; m < d; ++m) J[i][m] = V[m + 1][i] - V[0][i];
            r[i] = p[i] - V[0][i];
          }
          if (!solve_small(d, J, r, x)) continue;
          double lo = x[0], hi = x[0], sum = x[0];
          for (int m = 1; m < d; ++m) {
            lo = std::min(lo, x[m]);
            hi = std::max(hi, x[m]);
            sum += x[m];
          }
          const double top = cfg.diagonal == SG_DIAGONAL_QUAD ? hi : sum;
          if (!(lo >= -1e-12 && top <= 1.0 + 1e-12)) continue;
          if (!mine) return -1;     // the winner lies in a neighbouring block
          for (int m = 0; m < d; ++m) xi[m] = x[m];
          const int64_t cube = c[0] + (int64_t)cfg.n[0] * ((d > 1 ? c[1] : 0) + (int64_t)(d > 1 ? cfg.n[1] : 1) * (d > 2 ? c[2] : 0));
          return cube * G.ncls + k;
        }
      }
  return -1;
}

ReceiverPlan plan_receivers(const NodeGeom& G, const Layout& L, int kind, int64_t nrec, const double* pts, int what, int64_t capacity) {
  const int d = G.d;
  ReceiverPlan pl;
  pl.own.assign((size_t)nrec, 0);
  pl.ncomp = ((what & 1) ? d : 0) + ((what & 2) ? d * d : 0);
  for (int64_t k = 0; k < nrec; ++k) {
    double xi[3] = {0, 0, 0};
    const int64_t cell = locate_point(G, pts + k * d, xi);
    if (cell < 0) continue;
    const int64_t cube = cell / L.ncls, cls = cell % L.ncls;
    pl.own[(size_t)k] = 1;
    pl.row.push_back(k);
    pl.item.push_back(L.item(cube, cls));
    pl.lane.push_back((int32_t)L.lane(cube));
    pl.phi.resize(pl.phi.size() + (size_t)L.nd);
    tabulate(d, G.degree, 1, xi, pl.phi.data() + pl.phi.size() - L.nd, kind);
  }
  const int64_t nown = (int64_t)pl.row.size();
  if (nown > 0 && capacity > ((int64_t)1 << 40) / (nown * pl.ncomp)) throw std::invalid_argument("capacity too large");
  return pl;
}

void gauge_weights(int dim, int degree, int cell_kind, int nd, const double* xi, double* D) {
  std::vector<double> dphi((size_t)nd * dim);
  tabulate_grad(dim, degree, 1, xi, dphi.data(), cell_kind);
  for (int r = 0; r < dim; ++r)
    for (int a = 0; a < nd; ++a) D[(size_t)r * nd + a] = dphi[(size_t)a * dim + r];
}

GaugePlan plan_gauges(const NodeGeom& G, const Layout& L, int cell_kind, int64_t npts, const double* pts, int kind, int64_t capacity) {
  const int d = G.d;
  GaugePlan pl;
  pl.own.assign((size_t)npts, 0);
  pl.ncomp = grad_ncomp(d, kind);
  const size_t per = (size_t)d * (size_t)L.nd;
  for (int64_t k = 0; k < npts; ++k) {
    double xi[3] = {0, 0, 0};
    const int64_t cell = locate_point(G, pts + k * d, xi);
    if (cell < 0) continue;
    const int64_t cube = cell / L.ncls, cls = cell % L.ncls;
    pl.own[(size_t)k] = 1;
    pl.row.push_back(k);
    pl.item.push_back(L.item(cube, cls));
    pl.lane.push_back((int32_t)L.lane(cube));
    pl.cls.push_back((int32_t)cls);
    pl.D.resize(pl.D.size() + per);
    gauge_weights(d, G.degree, cell_kind, (int)L.nd, xi, pl.D.data() + pl.D.size() - per);
  }
  const int64_t nown = (int64_t)pl.row.size();
  if (nown > 0 && pl.ncomp > 0 && capacity > ((int64_t)1 << 40) / (nown * pl.ncomp)) throw std::invalid_argument("capacity too large");
  return pl;
}

void injector_weights(const RefElem& re, int degree, double detj, const double* xi, double* psi) {
  std::vector<double> phi((size_t)re.nd);
  tabulate(re.dim, degree, 1, xi, phi.data(), re.kind);
  for (int a = 0; a < re.nd; ++a) {
    double v = 0.0;
    for (int b = 0; b < re.nd; ++b) v = std::fma(re.Minv[(size_t)a * re.nd + b], phi[(size_t)b], v);
    psi[a] = v / detj;
  }
}

InjectorPlan injector_plan(const NodeGeom& G, const Layout& L, const RefElem& re, int64_t npts, const double* pts, int what) {
  const int d = G.d;
  InjectorPlan pl;
  pl.own.assign((size_t)npts, 0);
  pl.ncomp = ((what & 1) ? d : 0) + ((what & 2) ? d * d : 0);
  double detj = 1.0;
  for (int a = 0; a < d; ++a) detj *= G.cfg->h[a];
  std::vector<int64_t> cell_of((size_t)npts, -1);
  std::vector<double> xi((size_t)npts * 3, 0.0);
  for (int64_t k = 0; k < npts; ++k) {
    cell_of[(size_t)k] = locate_point(G, pts + k * d, &xi[(size_t)k * 3]);
    if (cell_of[(size_t)k] < 0) continue;
    pl.own[(size_t)k] = 1;
    pl.row.push_back(k);
  }
  std::stable_sort(pl.row.begin(), pl.row.end(), [&](int64_t x, int64_t y) { return cell_of[(size_t)x] < cell_of[(size_t)y]; });
  pl.psi.resize(pl.row.size() * (size_t)L.nd);
  for (size_t r = 0; r < pl.row.size(); ++r) {
    const int64_t k = pl.row[r], cell = cell_of[(size_t)k];
    if (pl.cell.empty() || pl.cell.back() != cell) {
      const int64_t cube = cell / L.ncls, cls = cell % L.ncls;
      pl.cell.push_back(cell);
      pl.item.push_back(L.item(cube, cls));
      pl.lane.push_back((int32_t)L.lane(cube));
      pl.start.push_back((int64_t)r);
    }
    injector_weights(re, G.degree, detj, &xi[(size_t)k * 3], &pl.psi[r * (size_t)L.nd]);
  }
  pl.start.push_back((int64_t)pl.row.size());
  return pl;
}

std::vector<double> injector_gather(const InjectorPlan& pl, int64_t npts, int64_t nsteps, const double* amp) {
  const size_t nown = pl.row.size(), nc = (size_t)pl.ncomp;
  std::vector<double> out((size_t)nsteps * nown * nc);
  for (int64_t k = 0; k < nsteps; ++k)
    for (size_t r = 0; r < nown; ++r)
      std::memcpy(&out[((size_t)k * nown + r) * nc], amp + ((size_t)k * (size_t)npts + (size_t)pl.row[r]) * nc, nc * sizeof(double));
  return out;
}

bool injector_symmetric(const InjectorPlan& pl, int dim, int what, int64_t nsteps, const std::vector<double>& gathered) {
  if (!(what & 2)) return true;
  const size_t nown = pl.row.size(), nc = (size_t)pl.ncomp, off = (what & 1) ? (size_t)dim : 0;
  for (size_t e = 0; e < (size_t)nsteps * nown; ++e)
    for (int i = 0; i < dim; ++i)
      for (int j = i + 1; j < dim; ++j)
        if (std::memcmp(&gathered[e * nc + off + (size_t)(i * dim + j)], &gathered[e * nc + off + (size_t)(j * dim + i)], sizeof(double)) != 0)
          return false;
  return true;
}

FramePlan frame_plan(const sg_config& cfg, int gw, int ncls, const sg_frame& fr) {
  FramePlan p;
  const int d = cfg.dim;
  p.dim = d;
  p.gw = gw;
  p.ncls = ncls;
  int nfree = 0;
  p.owns = true;
  for (int a = 0; a < d; ++a) {
    if (fr.fixed[a] != 0 && fr.fixed[a] != 1) return p.err = "sg_frame: fixed[a] is 0 or 1", p;
    p.fixed[a] = fr.fixed[a];
    if (!fr.fixed[a]) {
      if (fr.m[a] < 1 || fr.m[a] > FRAME_MAX_M) return p.err = "sg_frame: m[a] outside 1 .. 8", p;
      p.m[a] = fr.m[a];
      p.P[a] = (int64_t)cfg.n[a] * fr.m[a];
      p.Q *= fr.m[a];
      nfree += 1;
      continue;
    }
    // the candidates of locate_point for this axis, in its order; the first whose fraction passes its tests wins
    const double t = (fr.at[a] - cfg.origin[a]) / cfg.h[a];
    if (!(std::fabs(t) < 1e15)) return p.err = "sg_frame: at[a] is not a coordinate", p;
    const int64_t i = (int64_t)std::floor(t);
    int64_t cand[2];
    int nc = 0;
    if (std::fabs(t - std::nearbyint(t)) < 1e-9 && i - 1 >= 0) cand[nc++] = i - 1;
    if (i >= 0) cand[nc++] = i;
    int64_t g = -1;
    for (int k = 0; k < nc && g < 0; ++k) {
      const double tf = t - (double)cand[k];
      if (tf >= -1e-12 && tf <= 1.0 + 1e-12) g = cand[k];
    }
    if (g >= 0) p.t_fixed[a] = t - (double)g;   // (the fraction belongs to the mesh's layer, whichever block holds it)
    const int64_t l = g - cfg.cube0[a];
    if (g < 0 || l < 0 || l >= cfg.n[a]) {
      p.owns = false;
      continue;
    }
    p.layer[a] = (int32_t)l;
  }
  if (nfree == 0) return p.err = "sg_frame: no free axis", p;
  if (p.Q > FRAME_MAX_Q) return p.err = "sg_frame: more than 64 pixels in a cube", p;
  if (!p.owns) {
    for (int a = 0; a < 3; ++a) p.layer[a] = -1;
    return p;
  }
  // the groups that hold a cube of the layer: the cubes in ascending order, hence the groups too
  int lo[3] = {0, 0, 0}, hi[3] = {1, 1, 1};
  for (int a = 0; a < d; ++a) {
    lo[a] = p.fixed[a] ? p.layer[a] : 0;
    hi[a] = p.fixed[a] ? p.layer[a] + 1 : cfg.n[a];
  }
  const int64_t n0 = cfg.n[0], n1 = d > 1 ? cfg.n[1] : 1;
  int64_t ncubes = 0;
  for (int c2 = lo[2]; c2 < hi[2]; ++c2)
    for (int c1 = lo[1]; c1 < hi[1]; ++c1)
      for (int c0 = lo[0]; c0 < hi[0]; ++c0) {
        const int64_t group = (c0 + n0 * (c1 + n1 * c2)) / gw;
        if (p.groups.empty() || p.groups.back() != (int32_t)group) p.groups.push_back((int32_t)group);
        ncubes += 1;
      }
  if (gw == 1) {
    p.units = ncubes * p.Q;
    p.grid = std::min((p.units + FRAME_THREADS - 1) / FRAME_THREADS, FRAME_GRID_CAP);
  } else {
    const int64_t per_wave = 64 / gw;
    p.units = (((int64_t)p.groups.size() + per_wave - 1) / per_wave) * ncls;
    p.grid = std::min((p.units + FRAME_THREADS / 64 - 1) / (FRAME_THREADS / 64), FRAME_GRID_CAP);
  }
  return p;
}

bool frame_weights(const sg_config& cfg, int degree, const FramePlan& p, int32_t* cls, double* xi, double* phi, std::string* err) {
  sg_config unit;
  std::memset(&unit, 0, sizeof(unit));
  unit.dim = cfg.dim;
  unit.degree = degree;
  unit.diagonal = cfg.diagonal;
  for (int a = 0; a < 3; ++a) {
    unit.n[a] = 1;
    unit.h[a] = 1.0;
  }
  NodeGeom G;
  if (!G.init(&unit, degree)) return *err = "sg_frame: no such element", false;
  const int d = cfg.dim;
  const int kind = cfg.diagonal == SG_DIAGONAL_QUAD ? KIND_TENSOR : KIND_SIMPLEX;
  const int nd = G.nq;
  for (int q = 0; q < p.Q; ++q) {
    double t[3] = {0, 0, 0}, x[3] = {0, 0, 0};
    for (int a = 0; a < d; ++a) t[a] = p.fraction(q, a);
    const int64_t cell = locate_point(G, t, x);
    if (cell < 0) return *err = "sg_frame: a pixel lies in no cell of its cube", false;
    cls[q] = (int32_t)cell;   // (one cube: the cell is the class)
    for (int a = 0; a < d; ++a) xi[(size_t)q * d + a] = x[a];
    tabulate(d, degree, 1, x, phi + (size_t)q * nd, kind);
  }
  return true;
}

// what the device-free frame exports check of a configuration, and the layout's group width and classes sg_create would choose
static bool frame_config(const sg_config* cfg, const sg_frame* fr, int* gw, int* ncls) {
  if (!cfg || !fr || cfg->dim < 1 || cfg->dim > 3) return false;
  for (int a = 0; a < cfg->dim; ++a)
    if (cfg->n[a] < 1 || !(cfg->h[a] > 0.0)) return false;
  const bool quad = cfg->diagonal == SG_DIAGONAL_QUAD;
  if (quad && cfg->dim == 1) return false;
  *gw = family_gw(choose_kernel_path(*cfg));
  *ncls = quad ? 1 : (cfg->dim == 1 ? 1 : (cfg->dim == 2 ? 2 : 6));
  return true;
}

extern "C" {

int sg_abi_version(void) { return SG_ABI_VERSION; }

int sg_frame_plan(const sg_config* cfg, const sg_frame* fr, int64_t out[12]) {
  int gw = 1, ncls = 1;
  if (!out || !frame_config(cfg, fr, &gw, &ncls)) return SG_ERR_ARG;
  const FramePlan p = frame_plan(*cfg, gw, ncls, *fr);
  if (!p.err.empty()) {
    g_create_err = p.err;
    return SG_ERR_ARG;
  }
  for (int a = 0; a < 3; ++a) {
    out[a] = p.P[a];
    out[5 + a] = p.layer[a];
  }
  out[3] = p.Q;
  out[4] = p.owns ? 1 : 0;
  out[8] = (int64_t)p.groups.size();
  out[9] = p.units;
  out[10] = p.grid;
  out[11] = gw;
  return SG_OK;
}

int64_t sg_frame_groups(const sg_config* cfg, const sg_frame* fr, int32_t* groups, int64_t max_groups) {
  int gw = 1, ncls = 1;
  if (!frame_config(cfg, fr, &gw, &ncls)) return SG_ERR_ARG;
  const FramePlan p = frame_plan(*cfg, gw, ncls, *fr);
  if (!p.err.empty()) {
    g_create_err = p.err;
    return SG_ERR_ARG;
  }
  if (groups) {
    if ((int64_t)p.groups.size() > max_groups) return SG_ERR_ARG;
    std::copy(p.groups.begin(), p.groups.end(), groups);
  }
  return (int64_t)p.groups.size();
}

int sg_frame_weights(const sg_config* cfg, int degree, const sg_frame* fr, int32_t* cls, double* xi, double* phi) {
  int gw = 1, ncls = 1;
  if (!cls || !xi || !phi || degree < 1 || degree > 8 || !frame_config(cfg, fr, &gw, &ncls)) return SG_ERR_ARG;
  const FramePlan p = frame_plan(*cfg, gw, ncls, *fr);
  if (!p.err.empty() || !frame_weights(*cfg, degree, p, cls, xi, phi, &g_create_err)) {
    if (!p.err.empty()) g_create_err = p.err;
    return SG_ERR_ARG;
  }
  return SG_OK;
}

int sg_spectra_clock(int64_t every, int64_t nsamples, int64_t steps, int64_t more, int64_t out[4]) {
  if (!out || every < 1 || nsamples < 0 || steps < 0 || more < 0) return SG_ERR_ARG;
  const StepClock c{every, nsamples, steps};
  out[0] = c.due_at(steps + 1) ? 1 : 0;
  out[1] = c.due_at(steps + 1) ? c.sample_at(steps + 1) : -1;
  out[2] = c.active() ? 1 : 0;
  out[3] = c.capped_samples_after(more);   // the spectra run out: no more than nsamples
  return SG_OK;
}

int sg_xfer_plan(int gw, int ncls, int nd, int ncomp, int dev_bytes, int caller_bytes, int64_t cell0, int64_t ncells, int64_t out[6]) {
  if (!out || (gw != 1 && gw != 16 && gw != 64) || ncls < 1 || nd < 1 || ncomp < 1 || cell0 < 0 || ncells < 0) return SG_ERR_ARG;
  if ((dev_bytes != 4 && dev_bytes != 8) || (caller_bytes != 4 && caller_bytes != 8)) return SG_ERR_ARG;
  const XferPlan p = xfer_plan(gw, ncls, nd, ncomp, dev_bytes, cell0, ncells);   // (the LDS image is in the block's type)
  out[0] = p.item0;
  out[1] = p.nitems;
  out[2] = p.rows_per_slice;
  out[3] = p.slices;
  out[4] = p.grid;
  out[5] = p.lds_bytes;
  return SG_OK;
}

int sg_gradient_plan(int gw, int ncls, int nd, int dim, int ncomp, int dev_bytes, int caller_bytes, int64_t cell0, int64_t ncells,
                     int64_t out[6]) {
  if (!out || (gw != 1 && gw != 16 && gw != 64) || ncls < 1 || nd < 1 || dim < 1 || dim > 3 || ncomp < 1 || ncomp > dim * dim) return SG_ERR_ARG;
  if (cell0 < 0 || ncells < 0 || (dev_bytes != 4 && dev_bytes != 8) || (caller_bytes != 4 && caller_bytes != 8)) return SG_ERR_ARG;
  const GradPlan p = grad_plan(gw, ncls, nd, dim, ncomp, cell0, ncells);
  if (!p.ok) {
    g_create_err = "sg_gradient_plan: the item's velocity block leaves no room for a node's values in the LDS budget";
    return SG_ERR_ARG;
  }
  out[0] = p.item0;
  out[1] = p.nitems;
  out[2] = p.nodes_per_slice;
  out[3] = p.slices;
  out[4] = p.grid;
  out[5] = p.lds_bytes;
  return SG_OK;
}

int sg_tabulate_grad_cell(int cell_type, int dim, int degree, int64_t npts, const double* xi, double* dphi) {
  if (dim < 1 || dim > 3 || degree < 1 || degree > 8 || npts < 0 || !xi || !dphi) return SG_ERR_ARG;
  if (cell_type != KIND_SIMPLEX && cell_type != KIND_TENSOR) return SG_ERR_ARG;
  tabulate_grad(dim, degree, (int)npts, xi, dphi, cell_type);
  return SG_OK;
}

int64_t sg_gradient_tables(const sg_config* cfg, double* C, double* J) {
  if (!cfg || cfg->dim < 1 || cfg->dim > 3 || cfg->degree < 1 || cfg->degree > 4) return SG_ERR_ARG;
  const bool quad = cfg->diagonal == SG_DIAGONAL_QUAD;
  if (quad && cfg->dim == 1) return SG_ERR_ARG;
  for (int a = 0; a < cfg->dim; ++a)
    if (!(cfg->h[a] > 0.0)) return SG_ERR_ARG;
  try {
    const RefElem re = make_refelem(cfg->dim, cfg->degree, quad ? KIND_TENSOR : KIND_SIMPLEX);
    const int64_t size = (int64_t)cfg->dim * re.nd * re.nd;
    if (C) {
      const std::vector<double> c = grad_dense_tables(re.kind, cfg->dim, cfg->degree, re.lattice);
      std::memcpy(C, c.data(), c.size() * sizeof(double));
    }
    if (J) {
      MeshDev md;
      std::memset(&md, 0, sizeof(md));
      md.nd = re.nd;
      md.nf = re.nf;
      double hh[3] = {1, 1, 1};
      for (int a = 0; a < cfg->dim; ++a) hh[a] = cfg->h[a];
      build_mesh_tables(cfg->dim, cfg->degree, cfg->diagonal, hh, re.fnode.data(), re.lattice.data(), md);
      for (int c = 0; c < md.ncls; ++c)
        for (int r = 0; r < 3; ++r)
          for (int j = 0; j < 3; ++j) J[((size_t)c * 3 + r) * 3 + j] = md.Jinv[c][r][j];
    }
    return size;
  } catch (const std::exception& e) {
    g_create_err = e.what();
    return SG_ERR_ARG;
  }
}

int64_t sg_mfma_class_frame(const sg_config* cfg, int32_t* p, double* s, double* cn, int32_t* lines, double* E, double* Ed) {
  if (!cfg || cfg->dim != 3 || cfg->degree < 1 || cfg->degree > 4 || cfg->diagonal == SG_DIAGONAL_QUAD) return SG_ERR_ARG;
  for (int a = 0; a < 3; ++a)
    if (!(cfg->h[a] > 0.0)) return SG_ERR_ARG;
  try {
    const RefElem re = make_refelem(3, cfg->degree, KIND_SIMPLEX);
    MeshDev md;
    std::memset(&md, 0, sizeof(md));
    md.nd = re.nd;
    md.nf = re.nf;
    build_mesh_tables(3, cfg->degree, cfg->diagonal, cfg->h, re.fnode.data(), re.lattice.data(), md);
    for (int k = 0; k < 6; ++k) {
      MfmaClassConst kc;
      std::memset(&kc, 0, sizeof(kc));
      mfma_trace_lines(md, k, kc);
      mfma_class_frame(md, k, kc);
      for (int m = 0; m < 3; ++m) {
        if (p) p[k * 3 + m] = kc.cf_p[m];
        if (s) s[k * 3 + m] = kc.cf_s[m];
      }
      for (int f = 0; f < 4 && cn; ++f)
        for (int c = 0; c < 2; ++c) cn[(k * 4 + f) * 2 + c] = kc.cf_cn[f][c];
      for (int sym = 0; sym < 2 && lines; ++sym) {
        int32_t* l = lines + (size_t)(k * 2 + sym) * 36;
        for (int c = 0; c < 9; ++c) l[c] = kc.cf_own[sym][c];
        for (int f = 0; f < 4; ++f)
          for (int c = 0; c < 6; ++c) l[9 + f * 6 + c] = kc.cf_tr[sym][f][c];
        for (int m = 0; m < 3; ++m) l[33 + m] = kc.cf_vel[m];
      }
    }
    for (int r = 0; r < 3; ++r)
      for (int a = 0; a < re.nd; ++a)
        for (int b = 0; b < re.nd; ++b) {
          if (E) E[((size_t)r * re.nd + a) * re.nd + b] = mfma_E(re, r, a, b);
          if (Ed) Ed[((size_t)r * re.nd + a) * re.nd + b] = mfma_Ediff(re, r, a, b);
        }
    return re.nd;
  } catch (const std::exception& e) {
    g_create_err = e.what();
    return SG_ERR_ARG;
  }
}

int sg_spectra_lines(int dim, int sym, int32_t* lines, int max_lines) {
  if (dim < 1 || dim > 3 || !lines) return SG_ERR_ARG;
  const std::vector<int32_t> r = spectra_lines(dim, sym != 0);
  if ((int)r.size() > max_lines) return SG_ERR_ARG;
  std::copy(r.begin(), r.end(), lines);
  return (int)r.size();
}

int sg_injector_weights(const sg_config* cfg, int64_t npts, const double* pts, int64_t* cell, double* psi) {
  if (!cfg || npts < 0 || (npts > 0 && (!pts || !cell || !psi))) return SG_ERR_ARG;
  if (cfg->dim < 1 || cfg->dim > 3 || cfg->degree < 1 || cfg->degree > 4) return SG_ERR_ARG;
  for (int a = 0; a < cfg->dim; ++a)
    if (cfg->n[a] < 1 || !(cfg->h[a] > 0.0)) return SG_ERR_ARG;
  NodeGeom G;
  if (!G.init(cfg, cfg->degree)) return SG_ERR_ARG;
  const int d = cfg->dim;
  try {
    const RefElem re = make_refelem(d, cfg->degree, cfg->diagonal == SG_DIAGONAL_QUAD ? KIND_TENSOR : KIND_SIMPLEX);
    double detj = 1.0;
    for (int a = 0; a < d; ++a) detj *= cfg->h[a];
    for (int64_t k = 0; k < npts; ++k) {
      double xi[3] = {0, 0, 0};
      cell[k] = locate_point(G, pts + k * d, xi);
      if (cell[k] >= 0)
        injector_weights(re, cfg->degree, detj, xi, psi + k * re.nd);
      else
        for (int a = 0; a < re.nd; ++a) psi[k * re.nd + a] = 0.0;
    }
  } catch (const std::exception& e) {
    g_create_err = e.what();
    return SG_ERR_ARG;
  }
  return SG_OK;
}

int64_t sg_gauge_weights(const sg_config* cfg, int64_t npts, const double* pts, int64_t* cell, double* dphi) {
  if (!cfg || npts < 0 || (npts > 0 && (!pts || !cell || !dphi))) return SG_ERR_ARG;
  if (cfg->dim < 1 || cfg->dim > 3 || cfg->degree < 1 || cfg->degree > 4) return SG_ERR_ARG;
  for (int a = 0; a < cfg->dim; ++a)
    if (cfg->n[a] < 1 || !(cfg->h[a] > 0.0)) return SG_ERR_ARG;
  NodeGeom G;
  if (!G.init(cfg, cfg->degree)) return SG_ERR_ARG;
  const int d = cfg->dim, kind = cfg->diagonal == SG_DIAGONAL_QUAD ? KIND_TENSOR : KIND_SIMPLEX;
  const int nd = G.nq;
  for (int64_t k = 0; k < npts; ++k) {
    double xi[3] = {0, 0, 0};
    double* const D = dphi + (size_t)k * d * nd;
    cell[k] = locate_point(G, pts + k * d, xi);
    if (cell[k] >= 0)
      gauge_weights(d, cfg->degree, kind, nd, xi, D);
    else
      for (int a = 0; a < d * nd; ++a) D[a] = 0.0;
  }
  return nd;
}

int sg_locate_points(const sg_config* cfg, int64_t npts, const double* pts, int64_t* cell, double* xi) {
  if (!cfg || npts < 0 || (npts > 0 && (!pts || !cell || !xi))) return SG_ERR_ARG;
  if (cfg->dim < 1 || cfg->dim > 3 || cfg->degree < 1 || cfg->degree > 8) return SG_ERR_ARG;
  for (int a = 0; a < cfg->dim; ++a)
    if (cfg->n[a] < 1 || !(cfg->h[a] > 0.0)) return SG_ERR_ARG;
  NodeGeom G;
  if (!G.init(cfg, cfg->degree)) return SG_ERR_ARG;
  const int d = cfg->dim;
  for (int64_t k = 0; k < npts; ++k) {
    for (int m = 0; m < d; ++m) xi[k * d + m] = 0.0;
    cell[k] = locate_point(G, pts + k * d, xi + k * d);
  }
  return SG_OK;
}

int sg_block_node_coords(const sg_config* cfg, int degree, double* out, size_t nbytes) {
  if (!cfg || !out || degree < 1 || degree > 8 || cfg->dim < 1 || cfg->dim > 3) return SG_ERR_ARG;
  NodeGeom G;
  if (!G.init(cfg, degree)) return SG_ERR_ARG;
  const int d = G.d;
  int n[3] = {1, 1, 1};
  for (int a = 0; a < d; ++a) n[a] = cfg->n[a];
  if (nbytes != (size_t)n[0] * n[1] * n[2] * G.ncls * G.nq * d * sizeof(double)) return SG_ERR_ARG;
  size_t o = 0;
  for (int ck = 0; ck < n[2]; ++ck)
    for (int cj = 0; cj < n[1]; ++cj)
      for (int ci = 0; ci < n[0]; ++ci) {
        const int c[3] = {ci, cj, ck};
        for (int k = 0; k < G.ncls; ++k)
          for (int a = 0; a < G.nq; ++a) {
            double x[3];
            G.node(c, k, a, x);
            for (int i = 0; i < d; ++i) out[o++] = x[i];
          }
      }
  return SG_OK;
}

int64_t sg_reference_operator(int dim, int degree, int which, int q, double* out, size_t nbytes) {
  return sg_reference_operator_cell(0, dim, degree, which, q, out, nbytes);
}

int64_t sg_reference_operator_cell(int cell_type, int dim, int degree, int which, int q, double* out, size_t nbytes) {
  std::vector<double> v;
  if (cell_type != KIND_SIMPLEX && cell_type != KIND_TENSOR) return SG_ERR_ARG;
  try {
    if (which == 3) {
      if (q < 1 || q > 6 || dim < 1 || dim > 3 || degree < 1 || degree > 4) return SG_ERR_ARG;
      v = sponge_tensor(dim, degree, q, cell_type);
    } else {
      RefElem re = make_refelem(dim, degree, cell_type);
      if (which == 0) v = re.D;
      else if (which == 1) v = re.L;
      else if (which == 2) v = re.Mhat;
      else if (which == 4) v.assign(re.fnode.begin(), re.fnode.end());
      else return SG_ERR_ARG;
    }
  } catch (const std::exception& e) {
    g_create_err = e.what();
    return SG_ERR_ARG;
  }
  if (out) {
    if (nbytes != v.size() * sizeof(double)) return SG_ERR_ARG;
    std::memcpy(out, v.data(), nbytes);
  }
  return (int64_t)v.size();
}

int sg_tabulate(int dim, int degree, int64_t npts, const double* xi, double* phi) {
  return sg_tabulate_cell(0, dim, degree, npts, xi, phi);
}

int sg_tabulate_cell(int cell_type, int dim, int degree, int64_t npts, const double* xi, double* phi) {
  if (dim < 1 || dim > 3 || degree < 1 || degree > 8 || npts < 0 || !xi || !phi) return SG_ERR_ARG;
  if (cell_type != KIND_SIMPLEX && cell_type != KIND_TENSOR) return SG_ERR_ARG;
  tabulate(dim, degree, (int)npts, xi, phi, cell_type);
  return SG_OK;
}

int sg_mesh_tables(int dim, int degree, int diagonal, const double* h, int32_t* nb, int32_t* nb_node, double* cn,
                   double* jinv) {
  if (!h || !nb || !nb_node || !cn || !jinv) return SG_ERR_ARG;
  try {
    RefElem re = make_refelem(dim, degree, diagonal == SG_DIAGONAL_QUAD ? KIND_TENSOR : KIND_SIMPLEX);
    MeshDev md;
    std::memset(&md, 0, sizeof(md));
    md.nd = re.nd;
    md.nf = re.nf;
    double hh[3] = {1, 1, 1};
    for (int a = 0; a < dim; ++a) hh[a] = h[a];
    build_mesh_tables(dim, degree, diagonal, hh, re.fnode.data(), re.lattice.data(), md);
    for (int c = 0; c < md.ncls; ++c) {
      for (int f = 0; f < md.nfaces; ++f) {
        int32_t* o = nb + ((size_t)c * md.nfaces + f) * 5;
        o[0] = md.nb_axis[c][f];
        o[1] = md.nb_dir[c][f];
        o[2] = md.nb_cls[c][f];
        o[3] = md.nb_face[c][f];
        o[4] = md.face_ord[c][f];
        for (int b = 0; b < md.nf; ++b) nb_node[((size_t)c * md.nfaces + f) * md.nf + b] = md.nb_node[c][f][b];
        for (int j = 0; j < 3; ++j) cn[((size_t)c * md.nfaces + f) * 3 + j] = md.cn[c][f][j];
      }
      for (int r = 0; r < 3; ++r)
        for (int j = 0; j < 3; ++j) jinv[((size_t)c * 3 + r) * 3 + j] = md.Jinv[c][r][j];
    }
  } catch (const std::exception& e) {
    g_create_err = e.what();
    return SG_ERR_ARG;
  }
  return SG_OK;
}

int sg_region_boxes(const sg_config* cfg, int region, int32_t* boxes, int max_boxes) {
  if (!cfg || !boxes || cfg->dim < 1 || cfg->dim > 3 || region < 0 || region > 4 || max_boxes < 0) return SG_ERR_ARG;
  int32_t n[3] = {1, 1, 1}, has_nbr[6] = {0, 0, 0, 0, 0, 0};
  for (int a = 0; a < cfg->dim; ++a) n[a] = cfg->n[a];
  for (int s2 = 0; s2 < 2 * cfg->dim; ++s2) has_nbr[s2] = (cfg->nbr_mask >> s2) & 1;
  std::vector<Box> out;
  region_boxes(cfg->dim, n, has_nbr, region, out, shell_width_x(family_gw(choose_kernel_path(*cfg)), n[0], has_nbr[0] != 0, has_nbr[1] != 0));
  int cnt = 0;
  for (const Box& b : out) {
    if (b.n[0] <= 0 || b.n[1] <= 0 || b.n[2] <= 0) continue;
    if (cnt < max_boxes)
      for (int k = 0; k < 3; ++k) {
        boxes[6 * cnt + k] = b.o[k];
        boxes[6 * cnt + 3 + k] = b.n[k];
      }
    cnt += 1;
  }
  return cnt;
}

}  // extern "C"
