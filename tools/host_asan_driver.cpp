// CPU sanitizer driver (SURVEY 5 "sanitizers"; `make -C seigen_amd/csrc host-asan`): everything of libseigen_hip that
// needs no device - reference elements, mesh tables, MFMA fragment tables, the sponge, source, receiver and injector plans, the items
// of split-stage regions, the stage table, what stepping remembers between calls, the correlation's plan, the gradient's tables and plan, the device-free C-ABI entry points - built with
// -fsanitize=address,undefined and walked over every (dim, degree, cell type, diagonal) the library accepts, plus the
// argument errors the entry points must refuse.  Exit code 0 and no sanitizer report = clean.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <stdexcept>
#include <vector>

#include "hostlogic.hpp"
#include "kernels.hpp"
#include "mfma_tables.hpp"
#include "source_tables.hpp"
#include "sponge_tables.hpp"

using namespace sg;

static int nfail = 0;
#define EXPECT(cond)                                                        \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
      nfail += 1;                                                           \
    }                                                                       \
  } while (0)

static double checksum(const std::vector<double>& v) {
  double s = 0;
  for (double x : v) s += std::fabs(x);
  return s;
}

static void reference_operators(int cell_type, int dim, int degree) {
  for (int which = 0; which <= 4; ++which) {
    const int q = which == 3 ? 4 : 0;
    const int64_t n = sg_reference_operator_cell(cell_type, dim, degree, which, q, nullptr, 0);
    EXPECT(n > 0);
    if (n <= 0) continue;
    std::vector<double> v((size_t)n);
    EXPECT(sg_reference_operator_cell(cell_type, dim, degree, which, q, v.data(), v.size() * sizeof(double)) == n);
    EXPECT(std::isfinite(checksum(v)));
    // a wrong size must be refused, not written through
    EXPECT(sg_reference_operator_cell(cell_type, dim, degree, which, q, v.data(), (v.size() - 1) * sizeof(double)) == SG_ERR_ARG);
  }
  // tabulation at the lattice points = the identity (Lagrange basis), degrees up to 8
  for (int P = 1; P <= 8; ++P) {
    std::vector<int> lat;
    lattice_points(dim, P, lat, cell_type);
    const int nd = num_nodes(dim, P, cell_type);
    std::vector<double> xi((size_t)nd * dim), phi((size_t)nd * nd);
    for (size_t i = 0; i < xi.size(); ++i) xi[i] = (double)lat[i] / P;
    EXPECT(sg_tabulate_cell(cell_type, dim, P, nd, xi.data(), phi.data()) == SG_OK);
    double worst = 0;
    for (int p = 0; p < nd; ++p)
      for (int a = 0; a < nd; ++a) worst = std::fmax(worst, std::fabs(phi[(size_t)p * nd + a] - (p == a ? 1.0 : 0.0)));
    EXPECT(worst < 1e-9);
  }
}

static void mesh_tables(int dim, int degree, int diagonal) {
  const int kind = diagonal == SG_DIAGONAL_QUAD ? KIND_TENSOR : KIND_SIMPLEX;
  RefElem re = make_refelem(dim, degree, kind);
  const double h[3] = {0.5, 0.25, 2.0};
  std::vector<int32_t> nb((size_t)MAX_CLS * MAX_FACES * 5), nbn((size_t)MAX_CLS * MAX_FACES * (MAX_NF + 1));
  std::vector<double> cn((size_t)MAX_CLS * MAX_FACES * 3), jinv((size_t)MAX_CLS * 9);
  EXPECT(sg_mesh_tables(dim, degree, diagonal, h, nb.data(), nbn.data(), cn.data(), jinv.data()) == SG_OK);
}

static void mfma_tables_3d(int degree) {
  RefElem re = make_refelem(3, degree, KIND_SIMPLEX);
  EXPECT(!mfma_frags_F(re).empty() && !mfma_frags_G(re).empty() && !mfma_frags_L(re).empty());
  EXPECT(!mfma32_frags_F(re).empty() && !mfma32_frags_G(re).empty() && !mfma32_frags_L(re).empty());
  if (degree >= 3) {
    std::vector<double> Q, Pm;
    mfma_factorise_D(re, Q, Pm);
    EXPECT(!mfma_frags_Q(re).empty() && !mfma_frags_P(re).empty());
  }
  // the per-block tables of the MFMA path on small blocks, with and without neighbour blocks, ragged in x
  const int shapes[4][3] = {{16, 2, 2}, {5, 3, 2}, {33, 1, 3}, {1, 1, 1}};
  for (const auto& n : shapes)
    for (int mask : {0, 63, 5}) {
      MeshDev md;
      std::memset(&md, 0, sizeof(md));
      md.nd = re.nd;
      md.nf = re.nf;
      const double h[3] = {1.0 / n[0], 1.0 / n[1], 1.0 / n[2]};
      build_mesh_tables(3, degree, 0, h, re.fnode.data(), re.lattice.data(), md);
      for (int a = 0; a < 3; ++a) md.n[a] = n[a];
      for (int s = 0; s < 6; ++s) md.has_nbr[s] = (mask >> s) & 1;
      md.gw = 16;
      md.ncube = (int64_t)n[0] * n[1] * n[2];
      md.ncube_pad = (md.ncube + 15) / 16 * 16;
      const MfmaConst mk = mfma_const(md);
      EXPECT(mk.ncube == md.ncube);
      std::vector<int32_t> ft, tab;
      mfma_trace_offsets(md, 9, ft);
      mfma_trace_offsets(md, 3, ft);
      build_nbr_table(md, tab);
      EXPECT(tab.size() == (size_t)(md.ncube_pad / 16) * 6 * 64);
    }
}

// The stress lines a facet's scaled normal can see (mfma_tables.cpp mfma_trace_lines, read by kernels_mfma.hip load_trace /
// trace_flux) on two anisotropic cell sizes: one column along nb_axis on facets 0 and 3, two on facets 1 and 2; the flux
// formed from the listed lines alone equals the one over all three columns, in both storages, on a tensor that is not
// symmetric in full storage; and tables that break the rule are refused.
static void trace_lines_3d(int degree) {
  RefElem re = make_refelem(3, degree, KIND_SIMPLEX);
  const double hs[2][3] = {{0.3, 0.5, 0.7}, {2.0, 0.125, 0.75}};
  auto refused = [](const MeshDev& m, int k) {
    MfmaClassConst kc;
    std::memset(&kc, 0, sizeof(kc));
    try {
      mfma_trace_lines(m, k, kc);
    } catch (const std::runtime_error&) {
      return true;
    }
    return false;
  };
  for (const auto& h : hs) {
    MeshDev md;
    std::memset(&md, 0, sizeof(md));
    md.nd = re.nd;
    md.nf = re.nf;
    build_mesh_tables(3, degree, 0, h, re.fnode.data(), re.lattice.data(), md);
    for (int k = 0; k < 6; ++k) {
      MfmaClassConst kc;
      std::memset(&kc, 0, sizeof(kc));
      mfma_trace_lines(md, k, kc);
      for (int f = 0; f < 4; ++f) {
        const bool cube_face = f == 0 || f == 3;
        int nnz = 0;
        for (int j = 0; j < 3; ++j) nnz += md.cn[k][f][j] != 0.0;
        EXPECT(nnz == (cube_face ? 1 : 2));
        EXPECT(cube_face ? (kc.tr_col[f][0] == md.nb_axis[k][f] && kc.tr_col[f][1] == -1)
                         : (md.nb_axis[k][f] < 0 && kc.tr_col[f][0] >= 0 && kc.tr_col[f][0] < kc.tr_col[f][1] && kc.tr_col[f][1] < 3));
        EXPECT(cube_face ? kc.tr_cn[f][1] == 0.0 : kc.tr_cn[f][1] == md.cn[k][f][kc.tr_col[f][1]]);
        EXPECT(kc.tr_cn[f][0] == md.cn[k][f][kc.tr_col[f][0]]);
        for (int sym = 0; sym < 2; ++sym) {
          double slot[9];      // a node's nine slots: full storage holds T(i, j) at i * 3 + j, symmetric only the i <= j ones
          for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) slot[i * 3 + j] = (!sym || i <= j) ? 1.0 + 0.37 * i - 0.61 * j + 0.05 * i * j : std::nan("");
          for (int i = 0; i < 3; ++i) {
            double full = 0.0, part = 0.0;
            for (int j = 0; j < 3; ++j) full = std::fma(md.cn[k][f][j], slot[stress_line_slot(sym != 0, i, j)], full);
            for (int c = 0; c < (cube_face ? 1 : 2); ++c) {
              const int line = kc.tr_line[sym][f][3 * c + i];
              EXPECT(line >= 0 && line < 9 * 16 && line % 16 == 0);
              if (line < 0 || line >= 9 * 16) continue;
              EXPECT(line / 16 == stress_line_slot(sym != 0, i, kc.tr_col[f][c]));
              part = std::fma(kc.tr_cn[f][c], slot[line / 16], part);
            }
            EXPECT(full == part && std::isfinite(part));
          }
          // the entries the kernels never read still point into the node
          for (int c = 0; c < 6; ++c) EXPECT(kc.tr_line[sym][f][c] >= 0 && kc.tr_line[sym][f][c] < 9 * 16);
        }
      }
    }
    // what the kernels could not run on
    MeshDev bad = md;
    bad.cn[2][0][(md.nb_axis[2][0] + 1) % 3] = 1e-300;      // a second entry on a cube-face facet, however small
    EXPECT(refused(bad, 2) && !refused(md, 2));
    bad = md;
    for (int j = 0; j < 3; ++j)
      if (md.cn[1][1][j] == 0.0) bad.cn[1][1][j] = 1.0;      // a third entry on an inner facet
    EXPECT(refused(bad, 1));
    bad = md;
    bad.cn[4][2][0] = bad.cn[4][2][1] = bad.cn[4][2][2] = 0.0;
    bad.cn[4][2][1] = 1.0;                                   // one entry on an inner facet
    EXPECT(refused(bad, 4));
    bad = md;
    bad.nb_axis[0][3] = -1;                                  // a cube-face facet without its axis
    EXPECT(refused(bad, 0));
    bad = md;
    bad.nb_axis[5][0] = (md.nb_axis[5][0] + 1) % 3;          // the entry is not along the axis
    EXPECT(refused(bad, 5));
    bad = md;
    bad.nb_axis[3][1] = 0;                                   // an inner facet that claims an axis
    EXPECT(refused(bad, 3));
    bad = md;
    bad.cn[0][0][md.nb_axis[0][0]] = std::nan("");
    EXPECT(refused(bad, 0));
    bool whole_refused = false;
    try {
      (void)mfma_const(bad);
    } catch (const std::runtime_error&) {
      whole_refused = true;
    }
    EXPECT(whole_refused);
  }
}

// The class frame of the F stages (mfma_tables.cpp mfma_class_frame): p, s and the permuted (c n) rebuild the block's tables
// exactly, every line offset is stress_line_slot of the permuted pair, the difference tiles are the E_m - E_(m-1) of the
// operators, and tables of any other shape - one more non-zero, a J^-1 that is not the bidiagonal in the order p - are refused.
static void class_frame_3d(int degree) {
  RefElem re = make_refelem(3, degree, KIND_SIMPLEX);
  const double hs[2][3] = {{0.3, 0.5, 0.7}, {2.0, 0.125, 0.75}};
  auto refused = [](const MeshDev& m, int k) {
    MfmaClassConst kc;
    std::memset(&kc, 0, sizeof(kc));
    try {
      mfma_class_frame(m, k, kc);
    } catch (const std::runtime_error&) {
      return true;
    }
    return false;
  };
  double emax = 0.0;
  for (int m = 0; m < 3; ++m)
    for (int a = 0; a < re.nd; ++a)
      for (int b = 0; b < re.nd; ++b) emax = std::fmax(emax, std::fabs(mfma_E(re, m, a, b)));
  for (int m = 0; m < 3; ++m)
    for (int a = 0; a < re.nd; a += 3)
      for (int b = 0; b < re.nd; ++b) {
        // (the tiles take the difference before rounding, this one after: at most two roundings in each E, one in the
        // difference and one in E', each half an ulp of the largest entry at most)
        const double e1 = mfma_E(re, m, a, b), e0 = m > 0 ? mfma_E(re, m - 1, a, b) : 0.0;
        EXPECT(std::fabs(mfma_Ediff(re, m, a, b) - (e1 - e0)) <= 6 * 0x1p-53 * emax);
      }
  EXPECT(mfma_Ediff(re, 1, re.nd, 0) == 0.0 && mfma_Ediff(re, 1, 0, re.nd) == 0.0);
  for (const auto& h : hs) {
    MeshDev md;
    std::memset(&md, 0, sizeof(md));
    md.nd = re.nd;
    md.nf = re.nf;
    build_mesh_tables(3, degree, 0, h, re.fnode.data(), re.lattice.data(), md);
    for (int k = 0; k < 6; ++k) {
      MfmaClassConst kc;
      std::memset(&kc, 0, sizeof(kc));
      mfma_class_frame(md, k, kc);
      const int* p = kc.cf_p;
      EXPECT(p[0] >= 0 && p[0] < 3 && p[1] >= 0 && p[1] < 3 && p[2] >= 0 && p[2] < 3 && p[0] != p[1] && p[0] != p[2] && p[1] != p[2]);
      double J[3][3] = {{0}}, cn[4][3] = {{0}};
      for (int r = 0; r < 3; ++r) {
        J[r][p[r]] = kc.cf_s[r];
        if (r < 2) J[r][p[r + 1]] = -kc.cf_s[r + 1];
      }
      cn[0][p[0]] = kc.cf_cn[0][0];
      cn[1][p[0]] = kc.cf_cn[1][0];
      cn[1][p[1]] = kc.cf_cn[1][1];
      cn[2][p[1]] = kc.cf_cn[2][0];
      cn[2][p[2]] = kc.cf_cn[2][1];
      cn[3][p[2]] = kc.cf_cn[3][0];
      for (int r = 0; r < 3; ++r)
        for (int j = 0; j < 3; ++j) EXPECT(J[r][j] == md.Jinv[k][r][j]);
      for (int f = 0; f < 4; ++f)
        for (int j = 0; j < 3; ++j) EXPECT(cn[f][j] == md.cn[k][f][j]);
      EXPECT(kc.cf_cn[0][1] == 0.0 && kc.cf_cn[3][1] == 0.0);
      for (int sym = 0; sym < 2; ++sym) {
        for (int a = 0; a < 3; ++a) {
          EXPECT(kc.cf_vel[a] == 16 * p[a]);
          for (int b = 0; b < 3; ++b) EXPECT(kc.cf_own[sym][3 * a + b] == 16 * stress_line_slot(sym != 0, p[a], p[b]));
        }
        for (int f = 0; f < 4; ++f)
          for (int c = 0; c < 6; ++c) EXPECT(kc.cf_tr[sym][f][c] >= 0 && kc.cf_tr[sym][f][c] < 9 * 16 && kc.cf_tr[sym][f][c] % 16 == 0);
        // the flux from the listed lines alone is the flux over all three columns (the tensor not symmetric in full storage)
        double slot[9];
        for (int i = 0; i < 3; ++i)
          for (int j = 0; j < 3; ++j) slot[i * 3 + j] = (!sym || i <= j) ? 1.0 + 0.37 * i - 0.61 * j + 0.05 * i * j : std::nan("");
        for (int f = 0; f < 4; ++f)
          for (int i = 0; i < 3; ++i) {      // row i of the frame = component p[i]
            double full = 0.0, part;
            for (int j = 0; j < 3; ++j) full = std::fma(md.cn[k][f][p[j]], slot[stress_line_slot(sym != 0, p[i], p[j])], full);
            const int32_t* t = kc.cf_tr[sym][f];
            if (f == 0 || f == 3) {
              part = kc.cf_cn[f][0] * slot[t[i] / 16];
            } else if (sym) {
              const int x = f == 1 ? 0 : 2, a = i == x ? 0 : (i == 1 ? 1 : 3);
              part = f == 1 ? std::fma(kc.cf_cn[f][1], slot[t[a + 1] / 16], kc.cf_cn[f][0] * slot[t[a] / 16])
                            : std::fma(kc.cf_cn[f][1], slot[t[a] / 16], kc.cf_cn[f][0] * slot[t[a + 1] / 16]);
            } else {
              part = std::fma(kc.cf_cn[f][1], slot[t[3 + i] / 16], kc.cf_cn[f][0] * slot[t[i] / 16]);
            }
            EXPECT(full == part && std::isfinite(part));
          }
      }
    }
    // what the kernels could not run on
    EXPECT(!refused(md, 0) && !refused(md, 5));
    for (int k = 0; k < 6; ++k)
      for (int r = 0; r < 3; ++r)
        for (int j = 0; j < 3; ++j)
          if (md.Jinv[k][r][j] == 0.0) {
            MeshDev bad = md;
            bad.Jinv[k][r][j] = 1e-300;                         // one more non-zero in J^-1, however small
            EXPECT(refused(bad, k));
          }
    MeshDev bad = md;
    bad.Jinv[1][0][md.nb_axis[1][0]] *= 1.0 + 1e-15;            // the entry above a diagonal one is no longer its negative ...
    EXPECT(refused(bad, 1));
    bad = md;
    for (int j = 0; j < 3; ++j)
      if (md.cn[3][1][j] == 0.0) bad.cn[3][1][j] = 1e-300;      // one more non-zero in a scaled normal
    EXPECT(refused(bad, 3));
    bad = md;
    bad.cn[2][3][md.nb_axis[2][3]] *= 2.0;                      // a scaled normal that is not -1/2 grad lambda
    EXPECT(refused(bad, 2));
    bad = md;
    std::swap(bad.Jinv[4][0], bad.Jinv[4][2]);                  // the bidiagonal upside down
    EXPECT(refused(bad, 4));
    bad = md;
    bad.Jinv[0][2][md.nb_axis[0][3]] = -md.Jinv[0][2][md.nb_axis[0][3]];      // a negative scale
    EXPECT(refused(bad, 0));
    bad = md;
    bad.Jinv[5][1][0] = std::nan("");
    EXPECT(refused(bad, 5));
    bad = md;
    bad.nb_axis[2][0] = (md.nb_axis[2][0] + 1) % 3;             // facet 0 does not cross the face normal to p[0]
    EXPECT(refused(bad, 2));
    bool whole_refused = false;
    bad = md;
    bad.Jinv[3][2][(md.nb_axis[3][3] + 1) % 3] = 1e-300;
    try {
      (void)mfma_const(bad);
    } catch (const std::runtime_error&) {
      whole_refused = true;
    }
    EXPECT(whole_refused);
  }
}

static void tile_tables_2d(int degree, int kind) {
  RefElem re = make_refelem(2, degree, kind);
  EXPECT(!tile2d_frags_V(re, 1.0).empty() && !tile2d_frags_V(re, -1.0).empty() && !tile2d_frags_L(re).empty());
  EXPECT(!tile2d_frags32_V(re, 1.0).empty() && !tile2d_frags32_L(re).empty());
  MeshDev md;
  std::memset(&md, 0, sizeof(md));
  md.nd = re.nd;
  md.nf = re.nf;
  const double h[3] = {0.1, 0.2, 1.0};
  build_mesh_tables(2, degree, kind == KIND_TENSOR ? SG_DIAGONAL_QUAD : 0, h, re.fnode.data(), re.lattice.data(), md);
  md.n[0] = 7;
  md.n[1] = 3;
  md.n[2] = 1;
  md.gw = 16;
  md.ncube = 21;
  md.ncube_pad = 32;
  (void)tile2d_const(md);
}

static void regions_and_coords() {
  for (int dim = 1; dim <= 3; ++dim)
    for (int diagonal : {0, 1, 2}) {
      if (diagonal == 2 && dim == 1) continue;
      for (int degree = 1; degree <= 4; ++degree)
        for (int mask = 0; mask < (1 << (2 * dim)); mask += (dim == 3 ? 7 : 1)) {
          sg_config cfg;
          std::memset(&cfg, 0, sizeof(cfg));
          cfg.dim = dim;
          cfg.degree = degree;
          cfg.n[0] = 19;
          cfg.n[1] = dim > 1 ? 5 : 1;
          cfg.n[2] = dim > 2 ? 4 : 1;
          for (int a = 0; a < 3; ++a) cfg.h[a] = 0.5 + a;
          cfg.diagonal = diagonal;
          cfg.nbr_mask = mask;
          cfg.cube0[0] = 3;
          for (int region = 0; region <= 4; ++region) {
            int32_t boxes[SG_MAX_REGION_BOXES * 6];
            const int nb = sg_region_boxes(&cfg, region, boxes, SG_MAX_REGION_BOXES);
            EXPECT(nb >= 0 && nb <= SG_MAX_REGION_BOXES);
            EXPECT(sg_region_boxes(&cfg, region, boxes, 0) == nb);   // count only: nothing written
          }
          if (mask == 0) {
            sg_config small = cfg;
            small.n[0] = 3;
            small.n[1] = dim > 1 ? 2 : 1;
            small.n[2] = dim > 2 ? 2 : 1;
            NodeGeom G;
            EXPECT(G.init(&small, degree));
            const size_t cells = (size_t)small.n[0] * small.n[1] * small.n[2] * G.ncls;
            std::vector<double> X(cells * G.nq * dim);
            EXPECT(sg_block_node_coords(&small, degree, X.data(), X.size() * sizeof(double)) == SG_OK);
            EXPECT(sg_block_node_coords(&small, degree, X.data(), X.size() * sizeof(double) - 8) == SG_ERR_ARG);
          }
        }
    }
  EXPECT(sg_region_boxes(nullptr, 0, nullptr, 0) == SG_ERR_ARG);
}

// sg_locate_points (the receivers' point location) on every dim, cell kind and degree: points inside cells, on cube faces,
// edges and vertices (grid lines), on the faces between the simplices of a cube, on the mesh boundary and outside; the
// blocks of a 2 x 2 x 2 (2-D: 2 x 2, 1-D: 2) split must own every point inside exactly once, in the cell the whole mesh finds
static void point_location() {
  for (int dim = 1; dim <= 3; ++dim)
    for (int diagonal : {0, 1, 2}) {
      if (diagonal == 2 && dim == 1) continue;
      for (int degree = 1; degree <= 4; ++degree) {
        sg_config whole;
        std::memset(&whole, 0, sizeof(whole));
        whole.dim = dim;
        whole.degree = degree;
        for (int a = 0; a < 3; ++a) {
          whole.n[a] = a < dim ? 4 : 1;
          whole.h[a] = a < dim ? 0.25 * (a + 1) : 1.0;
        }
        whole.diagonal = diagonal;
        std::vector<double> pts;
        // fractions of a cube: on lines (0), on the inner faces (equal / complementary), inside; cubes -1 .. 4
        const double fr[] = {0.0, 0.25, 0.5, 0.75, 0.3, 0.7};
        for (int cz = (dim > 2 ? -1 : 0); cz <= (dim > 2 ? 4 : 0); ++cz)
          for (int cy = (dim > 1 ? -1 : 0); cy <= (dim > 1 ? 4 : 0); ++cy)
            for (int cx = -1; cx <= 4; ++cx)
              for (int f = 0; f < 6; ++f) {
                const int c[3] = {cx, cy, cz};
                for (int a = 0; a < dim; ++a) pts.push_back((c[a] + (a == 1 ? 1.0 - fr[f] : fr[f])) * whole.h[a]);
              }
        const int64_t np = (int64_t)pts.size() / dim;
        std::vector<int64_t> cell1(np), cell(np);
        std::vector<double> xi1(pts.size()), xi(pts.size());
        EXPECT(sg_locate_points(&whole, np, pts.data(), cell1.data(), xi1.data()) == SG_OK);
        std::vector<int> owners(np, 0);
        for (int b = 0; b < (1 << dim); ++b) {
          sg_config blk = whole;
          for (int a = 0; a < dim; ++a) {
            const int hi = (b >> a) & 1;
            blk.n[a] = 2;
            blk.cube0[a] = 2 * hi;
            blk.nbr_mask |= 1 << (2 * a + (1 - hi));
          }
          EXPECT(sg_locate_points(&blk, np, pts.data(), cell.data(), xi.data()) == SG_OK);
          for (int64_t k = 0; k < np; ++k) {
            if (cell[k] < 0) continue;
            owners[k] += 1;
            const int ncls = dim == 1 || diagonal == 2 ? 1 : (dim == 2 ? 2 : 6);
            const int64_t cube = cell[k] / ncls;
            const int64_t lc[3] = {cube % 2, (cube / 2) % 2, cube / 4};
            int64_t g = 0, mul = 1;
            for (int a = 0; a < dim; ++a) {
              g += (lc[a] + blk.cube0[a]) * mul;
              mul *= 4;
            }
            EXPECT(g * ncls + cell[k] % ncls == cell1[k]);
            for (int a = 0; a < dim; ++a) EXPECT(xi[k * dim + a] == xi1[k * dim + a]);
          }
        }
        for (int64_t k = 0; k < np; ++k) {
          EXPECT(owners[k] == (cell1[k] >= 0 ? 1 : 0));
          bool inside = true;
          for (int a = 0; a < dim; ++a) inside = inside && pts[k * dim + a] >= 0.0 && pts[k * dim + a] <= 4 * whole.h[a];
          EXPECT(inside == (cell1[k] >= 0));
          for (int a = 0; a < dim && cell1[k] >= 0; ++a) EXPECT(xi1[k * dim + a] >= -1e-12 && xi1[k * dim + a] <= 1.0 + 1e-12);
        }
      }
    }
  sg_config cfg;
  std::memset(&cfg, 0, sizeof(cfg));
  cfg.dim = 2;
  cfg.degree = 2;
  cfg.n[0] = cfg.n[1] = 2;
  cfg.h[0] = cfg.h[1] = 1.0;
  double p[2] = {0.5, 0.5}, x[2];
  int64_t c = 0;
  EXPECT(sg_locate_points(&cfg, -1, p, &c, x) == SG_ERR_ARG);
  EXPECT(sg_locate_points(&cfg, 1, nullptr, &c, x) == SG_ERR_ARG);
  EXPECT(sg_locate_points(nullptr, 1, p, &c, x) == SG_ERR_ARG);
  EXPECT(sg_locate_points(&cfg, 1, p, &c, x) == SG_OK && c >= 0);
  cfg.h[1] = 0.0;
  EXPECT(sg_locate_points(&cfg, 1, p, &c, x) == SG_ERR_ARG);
}

// Which kernel family runs a block (hostapi.cpp choose_kernel_path), pinned row by row: one row on each side of every size
// threshold, and every SEIGEN_HIP_PATH value - unset, the four names, an unknown string - for each dimension and cell type.
// (The lane thresholds only decide in 1-D: 2-D simplices take the tile kernels and 3-D ones the MFMA kernels first.)
static void kernel_family_table() {
  using F = Family;
  const int64_t hx = SG_HEX_LANE_MIN_CELLS(1), hx2 = SG_HEX_LANE_MIN_CELLS(2);
  struct Row {
    const char* path;   // SEIGEN_HIP_PATH, nullptr = unset
    int dim, diagonal, degree;
    int64_t n0, n1, n2;
    Family family;
    int gw;
  };
  const int Q = SG_DIAGONAL_QUAD;
  const Row rows[] = {
      // unset: the measured thresholds
      {nullptr, 1, 0, 1, 196607, 1, 1, F::Generic, 1},
      {nullptr, 1, 0, 1, 196608, 1, 1, F::Lane, 64},
      {nullptr, 1, 0, 2, 119999, 1, 1, F::Generic, 1},
      {nullptr, 1, 0, 2, 120000, 1, 1, F::Lane, 64},
      {nullptr, 1, 0, 4, 119999, 1, 1, F::Generic, 1},
      {nullptr, 1, 0, 4, 120000, 1, 1, F::Lane, 64},
      {nullptr, 2, 0, 1, 2, 2, 1, F::Tile2d, 16},
      {nullptr, 2, 1, 4, 512, 512, 1, F::Tile2d, 16},
      {nullptr, 3, 0, 1, 1, 1, 10922, F::Generic, 1},      // 65532 cells
      {nullptr, 3, 1, 1, 1, 1, 10923, F::Mfma, 16},        // 65538 cells
      {nullptr, 3, 0, 2, 2, 2, 2, F::Mfma, 16},
      {nullptr, 3, 0, 4, 2, 2, 2, F::Mfma, 16},
      {nullptr, 2, Q, 1, 2, 2, 1, F::Tile2d, 16},
      {nullptr, 2, Q, 4, 512, 512, 1, F::Tile2d, 16},
      {nullptr, 3, Q, 1, hx - 1, 1, 1, F::Generic, 1},
      {nullptr, 3, Q, 1, hx, 1, 1, F::Lane, 64},
      {nullptr, 3, Q, 2, hx2 - 1, 1, 1, F::Generic, 1},
      {nullptr, 3, Q, 2, hx2, 1, 1, F::Lane, 64},
      {nullptr, 3, Q, 3, 2, 2, 2, F::Hexm, 16},
      {nullptr, 3, Q, 4, 2, 2, 2, F::Hexm, 16},
      // generic: everywhere
      {"generic", 1, 0, 1, 196608, 1, 1, F::Generic, 1},
      {"generic", 2, 0, 2, 512, 512, 1, F::Generic, 1},
      {"generic", 3, 0, 1, 1, 1, 10923, F::Generic, 1},
      {"generic", 3, 0, 4, 2, 2, 2, F::Generic, 1},
      {"generic", 2, Q, 2, 512, 512, 1, F::Generic, 1},
      {"generic", 3, Q, 1, hx, 1, 1, F::Generic, 1},
      {"generic", 3, Q, 4, 2, 2, 2, F::Generic, 1},
      // lane: wherever lane kernels exist; not 3-D simplices P3 / P4 (generic), not 2-D quadrilaterals (tile), not DQ_3 / DQ_4
      {"lane", 1, 0, 1, 8, 1, 1, F::Lane, 64},
      {"lane", 1, 0, 4, 8, 1, 1, F::Lane, 64},
      {"lane", 2, 0, 1, 2, 2, 1, F::Lane, 64},
      {"lane", 2, 0, 4, 512, 512, 1, F::Lane, 64},
      {"lane", 3, 0, 1, 1, 1, 10923, F::Lane, 64},
      {"lane", 3, 0, 2, 2, 2, 2, F::Lane, 64},
      {"lane", 3, 0, 3, 2, 2, 2, F::Generic, 1},
      {"lane", 3, 0, 4, 2, 2, 2, F::Generic, 1},
      {"lane", 2, Q, 2, 2, 2, 1, F::Tile2d, 16},
      {"lane", 3, Q, 1, 2, 2, 2, F::Lane, 64},
      {"lane", 3, Q, 2, 2, 2, 2, F::Lane, 64},
      {"lane", 3, Q, 3, 2, 2, 2, F::Hexm, 16},
      // mfma: 3-D P1 simplices below the threshold; elsewhere as unset
      {"mfma", 1, 0, 1, 8, 1, 1, F::Generic, 1},
      {"mfma", 1, 0, 1, 196608, 1, 1, F::Lane, 64},
      {"mfma", 2, 0, 3, 2, 2, 1, F::Tile2d, 16},
      {"mfma", 3, 0, 1, 2, 2, 2, F::Mfma, 16},
      {"mfma", 3, 0, 1, 1, 1, 10923, F::Mfma, 16},
      {"mfma", 2, Q, 3, 2, 2, 1, F::Tile2d, 16},
      {"mfma", 3, Q, 1, hx - 1, 1, 1, F::Generic, 1},
      {"mfma", 3, Q, 1, hx, 1, 1, F::Lane, 64},
      {"mfma", 3, Q, 3, 2, 2, 2, F::Hexm, 16},
      // tile: as unset (the tile kernels are the default wherever they exist; ignored in 1-D and 3-D)
      {"tile", 1, 0, 1, 8, 1, 1, F::Generic, 1},
      {"tile", 1, 0, 1, 196608, 1, 1, F::Lane, 64},
      {"tile", 2, 0, 1, 2, 2, 1, F::Tile2d, 16},
      {"tile", 3, 0, 1, 2, 2, 2, F::Generic, 1},
      {"tile", 3, 0, 1, 1, 1, 10923, F::Mfma, 16},
      {"tile", 2, Q, 1, 2, 2, 1, F::Tile2d, 16},
      {"tile", 3, Q, 1, 2, 2, 2, F::Generic, 1},
      {"tile", 3, Q, 1, hx, 1, 1, F::Lane, 64},
      {"tile", 3, Q, 4, 2, 2, 2, F::Hexm, 16},
      // an unknown string (or an empty one): as unset
      {"bogus", 1, 0, 1, 196607, 1, 1, F::Generic, 1},
      {"bogus", 1, 0, 1, 196608, 1, 1, F::Lane, 64},
      {"bogus", 2, 0, 2, 2, 2, 1, F::Tile2d, 16},
      {"bogus", 3, 0, 1, 2, 2, 2, F::Generic, 1},
      {"bogus", 3, 0, 1, 1, 1, 10923, F::Mfma, 16},
      {"bogus", 3, 0, 3, 2, 2, 2, F::Mfma, 16},
      {"bogus", 2, Q, 2, 2, 2, 1, F::Tile2d, 16},
      {"bogus", 3, Q, 1, hx - 1, 1, 1, F::Generic, 1},
      {"bogus", 3, Q, 2, hx2, 1, 1, F::Lane, 64},
      {"bogus", 3, Q, 3, 2, 2, 2, F::Hexm, 16},
      {"", 3, 0, 1, 2, 2, 2, F::Generic, 1},
      {"", 2, 0, 1, 2, 2, 1, F::Tile2d, 16},
  };
  for (const Row& r : rows) {
    sg_config cfg;
    std::memset(&cfg, 0, sizeof(cfg));
    cfg.dim = r.dim;
    cfg.diagonal = r.diagonal;
    cfg.degree = r.degree;
    cfg.n[0] = (int32_t)r.n0;
    cfg.n[1] = (int32_t)r.n1;
    cfg.n[2] = (int32_t)r.n2;
    for (int a = 0; a < 3; ++a) cfg.h[a] = 1.0;
    if (r.path) setenv("SEIGEN_HIP_PATH", r.path, 1);
    else unsetenv("SEIGEN_HIP_PATH");
    const Family f = choose_kernel_path(cfg);
    const int gw = family_gw(f);
    if (f != r.family || gw != r.gw) {
      std::fprintf(stderr, "FAIL kernel family: SEIGEN_HIP_PATH=%s dim %d diagonal %d degree %d n %lld x %lld x %lld: family %d gw %d, want %d gw %d\n",
                   r.path ? r.path : "(unset)", r.dim, r.diagonal, r.degree, (long long)r.n0, (long long)r.n1, (long long)r.n2, (int)f, gw,
                   (int)r.family, r.gw);
      nfail += 1;
    }
  }
  unsetenv("SEIGEN_HIP_PATH");
}

// sg_set_absorption's host half (csrc/sponge_tables.cpp): every kind of cell - none, constant, affine, general - side by side on
// ragged blocks (a last group with padding), every family flavour (scalar or not, pre-pass or not, records or lines)
static void sponge_plans(int dim, int degree, int kind, int q) {
  const int nd = num_nodes(dim, degree, kind), nq = num_nodes(dim, q, kind);
  std::vector<int> latQ;
  lattice_points(dim, q, latQ, kind);
  const int ncls = kind == KIND_TENSOR ? 1 : (dim == 1 ? 1 : (dim == 2 ? 2 : 6));
  for (int gw : {1, 16, 64}) {
    const int64_t ncube = 37, ncells = ncube * ncls;      // 37 cubes: the last group is padded at gw = 16 and 64
    std::vector<double> sigma((size_t)ncells * nq, 0.0);
    unsigned seed = 12345u + (unsigned)(dim * 100 + degree * 10 + q);
    auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return (double)(seed >> 8) / (double)(1u << 24); };
    std::vector<int> want((size_t)ncells);
    for (int64_t e = 0; e < ncells; ++e) {
      const int what = (int)(rnd() * 4.0) & 3;      // 0 none, 1 constant, 2 affine, 3 general
      want[(size_t)e] = what;
      const double s0 = 1.0 + 9.0 * rnd(), g[3] = {rnd() - 0.5, rnd() - 0.5, rnd() - 0.5};
      for (int c = 0; c < nq; ++c) {
        double v = 0.0;
        if (what == 1) v = s0;
        if (what == 2) {
          v = s0;
          for (int k = 0; k < dim; ++k) v += g[k] * (double)latQ[(size_t)c * dim + k] / q;
        }
        if (what == 3) v = 10.0 * rnd();
        sigma[(size_t)e * nq + c] = v;
      }
    }
    for (int flavour = 0; flavour < 5; ++flavour) {
      SpongeRequest rq;
      rq.dim = dim; rq.degree = degree; rq.kind = kind; rq.sigma_degree = q; rq.ncells = ncells; rq.ncls = ncls; rq.gw = gw;
      rq.want_scalar = flavour >= 1;
      rq.pre_family = flavour >= 2;
      rq.try_affine = flavour >= 3;
      rq.line_layout = flavour == 4;
      const SpongePlan pl = plan_sponge(rq, sigma.data());
      EXPECT((int64_t)pl.slot.size() == ncells && pl.B.size() == (size_t)pl.nmat * nd * nd);
      int naff = 0;
      for (int64_t e = 0; e < ncells; ++e) {
        const int what = want[(size_t)e], sl = pl.slot[(size_t)e];
        const bool scalar = rq.want_scalar && what == 1;
        EXPECT((sl >= 0) == (what != 0 && !scalar));
        if (rq.want_scalar) {
          const double sg_ = pl.sig[(size_t)e];
          EXPECT(what == 0 ? sg_ == 0.0 : (what == 1 ? sg_ == sigma[(size_t)e * nq] : sg_ != sg_));
        }
        if (sl < 0) continue;
        EXPECT(sl < pl.nslots);
        if (!rq.pre_family) continue;
        EXPECT(pl.cells[(size_t)sl] == (int32_t)e);
        if (rq.line_layout) EXPECT(sl % gw == (int)((e / ncls) % gw));      // the cell's column of its item
        const bool affine = pl.mat_of[(size_t)sl] < 0;
        // q = 1 on a simplex: every sigma is affine; a constant cell of a family without scalars is affine too
        const bool must = what == 2 || (what == 1 && !rq.want_scalar) || (what == 3 && q == 1 && kind == KIND_SIMPLEX);
        EXPECT(affine == (rq.try_affine && must));
        if (affine) {
          naff += 1;
          for (int c = 0; c < nq; ++c) {      // the coefficients reproduce the nodal sigma
            double v = pl.aff_coef[(size_t)sl * (dim + 1)];
            for (int k = 0; k < dim; ++k) v += pl.aff_coef[(size_t)sl * (dim + 1) + 1 + k] * (double)latQ[(size_t)c * dim + k] / q;
            EXPECT(std::fabs(v - sigma[(size_t)e * nq + c]) < 1e-12);
          }
        } else {
          EXPECT(pl.mat_of[(size_t)sl] < pl.nmat);
        }
      }
      EXPECT(naff == pl.naffine);
      if (rq.pre_family) {
        for (int32_t ms : pl.mat_slots) EXPECT(ms >= 0 && ms < pl.nslots && pl.mat_of[(size_t)ms] >= 0);
        EXPECT((int)pl.mat_slots.size() + pl.naffine == (int)std::count_if(pl.slot.begin(), pl.slot.end(), [](int32_t v) { return v >= 0; }));
      }
      if (pl.naffine > 0) {
        EXPECT(pl.X.size() == (size_t)dim * nd * pl.W && pl.col.size() == (size_t)nd * pl.W && pl.item_slots.size() == pl.items.size() * gw);
        // X_k is multiplication by xi_k followed by the L2 projection: it maps the constant 1 to xi_k at the nodes
        std::vector<int> latP;
        lattice_points(dim, degree, latP, kind);
        for (int k = 0; k < dim; ++k)
          for (int a = 0; a < nd; ++a) {
            double row = 0.0, ell = 0.0;
            for (int b = 0; b < nd; ++b) row += pl.Xd[((size_t)k * nd + a) * nd + b];
            for (int j = 0; j < pl.W; ++j) ell += pl.X[((size_t)k * nd + a) * pl.W + j];
            EXPECT(std::fabs(row - (double)latP[(size_t)a * dim + k] / degree) < 1e-10 && std::fabs(row - ell) < 1e-12);
          }
        int seen = 0;
        for (int32_t s : pl.item_slots) seen += s >= 0;
        EXPECT(seen == pl.naffine);
      }
    }
  }
}

// The interleaved layout (hostlogic.hpp Layout) restated without its arithmetic: walk the storage of a field with ncomp
// components in the order it lies in memory - groups of gw cubes, classes, nodes, components, lanes - and count.
struct NaiveLayout {
  std::vector<int64_t> item, lane;   // [cube * ncls + cls]
  std::vector<int64_t> pos;          // [(cube * ncls + cls) * nd + b] -> position of component 0
  std::vector<int64_t> group;        // [cube]
  int64_t nitems = 0, len = 0;       // items, values allocated
  NaiveLayout(int64_t gw, int64_t ncls, int64_t nd, int64_t ncomp, int64_t ncube) {
    int64_t ngroups = 0;
    while (ngroups * gw < ncube) ngroups += 1;
    item.assign((size_t)(ngroups * gw * ncls), -1);
    lane = item;
    pos.assign((size_t)(ngroups * gw * ncls * nd), -1);
    group.assign((size_t)(ngroups * gw), -1);
    for (int64_t g = 0; g < ngroups; ++g)
      for (int64_t k = 0; k < ncls; ++k, ++nitems)
        for (int64_t b = 0; b < nd; ++b)
          for (int64_t c = 0; c < ncomp; ++c)
            for (int64_t w = 0; w < gw; ++w, ++len) {
              const int64_t cube = g * gw + w;
              group[(size_t)cube] = g;
              item[(size_t)(cube * ncls + k)] = nitems;
              lane[(size_t)(cube * ncls + k)] = w;
              if (c == 0) pos[(size_t)((cube * ncls + k) * nd + b)] = len;
            }
  }
};

template <typename F>
static bool throws_invalid(F&& f) {
  try {
    f();
  } catch (const std::invalid_argument&) {
    return true;
  }
  return false;
}

static int classes_of(int dim, int kind) { return kind == KIND_TENSOR || dim == 1 ? 1 : (dim == 2 ? 2 : 6); }

// The host half of sg_set_source / sg_set_source_separable (csrc/source_tables.cpp plan_source) against the definition:
// ragged blocks in every layout, FIRST regions that are empty / partial / everything, node lists with no / some / all
// duplicates and all nodes in one cell, table / static / separable sources, symmetric and non-symmetric values
static void source_plans(int dim, int kind) {
  const int degree = dim == 3 ? 1 : 2, nd = num_nodes(dim, degree, kind), ncls = classes_of(dim, kind), dd = dim * dim;
  const int32_t n[3] = {19, dim > 1 ? 3 : 1, dim > 2 ? 2 : 1};
  const int64_t ncube = (int64_t)n[0] * n[1] * n[2], ncells = ncube * ncls, nscalar = ncells * nd;
  unsigned seed = 777u + (unsigned)(dim * 10 + kind);
  auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return (double)(seed >> 8) / (double)(1u << 24); };
  for (int gw : {1, 16, 64}) {
    const NaiveLayout NL(gw, ncls, nd, dd, ncube);
    SourceRequest rq;
    rq.dim = dim;
    rq.L = Layout{gw, ncls, nd};
    rq.ncells = ncells;
    rq.ncube_pad = (int64_t)NL.group.size();
    std::copy(n, n + 3, rq.n);
    rq.want_fused = true;      // (only the 2-D tile family asks; the table is defined for every layout)
    rq.sym = true;
    // FIRST: of a block with neighbours on no / some / all sides, and the two extremes - no box, the whole block
    for (int first = 0; first < 5; ++first) {
      rq.first.clear();
      if (first < 3) {
        const int mask = first == 0 ? 0 : (first == 1 ? 0x25 & ((1 << (2 * dim)) - 1) : (1 << (2 * dim)) - 1);
        int32_t has_nbr[6];
        for (int s2 = 0; s2 < 6; ++s2) has_nbr[s2] = (mask >> s2) & 1;
        region_boxes(dim, n, has_nbr, SG_REGION_FIRST, rq.first, shell_width_x(gw, n[0], has_nbr[0] != 0, has_nbr[1] != 0));
      } else if (first == 4) {
        rq.first.push_back(Box{{0, 0, 0}, {n[0], n[1], n[2]}});
      }
      std::vector<char> in_first((size_t)ncube, 0);
      for (const Box& b : rq.first)
        for (int ck = b.o[2]; ck < b.o[2] + b.n[2]; ++ck)
          for (int cj = b.o[1]; cj < b.o[1] + b.n[1]; ++cj)
            for (int ci = b.o[0]; ci < b.o[0] + b.n[0]; ++ci) in_first[(size_t)(ci + n[0] * (cj + n[1] * ck))] = 1;
      for (int lists = 0; lists < 4; ++lists)        // 0 no duplicates, 1 some, 2 every node twice or more, 3 all in one cell
        for (int mode = 0; mode < 3; ++mode)          // 0 table of 3 slices, 1 static, 2 separable
          for (int sym = 0; sym < 2; ++sym) {
            const int64_t nnz = lists == 3 ? 3 * nd : 40;
            std::vector<int64_t> nodes;
            const int64_t one_cell = (int64_t)(rnd() * ncells);
            while ((int64_t)nodes.size() < nnz) {
              const size_t have = nodes.size();
              int64_t nx = lists == 3 ? one_cell * nd + (int64_t)(rnd() * nd) : (int64_t)(rnd() * nscalar);
              if (lists == 2 && have >= (size_t)nnz / 2) nx = nodes[have - (size_t)nnz / 2];
              if (lists == 1 && have % 5 == 4) nx = nodes[(size_t)(rnd() * have)];
              const bool seen = std::find(nodes.begin(), nodes.end(), nx) != nodes.end();
              if (seen && (lists == 0 || (lists <= 2 && have < (size_t)nnz / 2 && !(lists == 1 && have % 5 == 4)))) continue;
              nodes.push_back(nx);
            }
            const int64_t nsteps = mode == 0 ? 3 : (mode == 1 ? -1 : 5), nslices = mode == 0 ? 3 : 1;
            std::vector<double> values((size_t)(nslices * nnz * dd)), weights;
            for (int64_t i = 0; i < nslices * nnz; ++i)
              for (int a = 0; a < dim; ++a)
                for (int b = a; b < dim; ++b) {
                  const double v = std::ldexp(rnd() - 0.5, (int)(rnd() * 40) - 20);
                  values[(size_t)(i * dd + a * dim + b)] = v;
                  values[(size_t)(i * dd + b * dim + a)] = (sym || dim == 1 || i != nnz / 2) ? v : v + 1.0;
                }
            if (mode == 2)
              for (int k = 0; k < 5; ++k) weights.push_back(rnd());
            const SourcePlan pl = plan_source(rq, nnz, nodes.data(), nsteps, values.data(), mode == 2 ? weights.data() : nullptr);
            // the nodes: each listed node once, FIRST ones first, in listed order on both sides
            std::map<int64_t, int64_t> first_listed;
            for (int64_t k = nnz - 1; k >= 0; --k) first_listed[NL.pos[(size_t)nodes[(size_t)k]]] = k;
            EXPECT(pl.nnz == (int64_t)first_listed.size() && (int64_t)pl.offs.size() == pl.nnz);
            EXPECT(lists == 0 ? pl.nnz == nnz : pl.nnz < nnz);
            EXPECT(lists != 2 || pl.nnz == nnz / 2);
            EXPECT(pl.is_static == (mode == 1) && pl.nsteps == (mode == 1 ? 1 : nsteps));
            EXPECT(pl.weights == weights && (int64_t)pl.vals.size() == nslices * pl.nnz * dd);
            EXPECT(std::set<int64_t>(pl.offs.begin(), pl.offs.end()).size() == pl.offs.size());
            int64_t nfirst = 0;
            for (const auto& kv : first_listed) {
              int64_t cube = 0;      // the cube of the node at this position: the one whose nodes' positions hold it
              for (int64_t k = 0; k < nnz; ++k)
                if (NL.pos[(size_t)nodes[(size_t)k]] == kv.first) cube = nodes[(size_t)k] / ((int64_t)nd * ncls);
              nfirst += in_first[(size_t)cube];
            }
            EXPECT(pl.nfirst == nfirst);
            EXPECT(first == 3 ? pl.nfirst == 0 : (first == 4 ? pl.nfirst == pl.nnz : true));
            for (int64_t j = 0; j < (int64_t)pl.offs.size(); ++j) {
              const auto it = first_listed.find(pl.offs[(size_t)j]);
              EXPECT(pl.offs[(size_t)j] >= 0 && pl.offs[(size_t)j] + (int64_t)(dd - 1) * gw < NL.len && it != first_listed.end());
              if (it == first_listed.end()) continue;
              EXPECT((in_first[(size_t)(nodes[(size_t)it->second] / ((int64_t)nd * ncls))] != 0) == (j < pl.nfirst));
              if (j > 0 && j != pl.nfirst && first_listed.count(pl.offs[(size_t)j - 1]))
                EXPECT(first_listed[pl.offs[(size_t)j - 1]] < it->second);
            }
            // the values: scattering the plan = adding the caller's entries one by one in the order listed, bit for bit
            bool symmetric = true;
            for (int64_t sl = 0; sl < nslices && (int64_t)pl.vals.size() == nslices * pl.nnz * dd; ++sl) {
              std::vector<double> A((size_t)NL.len, 0.0), B((size_t)NL.len, 0.0);
              for (int64_t j = 0; j < pl.nnz; ++j)
                for (int c = 0; c < dd; ++c) A[(size_t)(pl.offs[(size_t)j] + (int64_t)c * gw)] = pl.vals[(size_t)((sl * pl.nnz + j) * dd + c)];
              for (int64_t k = 0; k < nnz; ++k)
                for (int c = 0; c < dd; ++c) B[(size_t)(NL.pos[(size_t)nodes[(size_t)k]] + (int64_t)c * gw)] += values[(size_t)((sl * nnz + k) * dd + c)];
              EXPECT(A == B);
              for (const auto& kv : first_listed)
                for (int a = 0; a < dim; ++a)
                  for (int b = 0; b < dim; ++b)
                    symmetric = symmetric && B[(size_t)(kv.first + (int64_t)(a * dim + b) * gw)] == B[(size_t)(kv.first + (int64_t)(b * dim + a) * gw)];
            }
            EXPECT(pl.symmetric == symmetric && (sym || dim == 1 || !symmetric));
            // the fused table: every source node is reached through slot / idx exactly once, every other entry is -1
            EXPECT((int64_t)pl.slot.size() == NL.nitems);
            std::vector<int> reached((size_t)pl.nnz, 0);
            std::set<int32_t> slots;
            for (int64_t cell = 0; cell < (int64_t)NL.item.size() && (int64_t)pl.slot.size() == NL.nitems; ++cell) {
              const int32_t sl = pl.slot[(size_t)NL.item[(size_t)cell]];
              if (sl < 0) continue;
              slots.insert(sl);
              EXPECT(((size_t)sl + 1) * nd * gw <= pl.idx.size());
              for (int b = 0; b < nd && ((size_t)sl + 1) * nd * gw <= pl.idx.size(); ++b) {
                const int32_t j = pl.idx[((size_t)sl * nd + b) * gw + (size_t)NL.lane[(size_t)cell]];
                if (j < 0) continue;
                EXPECT(j < pl.nnz && pl.offs[(size_t)j] == NL.pos[(size_t)(cell * nd + b)]);
                if (j < pl.nnz) reached[(size_t)j] += 1;
              }
            }
            EXPECT(std::count(reached.begin(), reached.end(), 1) == pl.nnz);
            EXPECT(pl.idx.size() == slots.size() * nd * gw && (slots.empty() || *slots.rbegin() == (int32_t)slots.size() - 1));
            EXPECT(std::count_if(pl.idx.begin(), pl.idx.end(), [](int32_t v) { return v >= 0; }) == pl.nnz);
            // not wanted: no table; nothing else changes
            SourceRequest plain = rq;
            plain.want_fused = false;
            const SourcePlan p2 = plan_source(plain, nnz, nodes.data(), nsteps, values.data(), mode == 2 ? weights.data() : nullptr);
            EXPECT(p2.slot.empty() && p2.idx.empty() && p2.offs == pl.offs && p2.vals == pl.vals && p2.nfirst == pl.nfirst);
          }
    }
    // no source, and what must be refused
    const int64_t node0[2] = {0, nscalar - 1}, low[1] = {-1}, high[1] = {nscalar};
    const std::vector<double> v((size_t)(2 * 3 * dd), 1.0);
    EXPECT(plan_source(rq, 0, nullptr, 5, nullptr, nullptr).nnz == 0 && plan_source(rq, 2, node0, 0, v.data(), nullptr).nnz == 0);
    EXPECT(plan_source(rq, 0, nullptr, 5, nullptr, nullptr).offs.empty() && plan_source(rq, 0, nullptr, 5, nullptr, nullptr).slot.empty());
    EXPECT(plan_source(rq, 2, node0, 3, v.data(), nullptr).nnz == 2);
    EXPECT(throws_invalid([&] { plan_source(rq, 2, nullptr, 3, v.data(), nullptr); }));
    EXPECT(throws_invalid([&] { plan_source(rq, 2, node0, 3, nullptr, nullptr); }));
    EXPECT(throws_invalid([&] { plan_source(rq, 2, node0, -2, v.data(), nullptr); }));
    EXPECT(throws_invalid([&] { plan_source(rq, -1, node0, 3, v.data(), nullptr); }));
    EXPECT(throws_invalid([&] { plan_source(rq, 2, node0, -1, v.data(), v.data()); }));
    EXPECT(throws_invalid([&] { plan_source(rq, 1, low, 3, v.data(), nullptr); }));
    EXPECT(throws_invalid([&] { plan_source(rq, 1, high, 3, v.data(), nullptr); }));
  }
}

// sg_set_source_box_ricker's host half: box_nodes against testing every node of the block, ricker_weights against the formula
static void box_ricker(int dim, int diagonal, int degree) {
  sg_config cfg;
  std::memset(&cfg, 0, sizeof(cfg));
  cfg.dim = dim;
  cfg.degree = degree;
  cfg.diagonal = diagonal;
  const int nn[3] = {5, 3, 2};
  for (int a = 0; a < 3; ++a) {
    cfg.n[a] = a < dim ? nn[a] : 1;
    cfg.h[a] = a < dim ? 0.25 * (a + 1) : 1.0;
    cfg.origin[a] = a < dim ? -0.5 + a : 0.0;
    cfg.cube0[a] = a < dim ? 2 - a : 0;
  }
  NodeGeom G;
  EXPECT(G.init(&cfg, degree));
  const size_t nnodes = (size_t)cfg.n[0] * cfg.n[1] * cfg.n[2] * G.ncls * G.nq;
  std::vector<double> X(nnodes * dim);
  EXPECT(sg_block_node_coords(&cfg, degree, X.data(), X.size() * sizeof(double)) == SG_OK);
  unsigned seed = 4242u + (unsigned)(dim * 100 + diagonal * 10 + degree);
  auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return (double)(seed >> 8) / (double)(1u << 24); };
  for (int trial = 0; trial < 40; ++trial) {
    // boxes inside, across the block's sides, outside, around the whole block; planes through grid lines (lo = hi)
    double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    for (int a = 0; a < dim; ++a) {
      const double x0 = cfg.origin[a] + cfg.cube0[a] * cfg.h[a], len = cfg.n[a] * cfg.h[a];
      lo[a] = x0 + (rnd() * 2.0 - 0.5) * len;
      hi[a] = lo[a] + rnd() * len;
      if (trial % 4 == 1) lo[a] = hi[a] = x0 + (int)(rnd() * (cfg.n[a] + 1)) * cfg.h[a];
      if (trial % 4 == 2 && a == 0) lo[a] = x0 - 10.0, hi[a] = x0 + len + 10.0;
      if (trial == 3) lo[a] = x0 + 2 * len, hi[a] = x0 + 3 * len;
    }
    std::vector<int64_t> want;
    for (size_t k = 0; k < nnodes; ++k) {
      bool in = true;
      for (int a = 0; a < dim; ++a) in = in && X[k * dim + a] >= lo[a] && X[k * dim + a] <= hi[a];
      if (in) want.push_back((int64_t)k);
    }
    EXPECT(box_nodes(G, lo, hi) == want);
    if (trial == 3) EXPECT(want.empty());
  }
  const double lo[3] = {0.5, 0.5, 0.5}, hi[3] = {0.4, 0.6, 0.6}, nan[3] = {std::nan(""), 0.0, 0.0};
  EXPECT(throws_invalid([&] { box_nodes(G, lo, hi); }));
  EXPECT(throws_invalid([&] { box_nodes(G, nan, lo); }));
  const double a = 159.42, t0 = 0.3, tf = 1.25e-3, dts = 2.5e-3;
  const std::vector<double> w = ricker_weights(a, t0, tf, dts, 300);
  EXPECT(w.size() == 300);
  for (size_t k = 0; k < w.size(); ++k) {
    const double dt_ = tf + (double)k * dts - t0, want = (2.0 * a * dt_ * dt_ - 1.0) * std::exp(-a * dt_ * dt_);
    EXPECT(std::fabs(w[k] - want) <= 1e-13 * std::fmax(1.0, std::fabs(want)));
  }
  EXPECT(ricker_weights(a, t0, tf, dts, 0).empty());
}

// sg_set_receivers' and sg_set_gauges' host halves (hostapi.cpp plan_receivers, plan_gauges) on the split of point_location(): the rows are the points that
// locate_point gives the block, in order; item and lane are the owning cell's in every layout; phi is the basis at the point
static void receiver_plans(int dim, int diagonal, int degree) {
  const int kind = diagonal == SG_DIAGONAL_QUAD ? KIND_TENSOR : KIND_SIMPLEX, nd = num_nodes(dim, degree, kind), ncls = classes_of(dim, kind);
  sg_config whole;
  std::memset(&whole, 0, sizeof(whole));
  whole.dim = dim;
  whole.degree = degree;
  whole.diagonal = diagonal;
  for (int a = 0; a < 3; ++a) {
    whole.n[a] = a < dim ? 4 : 1;
    whole.h[a] = a < dim ? 0.25 * (a + 1) : 1.0;
  }
  std::vector<double> pts;
  const double fr[] = {0.0, 0.5, 0.3};
  for (int cz = (dim > 2 ? -1 : 0); cz <= (dim > 2 ? 4 : 0); ++cz)
    for (int cy = (dim > 1 ? -1 : 0); cy <= (dim > 1 ? 4 : 0); ++cy)
      for (int cx = -1; cx <= 4; ++cx)
        for (int f = 0; f < 3; ++f) {
          const int c[3] = {cx, cy, cz};
          for (int a = 0; a < dim; ++a) pts.push_back((c[a] + (a == 1 ? 1.0 - fr[f] : fr[f])) * whole.h[a]);
        }
  const int64_t np = (int64_t)pts.size() / dim;
  std::vector<int64_t> cell(np);
  std::vector<double> xi(pts.size());
  std::vector<int> owners(np, 0);
  for (int b = 0; b < (1 << dim); ++b) {
    sg_config blk = whole;
    for (int a = 0; a < dim; ++a) {
      const int hi = (b >> a) & 1;
      blk.n[a] = 2;
      blk.cube0[a] = 2 * hi;
      blk.nbr_mask |= 1 << (2 * a + (1 - hi));
    }
    NodeGeom G;
    EXPECT(G.init(&blk, degree));
    EXPECT(sg_locate_points(&blk, np, pts.data(), cell.data(), xi.data()) == SG_OK);
    const int64_t ncube = 1 << dim;
    for (int gw : {1, 16, 64})
      for (int what = 1; what <= 3; ++what) {
        const NaiveLayout NL(gw, ncls, nd, 1, ncube);
        const ReceiverPlan pl = plan_receivers(G, Layout{gw, ncls, nd}, kind, np, pts.data(), what, 7);
        EXPECT(pl.ncomp == (what == 1 ? dim : (what == 2 ? dim * dim : dim + dim * dim)));
        EXPECT((int64_t)pl.own.size() == np && pl.item.size() == pl.row.size() && pl.lane.size() == pl.row.size() && pl.phi.size() == pl.row.size() * nd);
        size_t r = 0;
        for (int64_t k = 0; k < np && (int64_t)pl.own.size() == np; ++k) {
          EXPECT((pl.own[(size_t)k] != 0) == (cell[(size_t)k] >= 0));
          if (cell[(size_t)k] < 0) continue;
          if (gw == 1 && what == 1) owners[(size_t)k] += 1;
          EXPECT(r < pl.row.size() && pl.row[r] == k);
          if (r >= pl.row.size() || pl.phi.size() != pl.row.size() * nd) break;
          EXPECT(pl.item[r] == NL.item[(size_t)cell[(size_t)k]] && pl.lane[r] == NL.lane[(size_t)cell[(size_t)k]]);
          std::vector<double> phi((size_t)nd);
          EXPECT(sg_tabulate_cell(kind, dim, degree, 1, &xi[(size_t)k * dim], phi.data()) == SG_OK);
          double sum = 0.0;
          for (int a = 0; a < nd; ++a) {
            EXPECT(pl.phi[r * nd + a] == phi[(size_t)a]);
            sum += phi[(size_t)a];
          }
          EXPECT(std::fabs(sum - 1.0) < 1e-9);
          r += 1;
        }
        EXPECT(r == pl.row.size());
        // a trace of more than 2^40 values is refused - where the block owns a receiver at all
        EXPECT(throws_invalid([&] { plan_receivers(G, Layout{gw, ncls, nd}, kind, np, pts.data(), what, ((int64_t)1 << 40) + 1); }) == !pl.row.empty());
      }
    // sg_set_gauges' host half (hostapi.cpp plan_gauges) on the same points: the same rows, items and lanes, the cell's class,
    // and D = sg_gauge_weights' rows = the tabulated derivative at the point, transposed
    std::vector<int64_t> gcell(np);
    std::vector<double> gD((size_t)np * dim * nd);
    EXPECT(sg_gauge_weights(&blk, np, pts.data(), gcell.data(), gD.data()) == nd);
    for (int gw : {1, 16, 64})
      for (int gkind = 0; gkind < 4; ++gkind) {
        if (grad_ncomp(dim, gkind) == 0) continue;
        const NaiveLayout NL(gw, ncls, nd, 1, ncube);
        const GaugePlan pl = plan_gauges(G, Layout{gw, ncls, nd}, kind, np, pts.data(), gkind, 7);
        EXPECT(pl.ncomp == grad_ncomp(dim, gkind));
        EXPECT((int64_t)pl.own.size() == np && pl.item.size() == pl.row.size() && pl.lane.size() == pl.row.size() &&
               pl.cls.size() == pl.row.size() && pl.D.size() == pl.row.size() * dim * nd);
        size_t r = 0;
        for (int64_t k = 0; k < np && (int64_t)pl.own.size() == np; ++k) {
          EXPECT((pl.own[(size_t)k] != 0) == (cell[(size_t)k] >= 0) && gcell[(size_t)k] == cell[(size_t)k]);
          if (cell[(size_t)k] < 0) continue;
          EXPECT(r < pl.row.size() && pl.row[r] == k);
          if (r >= pl.row.size() || pl.D.size() != pl.row.size() * dim * nd) break;
          EXPECT(pl.item[r] == NL.item[(size_t)cell[(size_t)k]] && pl.lane[r] == NL.lane[(size_t)cell[(size_t)k]]);
          EXPECT(pl.cls[r] == (int32_t)(cell[(size_t)k] % ncls));
          std::vector<double> dphi((size_t)nd * dim);
          EXPECT(sg_tabulate_grad_cell(kind, dim, degree, 1, &xi[(size_t)k * dim], dphi.data()) == SG_OK);
          for (int rr = 0; rr < dim; ++rr) {
            double sum = 0.0;
            for (int a = 0; a < nd; ++a) {
              EXPECT(pl.D[(r * dim + rr) * nd + a] == dphi[(size_t)a * dim + rr]);
              EXPECT(gD[((size_t)k * dim + rr) * nd + a] == dphi[(size_t)a * dim + rr]);
              sum += dphi[(size_t)a * dim + rr];
            }
            EXPECT(std::fabs(sum) < 1e-9);     // the derivative of a partition of unity
          }
          r += 1;
        }
        EXPECT(r == pl.row.size());
        EXPECT(throws_invalid([&] { plan_gauges(G, Layout{gw, ncls, nd}, kind, np, pts.data(), gkind, ((int64_t)1 << 40) + 1); }) == !pl.row.empty());
      }
    const double far[3] = {-5.0, -5.0, -5.0};
    EXPECT(plan_gauges(G, Layout{16, ncls, nd}, kind, 1, far, 3, ((int64_t)1 << 40) + 1).row.empty());
    EXPECT(plan_gauges(G, Layout{16, ncls, nd}, kind, 0, nullptr, 3, 0).own.empty());
    EXPECT(plan_receivers(G, Layout{16, ncls, nd}, kind, 1, far, 3, ((int64_t)1 << 40) + 1).row.empty());
    EXPECT(plan_receivers(G, Layout{16, ncls, nd}, kind, 0, nullptr, 3, 0).own.empty());
  }
  std::vector<int64_t> cell1(np);
  EXPECT(sg_locate_points(&whole, np, pts.data(), cell1.data(), xi.data()) == SG_OK);
  for (int64_t k = 0; k < np; ++k) EXPECT(owners[(size_t)k] == (cell1[(size_t)k] >= 0 ? 1 : 0));
}

// The injectors' host half (hostapi.cpp injector_plan, injector_gather, injector_symmetric; hostlogic.hpp StepClock) on
// the split of receiver_plans(), every point listed twice more so that cells hold several points in interleaved order: the
// owners are locate_point's, the groups are the cells in ascending order, a cell's rows keep the order given (the order of
// the kernel's sum), item and lane are the cell's in every layout, psi is sg_injector_weights' and has the delta property
static void injector_plans(int dim, int diagonal, int degree) {
  const int kind = diagonal == SG_DIAGONAL_QUAD ? KIND_TENSOR : KIND_SIMPLEX, nd = num_nodes(dim, degree, kind), ncls = classes_of(dim, kind);
  const RefElem re = make_refelem(dim, degree, kind);
  sg_config whole;
  std::memset(&whole, 0, sizeof(whole));
  whole.dim = dim;
  whole.degree = degree;
  whole.diagonal = diagonal;
  for (int a = 0; a < 3; ++a) {
    whole.n[a] = a < dim ? 4 : 1;
    whole.h[a] = a < dim ? 0.25 * (a + 1) : 1.0;
  }
  std::vector<double> once, pts;
  const double fr[] = {0.0, 0.5, 0.3};
  for (int cz = (dim > 2 ? -1 : 0); cz <= (dim > 2 ? 4 : 0); ++cz)
    for (int cy = (dim > 1 ? -1 : 0); cy <= (dim > 1 ? 4 : 0); ++cy)
      for (int cx = -1; cx <= 4; ++cx)
        for (int f = 0; f < 3; ++f) {
          const int c[3] = {cx, cy, cz};
          for (int a = 0; a < dim; ++a) once.push_back((c[a] + (a == 1 ? 1.0 - fr[f] : fr[f])) * whole.h[a]);
        }
  // descending, ascending, descending: the same point comes back far from its first listing
  const int64_t n1 = (int64_t)once.size() / dim;
  for (int rep = 0; rep < 3; ++rep)
    for (int64_t k = 0; k < n1; ++k) {
      const int64_t src = rep == 1 ? k : n1 - 1 - k;
      for (int a = 0; a < dim; ++a) pts.push_back(once[(size_t)src * dim + a]);
    }
  const int64_t np = 3 * n1;
  double detj = 1.0;
  for (int a = 0; a < dim; ++a) detj *= whole.h[a];
  std::vector<double> Mone((size_t)nd, 0.0);     // |det J| Mhat 1: the functional of v = 1
  for (int a = 0; a < nd; ++a)
    for (int b = 0; b < nd; ++b) Mone[(size_t)a] += detj * re.Mhat[(size_t)a * nd + b];
  std::vector<int64_t> cell(np), wcell(np);
  std::vector<double> xi(pts.size()), wpsi((size_t)np * nd), bpsi((size_t)np * nd);
  EXPECT(sg_injector_weights(&whole, np, pts.data(), wcell.data(), wpsi.data()) == SG_OK);
  std::vector<int> owners(np, 0);
  for (int b = 0; b < (1 << dim); ++b) {
    sg_config blk = whole;
    for (int a = 0; a < dim; ++a) {
      const int hi = (b >> a) & 1;
      blk.n[a] = 2;
      blk.cube0[a] = 2 * hi;
      blk.nbr_mask |= 1 << (2 * a + (1 - hi));
    }
    NodeGeom G;
    EXPECT(G.init(&blk, degree));
    EXPECT(sg_locate_points(&blk, np, pts.data(), cell.data(), xi.data()) == SG_OK);
    std::vector<int64_t> icell(np);
    EXPECT(sg_injector_weights(&blk, np, pts.data(), icell.data(), bpsi.data()) == SG_OK);
    EXPECT(icell == cell);
    const int64_t ncube = 1 << dim;
    for (int gw : {1, 16, 64})
      for (int what = 1; what <= 3; ++what) {
        const NaiveLayout NL(gw, ncls, nd, 1, ncube);
        const InjectorPlan pl = injector_plan(G, Layout{gw, ncls, nd}, re, np, pts.data(), what);
        EXPECT(pl.ncomp == (what == 1 ? dim : (what == 2 ? dim * dim : dim + dim * dim)));
        const size_t ng = pl.cell.size();
        EXPECT((int64_t)pl.own.size() == np && pl.item.size() == ng && pl.lane.size() == ng && pl.start.size() == ng + 1 &&
               pl.psi.size() == pl.row.size() * nd);
        if ((int64_t)pl.own.size() != np || pl.start.size() != ng + 1 || pl.psi.size() != pl.row.size() * nd) continue;
        int64_t nown = 0;
        for (int64_t k = 0; k < np; ++k) {
          EXPECT((pl.own[(size_t)k] != 0) == (cell[(size_t)k] >= 0));
          nown += cell[(size_t)k] >= 0 ? 1 : 0;
          if (gw == 1 && what == 1 && cell[(size_t)k] >= 0) owners[(size_t)k] += 1;
        }
        EXPECT((int64_t)pl.row.size() == nown && pl.start.front() == 0 && pl.start.back() == nown);
        for (size_t g = 0; g < ng; ++g) {
          EXPECT(g == 0 || pl.cell[g - 1] < pl.cell[g]);
          EXPECT(pl.start[g] < pl.start[g + 1]);
          EXPECT(pl.item[g] == NL.item[(size_t)pl.cell[g]] && pl.lane[g] == NL.lane[(size_t)pl.cell[g]]);
          for (int64_t r = pl.start[g]; r < pl.start[g + 1] && r < nown; ++r) {
            const int64_t k = pl.row[(size_t)r];
            EXPECT(k >= 0 && k < np && cell[(size_t)k] == pl.cell[g]);
            EXPECT(r == pl.start[g] || pl.row[(size_t)r - 1] < k);      // stable: the order given
            if (k < 0 || k >= np) continue;
            double one = 0.0;
            for (int a = 0; a < nd; ++a) {
              EXPECT(pl.psi[(size_t)r * nd + a] == bpsi[(size_t)k * nd + a] && bpsi[(size_t)k * nd + a] == wpsi[(size_t)k * nd + a]);
              one += pl.psi[(size_t)r * nd + a] * Mone[(size_t)a];
            }
            EXPECT(std::fabs(one - 1.0) < 1e-10);
          }
        }
        // the caller's table in the order of the rows; symmetric only where every owned stress entry is, to the bit
        const int64_t nsteps = 2;
        std::vector<double> amp((size_t)(nsteps * np * pl.ncomp));
        for (size_t i = 0; i < amp.size(); ++i) amp[i] = 1.0 + (double)i;
        const int off = (what & 1) ? dim : 0;
        if (what & 2)
          for (int64_t e = 0; e < nsteps * np; ++e)
            for (int i = 0; i < dim; ++i)
              for (int j = 0; j < i; ++j) amp[(size_t)(e * pl.ncomp + off + i * dim + j)] = amp[(size_t)(e * pl.ncomp + off + j * dim + i)];
        std::vector<double> t = injector_gather(pl, np, nsteps, amp.data());
        EXPECT(t.size() == (size_t)(nsteps * nown * pl.ncomp));
        for (int64_t s2 = 0; s2 < nsteps; ++s2)
          for (int64_t r = 0; r < nown; ++r)
            for (int q = 0; q < pl.ncomp; ++q)
              EXPECT(t[(size_t)((s2 * nown + r) * pl.ncomp + q)] == amp[(size_t)((s2 * np + pl.row[(size_t)r]) * pl.ncomp + q)]);
        EXPECT(injector_symmetric(pl, dim, what, nsteps, t));
        if ((what & 2) && dim > 1 && nown > 0) {
          t[(size_t)((nsteps * nown - 1) * pl.ncomp + off + 1)] += 1.0;      // entry (0, 1) of the last owned point, last step
          EXPECT(!injector_symmetric(pl, dim, what, nsteps, t));
        }
      }
    const double far[3] = {-5.0, -5.0, -5.0};
    const InjectorPlan none = injector_plan(G, Layout{16, ncls, nd}, re, 1, far, 3);
    EXPECT(none.row.empty() && none.cell.empty() && none.start.size() == 1 && none.own.size() == 1 && none.own[0] == 0);
    EXPECT(injector_plan(G, Layout{16, ncls, nd}, re, 0, nullptr, 3).own.empty());
  }
  for (int64_t k = 0; k < np; ++k) EXPECT(owners[(size_t)k] == (wcell[(size_t)k] >= 0 ? 1 : 0));
  // the clock: entry k at the end of step k + 1, nothing after nsteps
  StepClock c;   // every = 1
  c.count = 3;
  EXPECT(!c.due_at(0) && c.due_at(1) && c.due_at(3) && !c.due_at(4) && c.active());
  c.steps = 3;
  EXPECT(!c.active());
  EXPECT(sg_injector_weights(&whole, 1, nullptr, nullptr, nullptr) == SG_ERR_ARG);
  EXPECT(sg_injector_weights(nullptr, 0, nullptr, nullptr, nullptr) == SG_ERR_ARG);
}

// The items of the regions of a split stage (hostapi.cpp region_items) against a per-cube brute force, on the ragged block
// and the neighbour masks of regions_and_coords(), in every layout
static void region_item_lists() {
  for (int dim = 1; dim <= 3; ++dim)
    for (int ncls : {1, dim == 1 ? 1 : (dim == 2 ? 2 : 6)})
      for (int gw : {1, 16, 64})
        for (int mask = 0; mask < (1 << (2 * dim)); mask += (dim == 3 ? 7 : 1)) {
          const int32_t n[3] = {19, dim > 1 ? 5 : 1, dim > 2 ? 4 : 1};
          int32_t has_nbr[6];
          for (int s2 = 0; s2 < 6; ++s2) has_nbr[s2] = (mask >> s2) & 1;
          const int64_t ncube = (int64_t)n[0] * n[1] * n[2];
          const NaiveLayout NL(gw, ncls, 1, 1, ncube);
          const int64_t ngroups = NL.nitems / ncls;
          for (int region = 0; region <= 4; ++region) {
            std::vector<Box> boxes;
            region_boxes(dim, n, has_nbr, region, boxes, shell_width_x(gw, n[0], has_nbr[0] != 0, has_nbr[1] != 0));
            const RegionItems got = region_items(boxes, n, Layout{gw, ncls, 1}, ncube, (int64_t)NL.group.size());
            std::vector<int> hit((size_t)ngroups, 0), real((size_t)ngroups, 0);
            int64_t cube = 0;
            for (int ck = 0; ck < n[2]; ++ck)
              for (int cj = 0; cj < n[1]; ++cj)
                for (int ci = 0; ci < n[0]; ++ci, ++cube) {
                  const int c[3] = {ci, cj, ck};
                  int inside = 0;
                  for (const Box& b : boxes) {
                    bool in = true;
                    for (int a = 0; a < 3; ++a) in = in && c[a] >= b.o[a] && c[a] < b.o[a] + b.n[a];
                    inside += in;
                  }
                  EXPECT(inside <= 1);      // the boxes of a region are disjoint
                  real[(size_t)NL.group[(size_t)cube]] += 1;
                  hit[(size_t)NL.group[(size_t)cube]] += inside;
                }
            std::vector<int32_t> items;
            bool whole = true;
            for (int64_t g = 0; g < ngroups; ++g) {
              if (hit[(size_t)g] == 0) continue;
              whole = whole && hit[(size_t)g] == real[(size_t)g];
              for (int k = 0; k < ncls; ++k) items.push_back((int32_t)NL.item[(size_t)(g * gw * ncls + k)]);
            }
            EXPECT(got.items == items && got.whole == whole);
            if (region == SG_REGION_ALL) EXPECT(got.whole && (int64_t)got.items.size() == NL.nitems);
          }
        }
  const int32_t n1[3] = {4, 1, 1};
  EXPECT(region_items({}, n1, Layout{16, 2, 1}, 4, 16).items.empty() && region_items({}, n1, Layout{16, 2, 1}, 4, 16).whole);
}

// SEIGEN_HIP_GRID_BLOCKS as a grid (hostlogic.hpp grid_blocks_override) and as the cap of the affine pre-pass's grid
// (affine_grid_cap): min(prepared, max(8, value / 8 * 8)) - it shrinks, never enlarges
static void grid_overrides() {
  const int in[] = {-5, 0, 1, 7, 8, 9, 15, 16, 17, 255, 256, 480, 511, 512, 100000};
  const int out[] = {8, 8, 8, 8, 8, 8, 8, 16, 16, 248, 256, 480, 504, 512, 100000};
  for (size_t k = 0; k < sizeof(in) / sizeof(in[0]); ++k) {
    EXPECT(grid_blocks_override(in[k]) == out[k]);
    for (int prepared : {1, 7, 8, 9, 256, 512, 1024}) {
      const int got = affine_grid_cap(prepared, in[k]);
      EXPECT(got == std::min(prepared, std::max(8, in[k] / 8 * 8)));
      EXPECT(got <= prepared && got >= std::min(prepared, 8));
    }
  }
  EXPECT(affine_grid_cap(1024, 8) == 8 && affine_grid_cap(512, 8) == 8 && affine_grid_cap(4, 8) == 4 && affine_grid_cap(1024, 4096) == 1024);
}

// The six launches of an LF4 step (hostlogic.hpp lf4_stage) against the rows written out here, for two (dt, rho) and the
// three density conventions of stage U1; every stage reads what the stage before it wrote, cyclically over the step.
// The printed lines are what tests/test_host_logic.py compares with seigen_amd/parallel.py STAGE_INPUT / STAGE_OUTPUT.
static void stage_table() {
  const int U = SG_FIELD_U, UH = SG_FIELD_UH, S = SG_FIELD_S, SH = SG_FIELD_SH;
  const double pairs[2][2] = {{1e-3, 1.0}, {0.25, 2.5}};
  for (const auto& p : pairs)
    for (int conv = 0; conv < 3; ++conv) {   // 0: rho u0 + ..., 1: u0 + (...) / rho (physical), 2: per-cell factors
      const double dt = p[0], rho = p[1], c3 = dt * dt * dt / 24.0;
      const double u_self = conv == 0 ? rho : 1.0, u_div = conv == 1 ? rho : 1.0;
      const StageOp want[6] = {
          // kind in out aux uabs mode c_self c_aux c_new with_source src_coef density
          {0, S, UH, -1, U, 0, 0.0, 0.0, 0.0, false, 1.0, false},
          {1, UH, SH, -1, U, 0, 0.0, 0.0, 0.0, true, 1.0, false},
          {0, SH, U, UH, U, 1, u_self, dt / u_div, c3 / u_div, false, 1.0, conv == 2},
          {1, U, SH, -1, U, 0, 0.0, 0.0, 0.0, true, 1.0, false},
          {0, SH, UH, U, U, 2, 0.0, dt, c3, false, 1.0, false},
          {1, UH, S, -1, U, 1, 1.0, 0.0, 1.0, true, dt + c3, false},
      };
      for (int k = 0; k < 6; ++k) {
        // (per-cell density wins over the physical flag, as the handle's rho2 table does)
        const StageOp got = lf4_stage(k, dt, rho, conv == 1, conv == 2), &w = want[k];
        EXPECT(got.kind == w.kind && got.in == w.in && got.out == w.out && got.aux == w.aux && got.uabs == w.uabs);
        EXPECT(got.mode == w.mode && got.c_self == w.c_self && got.c_aux == w.c_aux && got.c_new == w.c_new);
        EXPECT(got.with_source == w.with_source && got.src_coef == w.src_coef && got.density == w.density);
        EXPECT(lf4_stage_input(k) == w.in && lf4_stage_output(k) == w.out);
        EXPECT(lf4_stage_output(k) == lf4_stage_input((k + 1) % 6));
      }
    }
  EXPECT(lf4_stage(2, 0.25, 2.5, true, true).density && lf4_stage(2, 0.25, 2.5, true, true).c_aux == 0.25);
  EXPECT(lf4_stage(6, 1e-3, 1.0, false, false).kind == -1 && lf4_stage(-1, 1e-3, 1.0, false, false).kind == -1);
  for (int k = 0; k < 6; ++k) std::printf("stage %d: %d %d\n", k, lf4_stage_input(k), lf4_stage_output(k));
}

// What stepping remembers between calls (hostlogic.hpp FieldVersions, PrePass, source_slice, StepClock), against models
// written out here that share nothing with them.
//
// The pre-pass: the model gives every field a content id, raised whenever a launch or an upload writes the field, and tags the
// pre-pass buffer with the (field, content id) it was computed from.  A launch is described by the caller as the driver of a
// real run would know it: the op, the region, and whether it is the first launch of a stage instance.
struct PrePassModel {
  FieldVersions fv;     // the values under test ...
  PrePass pp;
  int content[4] = {0, 0, 0, 0};   // ... and the model
  int tag_field = -1, tag_id = -1;           // what the buffer holds (-1: nothing known)
  int want_field = -1, want_id = -1;         // what the running F stage must find in it
  int passes = 0;

  void launch(const StageOp& op, int region, bool first_of_instance) {
    const bool due = pp.due(op, region, fv);
    if (op.kind == 0) {
      if (first_of_instance) {
        want_field = op.uabs;
        want_id = content[op.uabs];
      }
      // the model's rule: compute at the first launch of an instance, unless the buffer holds exactly that state
      EXPECT(due == (first_of_instance && !(tag_field == want_field && tag_id == want_id)));
      if (due) {
        passes += 1;
        tag_field = op.uabs;
        tag_id = content[op.uabs];
      }
      EXPECT(tag_field == want_field && tag_id == want_id);   // (a): every region of the stage reads the state of its first
    } else {
      EXPECT(!due);
    }
    fv.written(op.out);      // the launch writes its output: after the decision, as stages.cpp run_op takes the pointer
    content[op.out] += 1;
  }
  void upload(int f) {
    fv.written(f);
    content[f] += 1;
  }
  void forget() {
    pp.forget();
    tag_field = tag_id = -1;
  }
  // one LF4 step under a region schedule (0: whole block, 1: FIRST + SECOND, 2: INTERIOR + BOUNDARY); the pre-passes it ran
  int step(int schedule) {
    const int regions[3][2] = {{SG_REGION_ALL, -1}, {SG_REGION_FIRST, SG_REGION_SECOND}, {SG_REGION_INTERIOR, SG_REGION_BOUNDARY}};
    const int before = passes;
    for (int st = 0; st < 6; ++st) {
      const StageOp op = lf4_stage(st, 1e-3, 1.0, false, false);
      for (int r = 0; r < 2; ++r)
        if (regions[schedule][r] >= 0) launch(op, regions[schedule][r], r == 0);
    }
    return passes - before;
  }
  // n captured steps: the capture forgets, walks the launch code (which counts writes although nothing runs), forgets again
  int capture(int n) {
    forget();
    int total = 0;
    for (int k = 0; k < n; ++k) total += step(0);
    forget();
    return total;
  }
  void replay() {    // whatever the graphs ran wrote all four fields; the model: new content everywhere, the buffer unknown
    fv.replayed();
    for (int& c : content) c += 1;
    forget();
  }
};

static void stepping_state() {
  const int U = SG_FIELD_U, UH = SG_FIELD_UH, S = SG_FIELD_S, SH = SG_FIELD_SH;
  // (b) two pre-passes in a handle's first step, one in every later step, under every region schedule
  for (int schedule = 0; schedule < 3; ++schedule) {
    PrePassModel m;
    const int first = m.step(schedule);
    EXPECT(first == 2);
    for (int k = 0; k < 3; ++k) EXPECT(m.step(schedule) == 1);
    // (c) what makes the next step compute UH1's pre-pass again: a new U, not a new stress; a forgotten buffer; a replay
    m.upload(U);
    EXPECT(m.step(schedule) == 2);
    m.upload(S);
    EXPECT(m.step(schedule) == 1);
    m.upload(SH);
    EXPECT(m.step(schedule) == 1);
    m.upload(UH);     // (UTEMP overwrites it before anything absorbs it)
    EXPECT(m.step(schedule) == 1);
    m.forget();
    EXPECT(m.step(schedule) == 2);
    for (int n : {1, 2, 8, 11}) {
      m.replay();
      (void)n;        // (however many steps the replay ran: the host saw none of their launches)
      EXPECT(m.step(schedule) == 2);
      EXPECT(m.step(schedule) == 1);
    }
    // the graphs of one and of eight steps, captured between eager steps; the step after them starts afresh
    EXPECT(m.capture(1) == 2);
    EXPECT(m.capture(8) == 9);
    EXPECT(m.step(schedule) == 2);
    EXPECT(m.step(schedule) == 1);
    // the schedules mixed from step to step: a stage's regions change, the field states do not
    for (int k = 0; k < 6; ++k) EXPECT(m.step((schedule + k) % 3) == 1);
  }
  // the order run_op keeps - decide, then count the output as written - is what (a) rests on for the in-place stage U1:
  // counted first, U1's pre-pass of u0 would pass for one of the u1 it writes, and UTEMP would absorb the step before
  {
    FieldVersions fv;
    PrePass pp;
    const StageOp u1 = lf4_stage(2, 1e-3, 1.0, false, false), utemp = lf4_stage(4, 1e-3, 1.0, false, false);
    fv.written(u1.out);
    EXPECT(pp.due(u1, SG_REGION_ALL, fv) && !pp.due(utemp, SG_REGION_ALL, fv));
  }
  // un-fused F applications (sg_apply_F) absorbing U and UH in turn, G applications and stage launches between them
  {
    PrePassModel m;
    const StageOp f_u{0, S, UH, -1, U}, f_uh{0, SH, U, -1, UH}, g{1, UH, S}, g2{1, U, SH};
    m.launch(f_u, SG_REGION_ALL, true);
    m.launch(f_u, SG_REGION_ALL, true);       // the same application again: the buffer holds it
    EXPECT(m.passes == 1);
    m.launch(g, SG_REGION_ALL, true);
    m.launch(f_uh, SG_REGION_ALL, true);      // absorbs UH, which f_u wrote; writes U
    EXPECT(m.passes == 2);
    m.launch(f_u, SG_REGION_ALL, true);       // U is new
    EXPECT(m.passes == 3);
    m.launch(f_uh, SG_REGION_ALL, true);      // ... and so is UH
    m.launch(g2, SG_REGION_ALL, true);
    m.launch(f_uh, SG_REGION_FIRST, true);    // UH untouched since: the buffer holds it
    EXPECT(m.passes == 4);
    m.launch(f_uh, SG_REGION_SECOND, false);
    m.launch(f_uh, SG_REGION_FIRST, true);    // a region seen before: the next instance, same state of UH
    m.launch(f_u, SG_REGION_INTERIOR, true);
    m.launch(f_u, SG_REGION_BOUNDARY, false);
    EXPECT(m.step(0) == 1 && m.step(2) == 1);   // U has not moved since f_u absorbed it
    m.launch(f_uh, SG_REGION_ALL, true);
    EXPECT(m.step(0) == 2);                   // f_uh wrote U and left its own pre-pass behind
  }
  // a new state of the absorbed field between two instances of ONE stage: a region seen before, or the whole block after
  // some regions, opens the next instance; and equal write counts of two fields are not the same state
  {
    PrePassModel m;
    const StageOp f_u{0, S, UH, -1, U}, f_uh{0, S, U, -1, UH};
    m.launch(f_u, SG_REGION_FIRST, true);
    m.upload(U);
    m.launch(f_u, SG_REGION_FIRST, true);
    EXPECT(m.passes == 2);
    m.launch(f_u, SG_REGION_INTERIOR, true);
    m.launch(f_u, SG_REGION_BOUNDARY, false);
    m.upload(U);
    m.launch(f_u, SG_REGION_ALL, true);
    EXPECT(m.passes == 3);
    PrePassModel e;
    e.upload(UH);
    e.launch(f_uh, SG_REGION_ALL, true);     // absorbs UH after its one write, writes U once
    e.launch(f_u, SG_REGION_ALL, true);      // absorbs U after its one write
    EXPECT(e.passes == 2 && e.fv.v[U] == 1);
  }
  // G stages never ask, and a PrePass that has seen nothing asks at the first F launch
  {
    FieldVersions fv;
    PrePass pp;
    EXPECT(!pp.due(StageOp{1, U, S}, SG_REGION_ALL, fv));
    EXPECT(pp.due(StageOp{0, S, UH, -1, U}, SG_REGION_ALL, fv));
  }

  // The source (seigen_hip.h sg_set_source, sg_set_source_separable): entry i of step k < nsteps adds values[k][i][dim * dim]
  // of a table, weights[k] * pattern[i][dim * dim] of a separable source, values[0][i] at every step of a static one; nothing
  // afterwards.  A capture made while the source is active hands slice and weight to the device (offset 0, scale 1, the
  // strides and flags of kernels.hpp SrcStep); one made after it ran out holds no source launch.
  for (int dim = 1; dim <= 3; ++dim)
    for (int64_t nnz : {1, 5})
      for (int64_t nsteps : {1, 3})
        for (int form = 0; form < 3; ++form) {    // 0: table, 1: static, 2: separable
          const std::vector<double> w = {0.5, -2.0, 4.0};
          SourceFacts s;
          s.nnz = nnz;
          s.nsteps = form == 1 ? 1 : nsteps;      // (source_tables.cpp plan_source: a static source has one slice)
          s.is_static = form == 1;
          s.weights = form == 2 ? w.data() : nullptr;
          s.dim = dim;
          for (int64_t k = 0; k <= nsteps + 1; ++k) {
            const bool runs = form == 1 || k < nsteps;
            const SourceSlice e = source_slice(s, k, false);
            EXPECT(e.active == runs && e.due == runs);
            if (runs) {
              EXPECT(e.offset == (form == 0 ? k * nnz * dim * dim : 0));
              EXPECT(e.scale == (form == 2 ? w[(size_t)k] : 1.0));
            }
            EXPECT(e.nsteps == 0 && e.stride == 0 && !e.is_static && !e.use_weights);   // the host chose: no stepper
            // the graphs are captured with the source exactly while it is active (stages.cpp ensure_graphs)
            const SourceSlice c = source_slice(s, k, /*capture=*/runs);
            EXPECT(c.due == runs && c.active == runs);
            if (runs) {
              EXPECT(c.offset == 0 && c.scale == 1.0);
              EXPECT(c.nsteps == s.nsteps && c.stride == (form == 0 ? nnz * dim * dim : 0));
              EXPECT(c.use_weights == (form == 2) && c.is_static == (form == 1));
            }
            // ... and replayed past its end: still launched, the kernel adds nothing beyond nsteps
            if (form != 1 && k >= nsteps) EXPECT(source_slice(s, k, true).due && !source_slice(s, k, true).active);
          }
        }
  EXPECT(!source_slice(SourceFacts{}, 0, false).active && !source_slice(SourceFacts{}, 0, false).due);

  // The receivers (seigen_hip.h sg_set_receivers): sample j is taken after step (j + 1) * every; capacity samples fit.
  for (int64_t every : {1, 2, 5})
    for (int64_t capacity : {0, 1, 3})
      for (int64_t call = 1; call <= 7; ++call) {
        StepClock c;
        c.every = every;
        c.count = capacity;
        int64_t done = 0;      // the model: steps completed, and the multiples of `every` among 1..done counted one by one
        auto multiples = [&](int64_t upto) {
          int64_t n = 0;
          for (int64_t s = 1; s <= upto; ++s) n += s % every == 0 ? 1 : 0;
          return n;
        };
        // calls of `call` steps (sg_step) while they fit ...
        for (int guard = 0; guard < 64; ++guard) {
          EXPECT(c.samples() == multiples(done));
          const bool fits = multiples(done + call) <= capacity;
          EXPECT(c.fits(call) == fits);
          EXPECT(c.samples_after(call) == multiples(done + call));
          if (!fits) break;
          c.steps += call;
          done += call;
        }
        // ... then one step at a time (sg_end_step) up to the step that would write sample capacity + 1
        for (int guard = 0; guard < 64; ++guard) {
          const bool refused = (done + 1) % every == 0 && multiples(done + 1) == capacity + 1;
          EXPECT(c.no_room_at(done + 1) == refused);
          EXPECT(c.fits(1) == !refused);
          if (refused) break;
          c.steps += 1;
          done += 1;
          EXPECT(c.samples() == multiples(done) && c.samples() <= capacity);
        }
        EXPECT(c.samples() == capacity);
      }

  // The monitor (seigen_hip.h sg_set_monitor) keeps that clock, armed with capacity >= 1: calls of sg_step while they fit,
  // then sg_end_step up to the refusal - every sample index it hands out lies inside the trace, none is handed out twice.
  for (int64_t every : {1, 3, 4})
    for (int64_t capacity : {1, 2, 5})
      for (int64_t call : {1, 2, 11}) {
        StepClock c;
        c.every = every;
        c.count = capacity;
        std::vector<int> taken((size_t)capacity, 0);
        auto step_done = [&](int64_t s) {     // what the kernels do with step s (kernels_measure.hip sample_index)
          if (s % every != 0) return;
          const int64_t j = s / every - 1;
          EXPECT(j >= 0 && j < capacity);
          if (j >= 0 && j < capacity) taken[(size_t)j] += 1;
        };
        while (c.fits(call)) {
          for (int64_t k = 1; k <= call; ++k) step_done(c.steps + k);
          c.steps += call;
          if (c.steps > 64 * every * capacity) break;
        }
        EXPECT(c.steps <= (capacity + 1) * every);
        for (int guard = 0; guard < 64 && !c.no_room_at(c.steps + 1); ++guard) {
          step_done(c.steps + 1);
          c.steps += 1;
        }
        EXPECT(c.no_room_at(c.steps + 1) && !c.fits(1) && c.samples() == capacity);
        for (int n : taken) EXPECT(n == 1);
      }
  // ... and what its kernels read, in order: the velocity's components, then the stress's - every entry of the tensor counted
  // once, whichever storage
  for (int dim = 1; dim <= 3; ++dim)
    for (bool sym : {false, true}) {
      const std::vector<MonitorComp> cs = monitor_components(dim, sym);
      EXPECT((int)cs.size() == dim + (sym ? dim * (dim + 1) / 2 : dim * dim) && (int)cs.size() <= sg::measure::MAX_COMP);
      std::vector<double> counted((size_t)dim * dim, 0.0);
      int ndiag = 0;
      for (size_t k = 0; k < cs.size(); ++k) {
        EXPECT(cs[k].stress == ((int)k >= dim));
        if (!cs[k].stress) {
          EXPECT(cs[k].comp == (int)k && cs[k].mult == 1.0 && !cs[k].diag);
          continue;
        }
        const int i = cs[k].comp / dim, j = cs[k].comp % dim;
        EXPECT(i < dim && (!sym || i <= j) && cs[k].diag == (i == j));
        counted[(size_t)i * dim + j] += cs[k].mult / (cs[k].mult == 2.0 ? 2.0 : 1.0);
        if (cs[k].mult == 2.0) counted[(size_t)j * dim + i] += 1.0;
        ndiag += cs[k].diag ? 1 : 0;
        if (k > (size_t)dim) EXPECT(cs[k].comp > cs[k - 1].comp);
      }
      EXPECT(ndiag == dim);
      for (double x : counted) EXPECT(x == 1.0);
    }
  {
    const int nd = 4;
    std::vector<double> M((size_t)nd * nd);
    for (int a = 0; a < nd; ++a)
      for (int b = 0; b < nd; ++b) M[(size_t)a * nd + b] = 10.0 * a + b;
    const std::vector<double> tri = mass_lower_rows(M, nd);
    EXPECT(tri.size() == (size_t)nd * (nd + 1) / 2);
    size_t m = 0;
    for (int a = 0; a < nd; ++a)
      for (int b = 0; b <= a; ++b) EXPECT(tri[m++] == 10.0 * a + b);
  }
}

// The correlation's plan (hostlogic.hpp xcorr_components, xcorr_mass_tiles, xcorr_first_difference) against a restatement
// that shares no code with it: two tensors stored the way each handle's storage mode stores them, read through the component
// table, must give sum_ij A_ij B_ij and the two traces; the A tiles, walked by (row, column), must be the mass matrix of
// sg_reference_operator_cell and zero beyond it.
static void correlation_plan(int cell_type, int dim, int degree) {
  const int64_t nn = sg_reference_operator_cell(cell_type, dim, degree, 2, 0, nullptr, 0);
  EXPECT(nn > 0);
  if (nn <= 0) return;
  std::vector<double> M((size_t)nn);
  EXPECT(sg_reference_operator_cell(cell_type, dim, degree, 2, 0, M.data(), M.size() * sizeof(double)) == nn);
  const int nd = num_nodes(dim, degree, cell_type);
  EXPECT((int64_t)nd * nd == nn);
  const std::vector<double> tiles = xcorr_mass_tiles(M, nd);
  int rows = 0, cols = 0;
  while (rows < nd) rows += 16;
  while (cols < nd) cols += 4;
  EXPECT(xcorr_row_tiles(nd) * 16 == rows && xcorr_k_steps(nd) * 4 == cols);
  EXPECT(tiles.size() == (size_t)rows * cols);
  if (tiles.size() == (size_t)rows * cols)
    for (int r = 0; r < rows; ++r)
      for (int c = 0; c < cols; ++c) {
        // lane (r mod 16) + 16 (c mod 4) of tile (r / 16, c / 4): the A operand map of the 16 x 16 x 4 f64 instruction
        const double v = tiles[((size_t)(r / 16) * (cols / 4) + c / 4) * 64 + (size_t)(c % 4) * 16 + r % 16];
        EXPECT(v == ((r < nd && c < nd) ? M[(size_t)r * nd + c] : 0.0));
      }
  for (bool sym_a : {false, true})
    for (bool sym_b : {false, true}) {
      const std::vector<XcorrComp> cs = xcorr_components(dim, sym_a, sym_b);
      EXPECT((int)cs.size() <= sg::xcorr::MAX_COMP);
      // small integers: every sum below is exact
      std::vector<double> A((size_t)dim * dim), B((size_t)dim * dim);
      for (int i = 0; i < dim; ++i)
        for (int j = 0; j < dim; ++j) {
          A[(size_t)i * dim + j] = sym_a ? 1 + 3 * std::min(i, j) + 35 * std::max(i, j) : 1 + 3 * i + 7 * j;
          B[(size_t)i * dim + j] = 2 + 11 * i * (sym_b ? j : 1) + (sym_b ? 13 * (i + j) : 5 * j);
        }
      // a line of the lower triangle holds nothing usable in symmetric storage
      std::vector<double> SA = A, SB = B;
      for (int i = 0; i < dim; ++i)
        for (int j = 0; j < i; ++j) {
          if (sym_a) SA[(size_t)i * dim + j] = 1e300;
          if (sym_b) SB[(size_t)i * dim + j] = 1e300;
        }
      double want = 0, tra = 0, trb = 0;
      for (int i = 0; i < dim; ++i) {
        tra += A[(size_t)i * dim + i];
        trb += B[(size_t)i * dim + i];
        for (int j = 0; j < dim; ++j) want += A[(size_t)i * dim + j] * B[(size_t)i * dim + j];
      }
      double got = 0, gta = 0, gtb = 0, mults = 0;
      int nvel = 0;
      for (size_t k = 0; k < cs.size(); ++k) {
        EXPECT(cs[k].stress == ((int)k >= dim));
        if (!cs[k].stress) {
          EXPECT(cs[k].comp_a == (int)k && cs[k].comp_b == (int)k && cs[k].mult == 1.0 && !cs[k].diag);
          nvel += 1;
          continue;
        }
        EXPECT(cs[k].comp_a >= 0 && cs[k].comp_a < dim * dim && cs[k].comp_b >= 0 && cs[k].comp_b < dim * dim);
        got += cs[k].mult * SA[(size_t)cs[k].comp_a] * SB[(size_t)cs[k].comp_b];
        mults += cs[k].mult;
        if (cs[k].diag) {
          gta += SA[(size_t)cs[k].comp_a];
          gtb += SB[(size_t)cs[k].comp_b];
        }
      }
      EXPECT(nvel == dim && mults == (double)(dim * dim));
      EXPECT(got == want && gta == tra && gtb == trb);
      EXPECT((int)cs.size() == dim + ((sym_a && sym_b) ? dim * (dim + 1) / 2 : dim * dim));
    }
}

static void correlation_compatibility() {
  sg_config a;
  std::memset(&a, 0, sizeof(a));
  a.dim = 3;
  a.degree = 4;
  for (int k = 0; k < 3; ++k) {
    a.n[k] = 4 + k;
    a.h[k] = 0.25;
  }
  EXPECT(xcorr_first_difference(a, 16, a, 16).empty());
  sg_config b = a;
  b.nbr_mask = 5;
  b.origin[1] = 2.0;
  b.cube0[2] = 7;
  EXPECT(xcorr_first_difference(a, 16, b, 16).empty());
  auto named = [&](const sg_config& x, int gw, const char* word) {
    const std::string d = xcorr_first_difference(a, 16, x, gw);
    EXPECT(d.find(word) != std::string::npos);
    EXPECT(!xcorr_first_difference(x, gw, a, 16).empty());
  };
  b = a; b.device = 1; named(b, 16, "device");
  b = a; b.dim = 2; named(b, 16, "dim");
  b = a; b.degree = 3; named(b, 16, "degree");
  b = a; b.diagonal = 1; named(b, 16, "diagonal");
  b = a; b.dtype = 1; named(b, 16, "dtype");
  b = a; b.n[1] = 9; named(b, 16, "n[1]");
  b = a; b.h[2] = 0.5; named(b, 16, "h[2]");
  named(a, 1, "layout");
  // the first difference in the documented order
  b = a; b.degree = 3; b.dtype = 1; named(b, 64, "degree");
}

// The spectra's clock and line list (hostlogic.hpp StepClock, spectra_lines; sg_spectra_clock, sg_spectra_lines) against
// the list of sample steps written out: sample j after step (j + 1) * every, nsamples of them.
static void spectra_clock_and_lines() {
  for (int64_t every : {1, 2, 3, 5})
    for (int64_t nsamples : {0, 1, 3, 4}) {
      std::vector<int64_t> at;
      for (int64_t j = 0; j < nsamples; ++j) at.push_back((j + 1) * every);
      for (int64_t steps = 0; steps < 24; ++steps) {
        StepClock c;
        c.every = every;
        c.count = nsamples;
        c.steps = steps;
        const auto hit = std::find(at.begin(), at.end(), steps + 1);
        EXPECT(c.due_at(steps + 1) == (hit != at.end()));
        if (hit != at.end()) EXPECT(c.sample_at(steps + 1) == hit - at.begin());
        EXPECT(c.active() == (!at.empty() && at.back() > steps));
        for (int64_t more : {0, 1, 7}) {
          const int64_t taken = std::count_if(at.begin(), at.end(), [&](int64_t s) { return s <= steps + more; });
          EXPECT(c.capped_samples_after(more) == taken);
          int64_t out[4] = {-9, -9, -9, -9};
          EXPECT(sg_spectra_clock(every, nsamples, steps, more, out) == SG_OK);
          EXPECT(out[0] == (hit != at.end() ? 1 : 0) && out[1] == (hit != at.end() ? hit - at.begin() : -1));
          EXPECT(out[2] == (c.active() ? 1 : 0) && out[3] == taken);
        }
      }
    }
  int64_t out[4];
  EXPECT(sg_spectra_clock(0, 1, 0, 0, out) == SG_ERR_ARG && sg_spectra_clock(1, 1, 0, 0, nullptr) == SG_ERR_ARG);
  for (int dim = 1; dim <= 3; ++dim)
    for (int sym : {0, 1}) {
      std::vector<int32_t> want;
      for (int i = 0; i < dim; ++i)
        for (int j = 0; j < dim; ++j)
          if (!sym || i <= j) want.push_back(i * dim + j);
      EXPECT(spectra_lines(dim, sym != 0) == want);
      std::vector<int32_t> got(want.size(), -1);
      EXPECT(sg_spectra_lines(dim, sym, got.data(), (int)got.size()) == (int)want.size() && got == want);
      if (want.size() > 1) EXPECT(sg_spectra_lines(dim, sym, got.data(), (int)got.size() - 1) == SG_ERR_ARG);   // no room: nothing written past the end
    }
  EXPECT(sg_spectra_lines(4, 0, nullptr, 16) == SG_ERR_ARG);
}

// The gradient's device-free half (sg_tabulate_grad_cell, sg_gradient_tables, sg_gradient_plan; hostlogic.hpp grad_dense_tables,
// grad_plan): the derivative of the basis sums to zero and reproduces the coordinate functions at every degree up to 8; the
// tables are the tabulation at the nodes and the mesh tables' Jinv, a tensor-product cell's line entries the 1-D matrix; the
// plan's slices cover the nodes once within the LDS budget for every layout, element and kind.
static void gradient_tables_and_plan(int cell_type, int dim) {
  for (int P = 1; P <= 8; ++P) {
    std::vector<int> lat;
    lattice_points(dim, P, lat, cell_type);
    const int nd = num_nodes(dim, P, cell_type);
    const double pts[3][3] = {{0.25, 0.125, 0.5}, {0.0, 0.0, 0.0}, {1.0 / 3, 1.0 / 7, 1.0 / 5}};
    std::vector<double> xi, dphi((size_t)3 * nd * dim);
    for (const auto& p : pts) xi.insert(xi.end(), p, p + dim);
    EXPECT(sg_tabulate_grad_cell(cell_type, dim, P, 3, xi.data(), dphi.data()) == SG_OK);
    double worst = 0;
    for (int p = 0; p < 3; ++p)
      for (int r = 0; r < dim; ++r) {
        double sum = 0, x[3] = {0, 0, 0};
        for (int a = 0; a < nd; ++a) {
          const double d = dphi[((size_t)p * nd + a) * dim + r];
          sum += d;
          for (int i = 0; i < dim; ++i) x[i] += d * lat[(size_t)a * dim + i] / P;   // the gradient of the coordinate x_i
        }
        worst = std::fmax(worst, std::fabs(sum));
        for (int i = 0; i < dim; ++i) worst = std::fmax(worst, std::fabs(x[i] - (i == r ? 1.0 : 0.0)));
      }
    EXPECT(worst < (P <= 4 ? 1e-12 : 1e-8));
    if (P > 4) continue;
    sg_config cfg;
    std::memset(&cfg, 0, sizeof(cfg));
    cfg.dim = dim;
    cfg.degree = P;
    for (int a = 0; a < 3; ++a) {
      cfg.n[a] = a < dim ? 3 : 1;
      cfg.h[a] = 0.5 / (a + 1);
    }
    for (int diagonal : {0, 1}) {
      cfg.diagonal = cell_type == KIND_TENSOR ? SG_DIAGONAL_QUAD : diagonal;
      const int64_t n = sg_gradient_tables(&cfg, nullptr, nullptr);
      EXPECT(n == (int64_t)dim * nd * nd);
      if (n <= 0) continue;
      const int ncls = classes_of(dim, cell_type);
      std::vector<double> C((size_t)n), J((size_t)ncls * 9, -1.0);
      EXPECT(sg_gradient_tables(&cfg, C.data(), J.data()) == n && sg_gradient_tables(&cfg, C.data(), nullptr) == n);
      EXPECT(C == grad_dense_tables(cell_type, dim, P, lat));
      std::vector<double> at((size_t)nd * dim), tab((size_t)nd * nd * dim);
      for (size_t k = 0; k < at.size(); ++k) at[k] = (double)lat[k] / (double)P;
      EXPECT(sg_tabulate_grad_cell(cell_type, dim, P, nd, at.data(), tab.data()) == SG_OK);
      bool same = true, line = true;
      const int n1 = P + 1;
      for (int r = 0; r < dim; ++r)
        for (int a = 0; a < nd; ++a)
          for (int b = 0; b < nd; ++b) {
            const double c = C[((size_t)r * nd + a) * nd + b];
            same = same && c == tab[((size_t)a * nd + b) * dim + r];
            if (cell_type != KIND_TENSOR) continue;
            bool on = true;
            for (int i = 0; i < dim; ++i) on = on && (i == r || lat[(size_t)a * dim + i] == lat[(size_t)b * dim + i]);
            if (on) line = line && c == C[(size_t)lat[(size_t)a * dim + r] * nd + lat[(size_t)b * dim + r]];   // C1 = C[0][:n1][:n1]
            else line = line && std::fabs(c) < 1e-14;
          }
      EXPECT(same && line && n1 <= nd);
      for (int k = 0; k < ncls; ++k)
        for (int r = 0; r < 3; ++r)
          for (int j = 0; j < 3; ++j) {
            const double v = J[((size_t)k * 3 + r) * 3 + j];
            if (r >= dim || j >= dim) EXPECT(v == 0.0);
            else if (cell_type == KIND_TENSOR) EXPECT(v == (r == j ? 1.0 / cfg.h[r] : 0.0));
            else EXPECT(std::isfinite(v));
          }
      if (cell_type == KIND_TENSOR) break;
    }
    // the plan
    const int ncls = classes_of(dim, cell_type);
    for (int gw : {1, 16, 64})
      for (int kind = 0; kind < 4; ++kind) {
        const int ncomp = grad_ncomp(dim, kind);
        if (ncomp == 0) {
          EXPECT(kind == 2 && dim == 1);
          continue;
        }
        for (int64_t ncube : {1, 17, 130}) {
          const int64_t ncells = ncube * ncls;
          for (const auto& rg : {std::pair<int64_t, int64_t>{0, ncells}, {ncells / 2, ncells - ncells / 2}, {ncells - 1, 1}, {0, 0}}) {
            int64_t out[6] = {-1, -1, -1, -1, -1, -1}, xf[6];
            const int rc = sg_gradient_plan(gw, ncls, nd, dim, ncomp, 8, 4, rg.first, rg.second, out);
            const GradPlan p = grad_plan(gw, ncls, nd, dim, ncomp, rg.first, rg.second);
            EXPECT((rc == SG_OK) == p.ok);
            if (rc != SG_OK) continue;   // (an element whose velocity block alone is beyond the budget on that layout: refused, not planned)
            EXPECT(sg_xfer_plan(gw, ncls, nd, ncomp, 8, 4, rg.first, rg.second, xf) == SG_OK && out[0] == xf[0] && out[1] == xf[1]);
            EXPECT(out[5] <= GRAD_LDS_BUDGET && out[4] <= XFER_GRID_CAP);
            if (rg.second == 0) {
              EXPECT(out[4] == 0);
              continue;
            }
            EXPECT(out[4] >= 1 && out[2] >= 1 && out[3] >= 1 && out[2] * out[3] >= nd && out[2] * (out[3] - 1) < nd);
            if (gw > 1) EXPECT(p.out_offset % 16 == 0 && p.out_offset >= (int64_t)nd * dim * (gw + 1) * 8 && out[5] == p.out_offset + out[2] * ncomp * (gw + 1) * 8);
          }
        }
      }
  }
  int64_t out[6];
  double x = 0, d[8];
  EXPECT(sg_gradient_plan(8, 1, 3, 1, 1, 8, 8, 0, 1, out) == SG_ERR_ARG && sg_gradient_plan(16, 1, 3, 1, 2, 8, 8, 0, 1, out) == SG_ERR_ARG);
  EXPECT(sg_gradient_plan(16, 1, 3, 1, 1, 8, 8, 0, 1, nullptr) == SG_ERR_ARG);
  EXPECT(sg_tabulate_grad_cell(0, 1, 9, 1, &x, d) == SG_ERR_ARG && sg_tabulate_grad_cell(2, 1, 2, 1, &x, d) == SG_ERR_ARG);
  EXPECT(sg_tabulate_grad_cell(0, 1, 2, 1, nullptr, d) == SG_ERR_ARG && sg_tabulate_grad_cell(0, 1, 2, 1, &x, nullptr) == SG_ERR_ARG);
  EXPECT(sg_gradient_tables(nullptr, nullptr, nullptr) == SG_ERR_ARG);
}

int main() {
  spectra_clock_and_lines();
  for (int cell_type : {0, 1})
    for (int dim = 1; dim <= 3; ++dim)
      for (int degree = 1; degree <= 4; ++degree)
        if (!(cell_type == 1 && dim == 1)) correlation_plan(cell_type, dim, degree);
  correlation_compatibility();
  for (int cell_type : {0, 1})
    for (int dim = 1; dim <= 3; ++dim)
      for (int degree = 1; degree <= 4; ++degree) {
        if (cell_type == 1 && dim == 1) {     // no tensor-product cell in 1-D (an interval is a simplex): refused
          EXPECT(sg_reference_operator_cell(1, 1, degree, 0, 0, nullptr, 0) == SG_ERR_ARG);
          continue;
        }
        reference_operators(cell_type, dim, degree);
      }
  for (int dim = 1; dim <= 3; ++dim)
    for (int degree = 1; degree <= 4; ++degree)
      for (int diagonal : {0, 1, 2}) {
        if (diagonal == 2 && dim == 1) continue;
        mesh_tables(dim, degree, diagonal);
      }
  for (int degree = 1; degree <= 4; ++degree) {
    mfma_tables_3d(degree);
    trace_lines_3d(degree);
    class_frame_3d(degree);
    tile_tables_2d(degree, KIND_SIMPLEX);
    tile_tables_2d(degree, KIND_TENSOR);
  }
  for (int cell_type : {0, 1})
    for (int dim = 1; dim <= 3; ++dim)
      if (!(cell_type == 1 && dim == 1)) gradient_tables_and_plan(cell_type, dim);
  regions_and_coords();
  point_location();
  kernel_family_table();
  grid_overrides();
  stage_table();
  stepping_state();
  for (int dim = 1; dim <= 3; ++dim)
    for (int degree : {1, 2, 4})
      for (int kind : {KIND_SIMPLEX, KIND_TENSOR}) {
        if (kind == KIND_TENSOR && dim == 1) continue;
        if (kind == KIND_TENSOR && dim == 3 && degree == 4) continue;      // 125^3 sponge tensor: minutes under the sanitizers
        for (int q : {1, 4}) sponge_plans(dim, degree, kind, q);
      }
  region_item_lists();
  for (int dim = 1; dim <= 3; ++dim)
    for (int kind : {KIND_SIMPLEX, KIND_TENSOR}) {
      if (kind == KIND_TENSOR && dim == 1) continue;
      source_plans(dim, kind);
      for (int degree : {1, 3}) {
        box_ricker(dim, kind == KIND_TENSOR ? SG_DIAGONAL_QUAD : dim % 2, degree);
        receiver_plans(dim, kind == KIND_TENSOR ? SG_DIAGONAL_QUAD : dim % 2, degree);
        injector_plans(dim, kind == KIND_TENSOR ? SG_DIAGONAL_QUAD : dim % 2, degree);
      }
    }
  // arguments the entry points must refuse
  EXPECT(sg_reference_operator_cell(7, 2, 2, 0, 0, nullptr, 0) == SG_ERR_ARG);
  EXPECT(sg_reference_operator_cell(0, 2, 2, 9, 0, nullptr, 0) == SG_ERR_ARG);
  EXPECT(sg_tabulate_cell(0, 4, 2, 1, nullptr, nullptr) == SG_ERR_ARG);
  EXPECT(sg_mesh_tables(2, 2, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == SG_ERR_ARG);
  std::printf("host_asan_driver: %s (%d failed expectations)\n", nfail ? "FAILED" : "clean", nfail);
  return nfail ? 1 : 0;
}
