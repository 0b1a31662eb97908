// CPU sanitizer driver (SURVEY 5 "sanitizers"; `make -C seigen_amd/csrc host-asan`): everything of libseigen_hip that
// needs no device - reference elements, mesh tables, MFMA fragment tables, the device-free C-ABI entry points - built with
// -fsanitize=address,undefined and walked over every (dim, degree, cell type, diagonal) the library accepts, plus the
// argument errors the entry points must refuse.  Exit code 0 and no sanitizer report = clean.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hostlogic.hpp"
#include "kernels.hpp"
#include "mfma_tables.hpp"
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

int main() {
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
    tile_tables_2d(degree, KIND_SIMPLEX);
    tile_tables_2d(degree, KIND_TENSOR);
  }
  regions_and_coords();
  point_location();
  kernel_family_table();
  stage_table();
  for (int dim = 1; dim <= 3; ++dim)
    for (int degree : {1, 2, 4})
      for (int kind : {KIND_SIMPLEX, KIND_TENSOR}) {
        if (kind == KIND_TENSOR && dim == 1) continue;
        if (kind == KIND_TENSOR && dim == 3 && degree == 4) continue;      // 125^3 sponge tensor: minutes under the sanitizers
        for (int q : {1, 4}) sponge_plans(dim, degree, kind, q);
      }
  // arguments the entry points must refuse
  EXPECT(sg_reference_operator_cell(7, 2, 2, 0, 0, nullptr, 0) == SG_ERR_ARG);
  EXPECT(sg_reference_operator_cell(0, 2, 2, 9, 0, nullptr, 0) == SG_ERR_ARG);
  EXPECT(sg_tabulate_cell(0, 4, 2, 1, nullptr, nullptr) == SG_ERR_ARG);
  EXPECT(sg_mesh_tables(2, 2, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == SG_ERR_ARG);
  std::printf("host_asan_driver: %s (%d failed expectations)\n", nfail ? "FAILED" : "clean", nfail);
  return nfail ? 1 : 0;
}
