// Host logic of libseigen_hip that needs no device and no HIP header: which kernel family runs a block, the layout of its
// fields, the six stages of an LF4 step, the boxes and items of the regions of a split stage, node coordinates of a block,
// point location, the receiver plan, the gauge plan, the injector plan, the transfer plan and the frame plan.  Defined in hostapi.cpp, which - with refelem.cpp, mesh_tables.cpp, mfma_tables.cpp,
// sponge_tables.cpp and source_tables.cpp - also builds on its own for the CPU sanitizer target (`make host-asan`).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/seigen_hip.h"
#include "mesh_tables.hpp"
#include "refelem.hpp"

extern std::string g_create_err;   // message of the last failed sg_create / device-free query

// Which kernel family runs a block (choose_kernel_path, hostapi.cpp):
//   Generic  thread-per-node, table-driven kernels on the host layout (kernels.hip); every element
//   Lane     lane-per-cell (kernels_lane.hip): 1-D / 2-D simplices and 3-D P1 / P2 on request, hexahedra DQ_1 / DQ_2
//   Mfma     3-D simplices on the matrix pipe (kernels_mfma.hip)
//   Tile2d   2-D MFMA tiles (kernels_tile2d.hip): triangles and quadrilaterals
//   Hexm     hexahedra DQ_3 / DQ_4, lines in registers, x lines on the matrix pipe (kernels_hexm.hip)
enum class Family { Generic, Lane, Mfma, Tile2d, Hexm };
Family choose_kernel_path(const sg_config& cfg);
// measured crossover of the (sum-factorised) generic and the lane kernels on hexahedra (tools/experiments/
// hex_crossover.py, profiles/r04/hexahedra.txt): between 24^3 and 32^3 cubes at both degrees
#ifndef SG_HEX_LANE_MIN_CELLS
#define SG_HEX_LANE_MIN_CELLS(degree) 24000
#endif

// What the host code asks about a family.  The layout's group width (MeshDev::gw): 16 cubes per 128-byte line for the
// matrix-pipe families, 64 for the lane kernels, 1 = host layout for the generic kernels.
inline int family_gw(Family f) { return f == Family::Generic ? 1 : (f == Family::Lane ? 64 : 16); }
// The interleaved layout of a block's fields, stated here once for the host code (the kernels keep their own arithmetic):
// gw consecutive cubes - a group - put the cells of one class side by side on the lanes of an ITEM, and node b, component c
// of a field with ncomp components of cell (cube, cls) lives at
//   ((((cube / gw) * ncls + cls) * nd + b) * ncomp + c) * gw + cube % gw
// (gw = 1: the host layout [cell][node][comp]).  The host numbers a scalar node (cube * ncls + cls) * nd + b.
struct Layout {
  int64_t gw = 1, ncls = 1, nd = 1;
  int64_t group(int64_t cube) const { return cube / gw; }   // (of ncube_pad: the number of groups)
  int64_t lane(int64_t cube) const { return cube % gw; }
  int64_t item(int64_t cube, int64_t cls) const { return group(cube) * ncls + cls; }
  int64_t offset(int64_t cube, int64_t cls, int64_t b, int64_t ncomp, int64_t c) const {
    return ((item(cube, cls) * nd + b) * ncomp + c) * gw + lane(cube);
  }
  struct Node {
    int64_t cube, cls, b;
  };
  Node split(int64_t node) const { return {node / nd / ncls, node / nd % ncls, node % nd}; }
};

// Every family but the generic one: interleaved layout, one launch per region over (cell group, class) items, the
// symmetric-stress mode, and a sigma that is one value on all nodes of a cell applied as sigma u at the node.
inline bool family_interleaved(Family f) { return f != Family::Generic; }
// sg_config.dtype = 1 (fields, halo buffers, operator tiles and arithmetic in float)
inline bool family_f32(Family f) { return f == Family::Mfma || f == Family::Tile2d; }
// F stages read B u_abs of the sponge cells from a pre-pass (kernels.hpp launch_sponge_pre); the 2-D tile kernels work
// their small matrices off themselves: a launch more per F stage costs them more
inline bool family_sponge_pre(Family f) { return f == Family::Mfma || f == Family::Hexm || f == Family::Lane; }
// ... and the pre-pass results live in line layout like the fields (3-D MFMA: a record per cell cost the affine
// pre-pass scattered 24-byte stores and the F stage scattered loads)
inline bool family_pre_lines(Family f) { return f == Family::Mfma; }
// the G stage kernels add the source themselves (StageArgs::src_slot / src_idx; SEIGEN_HIP_SOURCE_LAUNCH: a launch of its own)
inline bool family_fused_source(Family f) { return f == Family::Tile2d; }
// a region of whole cell groups runs as a whole-block launch: no cube coordinates, no box tests (StageArgs::all_active)
inline bool family_whole_groups(Family f) { return f == Family::Mfma || f == Family::Hexm; }

// SEIGEN_HIP_GRID_BLOCKS as a persistent grid: whole multiples of eight blocks (an item range belongs to an XCD label,
// blockIdx % 8), never fewer than eight ...
inline int grid_blocks_override(int value) { return value / 8 * 8 > 8 ? value / 8 * 8 : 8; }
// ... and what it leaves of the grid prepared for the affine-sigma pre-pass of sg_set_absorption (SpongeTables::aff_grid,
// either form): the switch only ever shrinks that grid, so that a block or wave of the pre-pass can be made to run item
// after item on a small mesh.  The item split changes speed, never a result.
inline int affine_grid_cap(int prepared, int value) { return prepared < grid_blocks_override(value) ? prepared : grid_blocks_override(value); }

// One launch of a stage kernel as a value (stages.cpp run_op): F or G of a field and the fused epilogue around it
// (kernels.hpp StageArgs::mode / c_self / c_aux / c_new).  The defaults are the un-fused application out = F(in; u) / G(in).
struct StageOp {
  int kind = -1;            // 0 = F (stress -> velocity), 1 = G (velocity -> stress)
  int in = -1, out = -1, aux = -1, uabs = SG_FIELD_U;   // SG_FIELD_*; aux = -1: none; uabs: what the sponge of an F stage absorbs
  int mode = 0;
  double c_self = 0.0, c_aux = 0.0, c_new = 0.0;
  bool with_source = false;   // a G stage that adds the source: in the kernel (2-D tile family) or by a launch after it
  double src_coef = 1.0;      // factor on the source
  bool density = false;       // the per-cell density factors go with the launch (stage U1)
};
// The six fused launches of an LF4 step (enum sg_stage), stated here alone: the native exchange takes a stage's input and
// output field from it, seigen_amd/parallel.py STAGE_INPUT / STAGE_OUTPUT is tested against it.  No such stage: kind = -1.
StageOp lf4_stage(int stage, double dt, double rho, bool rho_physical, bool per_cell_density);
inline int lf4_stage_input(int stage) { return lf4_stage(stage, 0.0, 1.0, false, false).in; }
inline int lf4_stage_output(int stage) { return lf4_stage(stage, 0.0, 1.0, false, false).out; }

// What the stepping calls remember from one call to the next, as values: written by stages.cpp and the transfers, stated and
// walked without a device (tools/host_asan_driver.cpp stepping_state).

// Writes to each of the four fields, counted: a field whose count stands still holds the state it held.
struct FieldVersions {
  uint64_t v[4] = {0, 0, 0, 0};
  void written(int f) { v[f] += 1; }
  void replayed() {   // a graph replay wrote all four
    for (uint64_t& x : v) x += 1;
  }
};

// The sponge pre-pass buffer of the F stages (handle.hpp SpongeTables::pre) holds B_e u_abs of a FIELD STATE: stages UH1 and
// U1 both absorb u0 (elastic.py:206-208 in form_uh1 and form_uh2), UTEMP absorbs the u1 that U1 wrote, and the next step's
// UH1 and U1 absorb that same u1 - so in the steady state of eager and host-driven steps UH1 finds UTEMP's pre-pass and a
// step runs ONE pre-pass (UTEMP's), not three.  A captured graph computes it afresh at its own first step (two in graph1,
// nine in graph8), and a replay leaves nothing to reuse.
struct PrePass {
  // A launch of `op` on `region` is about to be queued: does the pre-pass run first?  It does at the first launch of a stage
  // - whichever region the caller starts with: the same stage again, or a region it has already seen, is the next instance
  // of the stage - unless the buffer already holds that state of op.uabs.  Asked BEFORE the launch counts as a write of its
  // output: an in-place stage (U1) absorbs the state it overwrites, and its later regions find the pre-pass of the first.
  bool due(const StageOp& op, int region, const FieldVersions& fv) {
    if (op.kind != 0) return false;
    const int k = op.out * 4 + op.mode;
    const bool first_of_stage = k != key || (regions & (1 << region)) != 0 || region == SG_REGION_ALL;
    if (first_of_stage) regions = 0;
    key = k;
    regions |= 1 << region;
    if (!first_of_stage || (field == op.uabs && ver == fv.v[op.uabs])) return false;
    field = op.uabs;
    ver = fv.v[op.uabs];
    return true;
  }
  // the buffer holds nothing known: the launches of a capture compute their own, and so does whatever follows a replay
  void forget() { ver = ~0ull; }

 private:
  int key = -1, regions = 0;   // the F stage (output field, mode) whose pre-pass was asked for last, the regions launched since
  int field = -1;              // the state the buffer holds: this field at ...
  uint64_t ver = ~0ull;        // ... this count of its writes (~0: none)
};

// The source at one step (seigen_hip.h sg_set_source / sg_set_source_separable): which slice of the value table, which
// weight.  Eager launches get both from the host; the launches of a capture made while the source was active read them
// off a device-side step counter (kernels.hpp SrcStep) and are due at every replayed step - the kernel adds nothing
// once the source has run out.
struct SourceFacts {
  int64_t nnz = 0, nsteps = 0;
  bool is_static = false;            // one slice that holds at every step
  const double* weights = nullptr;   // [nsteps] on the host: a separable source (one slice, scaled), else null
  int dim = 0;
};
struct SourceSlice {
  bool active = false;    // the source has a slice for this step
  bool due = false;       // ... and a launch adds it
  int64_t offset = 0;     // doubles from the start of the value table to the slice (a capture: the kernel's business)
  double scale = 1.0;
  // SrcStep but for its device pointers; all zero outside a capture
  int64_t nsteps = 0, stride = 0;
  bool is_static = false, use_weights = false;
};
inline SourceSlice source_slice(const SourceFacts& s, int64_t step, bool capture) {
  SourceSlice r;
  r.active = s.nnz != 0 && (s.is_static || step < s.nsteps);
  r.due = capture || r.active;
  const int64_t stride = (s.is_static || s.weights) ? 0 : s.nnz * s.dim * s.dim;
  if (capture) {
    r.nsteps = s.nsteps;
    r.stride = stride;
    r.use_weights = s.weights != nullptr;
    r.is_static = s.is_static || (stride == 0 && !s.weights);
  } else if (r.active) {
    r.offset = step * stride;
    if (s.weights) r.scale = s.weights[step];
  }
  return r;
}

// The clock of everything that runs at the end of a step (stages.cpp hooks): sample j (0-based) belongs to step (j + 1) * every
// counted from the arming call, and there are `count` of them - the capacity of the receivers' and the monitor's trace, the
// spectra's and the peak maps' nsamples, the injectors' nsteps (every = 1: entry k is added at the end of step k + 1).  What
// happens when the series is full is the hook's business, not the clock's: the receivers and the monitor refuse the step (fits,
// no_room_at; their count of samples is the uncapped one, which the refusals keep within count), the spectra, the peak maps and
// the injectors run out silently (due_at, active; their count of samples is the capped one).
struct StepClock {
  int64_t every = 1, count = 0;
  int64_t steps = 0;   // completed since arming
  bool due_at(int64_t s) const { return s >= 1 && s % every == 0 && s / every <= count; }   // step s (1-based) has a sample
  int64_t sample_at(int64_t s) const { return s / every - 1; }                                 // ... this one
  bool active() const { return (steps + every) / every <= count; }                            // ... and so has some later step
  int64_t samples_after(int64_t n) const { return (steps + n) / every; }                      // due once n more steps are done
  int64_t samples() const { return samples_after(0); }
  int64_t capped_samples_after(int64_t n) const { return std::min(samples_after(n), count); }   // ... and taken: no more than count
  int64_t capped_samples() const { return capped_samples_after(0); }
  bool fits(int64_t n) const { return samples_after(n) <= count; }                          // n more steps
  bool no_room_at(int64_t s) const { return s % every == 0 && s / every > count; }          // step s is due a sample and has none
};

// What the monitor's kernels (seigen_hip.h sg_set_monitor) read, in the order they read it (kernels_measure.hip): the dim
// components of the velocity, then the stress's - all dim^2 of full storage, the i <= j ones of symmetric storage, where an
// off-diagonal form counts twice; the diagonal ones also make up the trace t.
struct MonitorComp {
  int comp = 0;        // index of the component in its field (velocity: i, stress: i * dim + j)
  bool stress = false, diag = false;
  double mult = 1.0;
};
inline std::vector<MonitorComp> monitor_components(int dim, bool sym) {
  std::vector<MonitorComp> r;
  for (int i = 0; i < dim; ++i) r.push_back({i, false, false, 1.0});
  for (int i = 0; i < dim; ++i)
    for (int j = sym ? i : 0; j < dim; ++j) r.push_back({i * dim + j, true, i == j, (sym && i != j) ? 2.0 : 1.0});
  return r;
}
// ... and the reference mass matrix as the rows b = 0 .. a of its lower triangle, nd (nd + 1) / 2 values
inline std::vector<double> mass_lower_rows(const std::vector<double>& Mhat, int nd) {
  std::vector<double> r;
  for (int a = 0; a < nd; ++a)
    for (int b = 0; b <= a; ++b) r.push_back(Mhat[(size_t)a * nd + b]);
  return r;
}

// The correlation of two handles' fields (seigen_hip.h sg_correlate; kernels_xcorr.hip).  What its kernels read, in the order
// they read it: the dim components of the velocity, then the stress's row-major.  Each handle reads entry (i, j) from the
// line its own storage holds - the mirror (min, max) in symmetric storage.  Both symmetric: only i <= j, an off-diagonal
// form counts twice; otherwise all dim^2 pairs.  The diagonal ones also make up the traces t_a, t_b.
struct XcorrComp {
  int comp_a = 0, comp_b = 0;   // index of the component in a's / b's field (velocity: i, stress: i * dim + j)
  bool stress = false, diag = false;
  double mult = 1.0;
};
inline std::vector<XcorrComp> xcorr_components(int dim, bool sym_a, bool sym_b) {
  std::vector<XcorrComp> r;
  for (int i = 0; i < dim; ++i) r.push_back({i, i, false, false, 1.0});
  const bool both = sym_a && sym_b;
  auto line = [dim](bool sym, int i, int j) { return sym && i > j ? j * dim + i : i * dim + j; };
  for (int i = 0; i < dim; ++i)
    for (int j = both ? i : 0; j < dim; ++j)
      r.push_back({line(sym_a, i, j), line(sym_b, i, j), true, i == j, (both && i != j) ? 2.0 : 1.0});
  return r;
}
// The reference mass matrix as the A operands of v_mfma_f64_16x16x4_f64, padded with zeros to whole 16 x 4 tiles: tile
// (rt, ks) holds rows 16 rt .. + 15, columns 4 ks .. + 3, and lane l of a wave holds its entry (row l & 15, column l >> 4):
// tiles[(rt * nks + ks) * 64 + l], nrt = ceil(nd / 16) row tiles of nks = ceil(nd / 4) k-steps.
inline int xcorr_row_tiles(int nd) { return (nd + 15) / 16; }
inline int xcorr_k_steps(int nd) { return (nd + 3) / 4; }
inline std::vector<double> xcorr_mass_tiles(const std::vector<double>& Mhat, int nd) {
  const int nrt = xcorr_row_tiles(nd), nks = xcorr_k_steps(nd);
  std::vector<double> r((size_t)nrt * nks * 64, 0.0);
  for (int rt = 0; rt < nrt; ++rt)
    for (int ks = 0; ks < nks; ++ks)
      for (int l = 0; l < 64; ++l) {
        const int row = 16 * rt + (l & 15), col = 4 * ks + (l >> 4);
        if (row < nd && col < nd) r[((size_t)rt * nks + ks) * 64 + l] = Mhat[(size_t)row * nd + col];
      }
  return r;
}
// Two handles correlate when they are on one device and agree in dim, degree, cell type and diagonal, dtype, n[], h[] and
// the layout of their fields (gw); nbr_mask, origin and everything set later may differ.  Returns the name of the first
// difference in that order, or an empty string.
inline std::string xcorr_first_difference(const sg_config& a, int gw_a, const sg_config& b, int gw_b) {
  if (a.device != b.device) return "device";
  if (a.dim != b.dim) return "dim";
  if (a.degree != b.degree) return "degree";
  if (a.diagonal != b.diagonal) return "diagonal";
  if (a.dtype != b.dtype) return "dtype";
  for (int k = 0; k < a.dim; ++k)
    if (a.n[k] != b.n[k]) return "n[" + std::to_string(k) + "]";
  for (int k = 0; k < a.dim; ++k)
    if (a.h[k] != b.h[k]) return "h[" + std::to_string(k) + "]";
  if (gw_a != gw_b) return "field layout (gw " + std::to_string(gw_a) + " against " + std::to_string(gw_b) + ")";
  return std::string();
}

struct Box {
  int o[3], n[3];
};
// shell thickness along x: the interleaved layouts put gw consecutive cubes of an x-row on the lanes of one item, so a
// one-cube shell next to an x side would use one lane in gw of every item it touches AND make the launch that owns the
// other gw - 1 lanes run the same item again.  With whole groups in the shell no item is cut (2 x 2 x 2).
// ... unless that would leave the launch that runs beside the exchange less than half of the block's rows to work on
// (a block with neighbours on both x sides and n[0] <= 2 gw had an EMPTY interior: nothing overlapped the exchange), or
// the layout is the lane kernels' (64 cubes per item: the shell would swallow blocks up to 128 cubes wide).  Then the
// shell is one cube thick again and the kernels mask the lanes of the groups it cuts (region_whole = false).
inline int shell_width_x(int gw, int n0, bool nbr_lo, bool nbr_hi) {
  if (gw <= 1 || gw >= 64) return 1;
  const int sides = (nbr_lo ? 1 : 0) + (nbr_hi ? 1 : 0);
  return 2 * (n0 - sides * gw) >= n0 ? gw : 1;
}
void region_boxes(int d, const int32_t n[3], const int32_t has_nbr[6], int region, std::vector<Box>& out, int xw);
// The (cell group, class) items that the boxes of a region touch, ascending, and whether every group they touch is whole
// (then the kernels skip the cube coordinates and the box tests, as in a whole-block launch).  The boxes are disjoint.
struct RegionItems {
  std::vector<int32_t> items;
  bool whole = true;
};
RegionItems region_items(const std::vector<Box>& boxes, const int32_t n[3], const Layout& L, int64_t ncube, int64_t ncube_pad);

// Node coordinates of a block: the affine image of the reference lattice under every cell's vertex map (one
// arithmetic, shared by sg_block_node_coords and the source box test of sg_set_source_box_ricker).
struct NodeGeom {
  int d = 0, degree = 0, nq = 0, ncls = 0;
  std::vector<int> lat;
  int off[sg::MAX_CLS][4][3];
  const sg_config* cfg = nullptr;
  bool init(const sg_config* c, int deg) {
    cfg = c;
    d = c->dim;
    degree = deg;
    const bool quad = c->diagonal == sg::SG_DIAGONAL_QUAD;
    if (quad && d != 2 && d != 3) return false;
    const int kind = quad ? sg::KIND_TENSOR : sg::KIND_SIMPLEX;
    sg::lattice_points(d, degree, lat, kind);
    nq = sg::num_nodes(d, degree, kind);
    if (quad) {   // vertex 0 the low corner, vertex 1 / 2 / 3 one cell along x / y / z: the affine map of the unit square / cube
      std::memset(off, 0, sizeof(off));
      ncls = 1;
      for (int m = 0; m < d; ++m) off[0][m + 1][m] = 1;
    } else {
      sg::class_vertices(d, c->diagonal, ncls, off);
    }
    return true;
  }
  // coordinates of node a of the cell of class k in cube c
  void node(const int c[3], int k, int a, double x[3]) const {
    double X[4][3];
    for (int v = 0; v <= d; ++v)
      for (int i = 0; i < d; ++i) X[v][i] = cfg->origin[i] + (double)(cfg->cube0[i] + c[i] + off[k][v][i]) * cfg->h[i];
    for (int i = 0; i < d; ++i) {
      double xv = X[0][i];
      for (int m = 0; m < d; ++m) xv += (X[m + 1][i] - X[0][i]) * ((double)lat[a * d + m] / (double)degree);
      x[i] = xv;
    }
  }
};

// Point location of sg_locate_points and sg_set_receivers: the rule of seigen_amd/functionspace.py locate, with the
// candidate cubes counted in the MESH's indices.  Per axis the cube holding the point; on a grid line (|t - round t| <
// 1e-9) also the one below it, provided that exists (global index >= 0).  The candidates are tried in ascending order
// (z slowest), in each the classes in ascending order; the first whose reference coordinates pass -1e-12 / 1 + 1e-12
// wins.  Every block of a partition finds the same winner; the block that holds it owns the point.
// Returns the block-local cell (xi[dim] its reference coordinates) or -1: another block's, or outside the mesh.
int64_t locate_point(const NodeGeom& G, const double* p, double* xi);

// What sg_set_receivers derives from the points: of the nrec points pts[nrec][dim] the ones this block owns (own[k] = 1),
// in the order given - their row of the output, the item and lane of the owning cell (Layout) and the cell's basis at the
// point.  Throws std::invalid_argument where capacity x owned x ncomp values of trace are more than 2^40.
struct ReceiverPlan {
  std::vector<int32_t> own;    // [nrec]
  std::vector<int64_t> row;    // [nown] -> receiver index
  std::vector<int64_t> item;   // [nown]
  std::vector<int32_t> lane;   // [nown]
  std::vector<double> phi;     // [nown][nd]
  int ncomp = 0;               // what bit 0: velocity (dim values), bit 1: stress (dim x dim)
};
ReceiverPlan plan_receivers(const NodeGeom& G, const Layout& L, int kind, int64_t nrec, const double* pts, int what, int64_t capacity);

// The gauges (seigen_hip.h sg_set_gauges / sg_probe_gradient; kernels_gauge.hip): the broken gradient of the velocity at physical
// points.  D[r][a] = d(phi_a)/d(xi_r) at the point's reference coordinates, dense over all nd nodes for both cell kinds: bitwise
// refelem.hpp tabulate_grad of the one point, transposed to rows the kernel's chain walks.
void gauge_weights(int dim, int degree, int cell_kind, int nd, const double* xi, double* D);
// What sg_set_gauges and sg_probe_gradient derive from the points: of the npts points pts[npts][dim] the ones this block owns
// (locate_point: the receivers' rule; on a grid line the lower cell), in the order given - their row of the output, the item and
// lane of the owning cell (Layout), the cell's class and D.  ncomp = grad_ncomp(dim, kind).  Throws std::invalid_argument where
// capacity x owned x ncomp values of trace are more than 2^40.
struct GaugePlan {
  std::vector<int32_t> own;    // [npts]
  std::vector<int64_t> row;    // [nown] -> point index
  std::vector<int64_t> item;   // [nown]
  std::vector<int32_t> lane;   // [nown]
  std::vector<int32_t> cls;    // [nown]
  std::vector<double> D;       // [nown][dim][nd]
  int ncomp = 0;
};
GaugePlan plan_gauges(const NodeGeom& G, const Layout& L, int cell_kind, int64_t npts, const double* pts, int kind, int64_t capacity);

// The injectors (seigen_hip.h sg_inject / sg_set_injectors): the transpose of the receivers.  Where the recorder forms
// sum_a phi_a(xi) field[cell][a][c], an injector adds amp * psi_a to the same cell, psi = Mhat^-1 phi(xi) / |det J| - the L2
// projection of amp * delta(x - x_r) onto the element.  psi_a = (sum_b Minv[a][b] phi_b) / |det J| over b ascending with fma
// from zero, then one division; |det J| = the product of the cell sizes (mesh_tables.hpp: every cell of a block has it).
void injector_weights(const sg::RefElem& re, int degree, double detj, const double* xi, double* psi);
// What the injector calls derive from the points: of the npts points the ones this block owns (locate_point: the receivers'
// rule), grouped by cell - the groups in ascending cell order, the points of a cell in the order given (a stable sort: the
// order of the kernel's sum) - with the item and lane of each group's cell (Layout) and psi of each point.
struct InjectorPlan {
  std::vector<int32_t> own;     // [npts]
  std::vector<int64_t> row;     // [nown] -> point index, group after group
  std::vector<double> psi;      // [nown][nd], in the order of row
  std::vector<int64_t> cell;    // [ngroups] block-local cell, ascending
  std::vector<int64_t> item;    // [ngroups]
  std::vector<int32_t> lane;    // [ngroups]
  std::vector<int64_t> start;   // [ngroups + 1]: group g holds rows start[g] .. start[g + 1] - 1
  int ncomp = 0;                // what bit 0: velocity (dim values), bit 1: stress (dim x dim)
};
InjectorPlan injector_plan(const NodeGeom& G, const Layout& L, const sg::RefElem& re, int64_t npts, const double* pts, int what);
// amp[nsteps][npts][ncomp] of the caller -> [nsteps][nown][ncomp] in the order of the plan's rows; and whether the stress part
// (the last dim * dim of a point's ncomp values, what bit 1) of every owned point is symmetric to the bit at every step
std::vector<double> injector_gather(const InjectorPlan& pl, int64_t npts, int64_t nsteps, const double* amp);
bool injector_symmetric(const InjectorPlan& pl, int dim, int what, int64_t nsteps, const std::vector<double>& gathered);

// The spectra (seigen_hip.h sg_set_spectra; kernels_spectra.hip): the lines c = i * dim + j of a stress word ((item * nd + a) * dim^2 + c) * gw + lane that are accumulated: all dim^2 of full
// storage, the i <= j ones of symmetric storage (the others hold no valid stress there)
inline bool spectra_line_kept(int dim, bool sym, int c) { return !sym || c / dim <= c % dim; }
inline std::vector<int32_t> spectra_lines(int dim, bool sym) {
  std::vector<int32_t> r;
  for (int c = 0; c < dim * dim; ++c)
    if (spectra_line_kept(dim, sym, c)) r.push_back(c);
  return r;
}

// Device-to-device field transfers (seigen_hip.h sg_get_field_dev / sg_set_field_dev / sg_get_spectrum_dev; kernels_xfer.hip):
// the launch plan of one transfer of `ncells` cells from `cell0`, for the launch wrapper (devxfer.cpp) and sg_xfer_plan alike.
// For one item (cube group, class) the device side is one block [row = node * ncomp + comp][lane < gw], the caller's side gw
// runs of rows = nd * ncomp words, one per cube: a [rows][gw] <-> [gw][rows] transpose per item, which a workgroup does for a
// SLICE of rows_per_slice rows at a time through an LDS image [row][pitch = gw + 1] in the block's word size.  The items are
// all classes of the groups that hold the first and the last cell of the range; a lane whose cell is outside the range (or
// is layout padding) moves nothing.  gw = 1: the layouts coincide, an item is a cell, no LDS - a flat pass of 256-word
// chunks.  The grid strides over the units (item, slice), or the chunks, beyond its cap.
static constexpr int64_t XFER_GRID_CAP = SG_XFER_GRID_CAP;
static constexpr int64_t XFER_LDS_BUDGET = 32768;   // of the 64 KB a block gets without an attribute: two slices of a P4 stress item, four blocks a CU
static constexpr int XFER_THREADS = 256;
struct XferPlan {
  int64_t item0 = 0, nitems = 0;   // items item0 .. item0 + nitems - 1
  int64_t rows = 0;                // nd * ncomp
  int64_t rows_per_slice = 0, slices = 0;   // slice s of an item: rows s * rows_per_slice .. min(rows, (s + 1) * rows_per_slice) - 1
  int64_t pitch = 0;               // words of an LDS row
  int64_t units = 0;               // nitems * slices; gw = 1: chunks of XFER_THREADS words
  int64_t grid = 0;                // blocks of XFER_THREADS threads, 0: nothing to move
  int64_t lds_bytes = 0;
};
inline XferPlan xfer_plan(int gw, int ncls, int nd, int ncomp, int dev_bytes, int64_t cell0, int64_t ncells) {
  XferPlan p;
  p.rows = (int64_t)nd * ncomp;
  if (ncells <= 0) return p;
  if (gw == 1) {
    p.item0 = cell0;
    p.nitems = ncells;
    p.rows_per_slice = p.rows;
    p.slices = 1;
    p.units = (ncells * p.rows + XFER_THREADS - 1) / XFER_THREADS;
  } else {
    const int64_t g0 = cell0 / ncls / gw, g1 = (cell0 + ncells - 1) / ncls / gw;
    p.item0 = g0 * ncls;
    p.nitems = (g1 - g0 + 1) * ncls;
    p.pitch = gw + 1;
    const int64_t fit = std::max<int64_t>(1, XFER_LDS_BUDGET / (p.pitch * dev_bytes));
    p.slices = (p.rows + fit - 1) / fit;
    p.rows_per_slice = (p.rows + p.slices - 1) / p.slices;
    p.slices = (p.rows + p.rows_per_slice - 1) / p.rows_per_slice;
    p.units = p.nitems * p.slices;
    p.lds_bytes = p.rows_per_slice * p.pitch * dev_bytes;
  }
  p.grid = std::min(p.units, XFER_GRID_CAP);
  return p;
}

// The gradient (seigen_hip.h sg_get_gradient_dev; grad.cpp, kernels_grad.hip): the broken gradient of a velocity field at the
// nodes.  Components of a kind (0 gradient, 1 divergence, 2 curl, 3 symmetric strain rate), 0: the kind does not exist there.
inline int grad_ncomp(int dim, int kind) {
  if (dim < 1 || dim > 3) return 0;
  if (kind == 0 || kind == 3) return dim * dim;
  if (kind == 1) return 1;
  if (kind == 2) return dim == 3 ? 3 : (dim == 2 ? 1 : 0);
  return 0;
}
// C[r][a][b] = d(phi_b)/d(xi_r) at the reference point of node a, dense for both cell kinds: refelem.hpp tabulate_grad at the
// lattice points a / P.  On a tensor-product cell the entries of the line through a along axis r are the 1-D derivative
// matrix C1[a_r][b_r] (the other 1-D factors are 1 at their own node), which is rows 0 .. P of C[0]: C1[al][be] = C[0][al][be].
inline std::vector<double> grad_dense_tables(int kind, int dim, int P, const std::vector<int>& lattice) {
  const int nd = (int)lattice.size() / dim;
  std::vector<double> xi((size_t)nd * dim), dphi((size_t)nd * nd * dim), C((size_t)dim * nd * nd);
  for (size_t k = 0; k < xi.size(); ++k) xi[k] = (double)lattice[k] / (double)P;
  sg::tabulate_grad(dim, P, nd, xi.data(), dphi.data(), kind);
  for (int r = 0; r < dim; ++r)
    for (int a = 0; a < nd; ++a)
      for (int b = 0; b < nd; ++b) C[((size_t)r * nd + a) * nd + b] = dphi[((size_t)a * nd + b) * dim + r];
  return C;
}
// The launch plan of one call, for the launch wrapper (grad.cpp) and sg_gradient_plan alike.  The items and the lanes that
// move nothing are those of xfer_plan.  A workgroup takes a UNIT (item, slice of nodes_per_slice output nodes): the item's whole
// velocity block [nd * dim rows][gw] as an LDS image of doubles, pitch gw + 1, and behind it (from the next multiple of 16
// bytes) the image of the slice's values [nodes_per_slice * ncomp rows][pitch]; both within GRAD_LDS_BUDGET, so that two
// workgroups fit a CU.  gw = 1: a thread per (cell, node), no LDS, chunks of GRAD_THREADS threads.  The grid strides over the
// units, or chunks, beyond its cap.  (The images are doubles whatever the block's and the caller's word sizes.)
static constexpr int64_t GRAD_LDS_BUDGET = 65536;
static constexpr int GRAD_THREADS = 256;
struct GradPlan {
  int64_t item0 = 0, nitems = 0;
  int64_t nodes_per_slice = 0, slices = 0;   // slice s: nodes s * nodes_per_slice .. min(nd, (s + 1) * nodes_per_slice) - 1
  int64_t pitch = 0;
  int64_t out_offset = 0;                    // bytes from the LDS base to the image of the values
  int64_t units = 0, grid = 0, lds_bytes = 0;
  bool ok = true;                            // false: not even one node's values fit beside the input image
};
inline GradPlan grad_plan(int gw, int ncls, int nd, int dim, int ncomp, int64_t cell0, int64_t ncells) {
  GradPlan p;
  if (ncells <= 0) return p;
  if (gw == 1) {
    p.item0 = cell0;
    p.nitems = ncells;
    p.nodes_per_slice = nd;
    p.slices = 1;
    p.units = (ncells * nd + GRAD_THREADS - 1) / GRAD_THREADS;
  } else {
    const int64_t g0 = cell0 / ncls / gw, g1 = (cell0 + ncells - 1) / ncls / gw;
    p.item0 = g0 * ncls;
    p.nitems = (g1 - g0 + 1) * ncls;
    p.pitch = gw + 1;
    const int64_t row = p.pitch * (int64_t)sizeof(double);
    p.out_offset = ((int64_t)nd * dim * row + 15) / 16 * 16;
    const int64_t fit = (GRAD_LDS_BUDGET - p.out_offset) / (ncomp * row);
    if (fit < 1) {
      p.ok = false;
      return p;
    }
    p.slices = (nd + fit - 1) / fit;
    p.nodes_per_slice = (nd + p.slices - 1) / p.slices;
    p.slices = (nd + p.nodes_per_slice - 1) / p.nodes_per_slice;
    p.units = p.nitems * p.slices;
    p.lds_bytes = p.out_offset + p.nodes_per_slice * ncomp * row;
  }
  p.grid = std::min(p.units, XFER_GRID_CAP);
  return p;
}

// Frames (seigen_hip.h sg_get_frame_dev; frame.cpp, kernels_frame.hip): a field rastered on a pixel lattice commensurate with
// the block's cubes.  Along a FREE axis a every cube holds m[a] pixels, pixel j of a cube at the cube fraction (j + 1/2) / m[a];
// a FIXED axis is the single plane x_a = at[a]: one layer of cubes and one fraction in it.  The Q = prod m[a] (free axes)
// in-cube pixels have the same cell class and reference coordinates in every cube, so the weights are one table [Q][nd].
// frame_plan states, for the launch wrapper and sg_frame_plan alike, the extents, the fractions, whether this block holds the
// layer of every fixed axis, the listed GROUPS of gw cubes (those with a cube in the layer; all of them without a fixed axis)
// and the launch: a wave takes 64 cubes - 64 / gw listed groups - of one class and one output component at a time (gw = 1: a
// thread per (listed cube, in-cube pixel)), the component is the grid's second dimension, the first strides over the rest
// beyond its cap.
static constexpr int FRAME_MAX_M = 8, FRAME_MAX_Q = 64, FRAME_THREADS = 256;
static constexpr int64_t FRAME_GRID_CAP = SG_FRAME_GRID_CAP;
struct FramePlan {
  int dim = 0, gw = 1, ncls = 1;
  int32_t m[3] = {1, 1, 1};       // in-cube pixels per axis (1 along a fixed axis and beyond dim)
  int32_t fixed[3] = {0, 0, 0};
  int32_t layer[3] = {-1, -1, -1};   // block-local cube layer of a fixed axis; -1: a free axis
  double t_fixed[3] = {0, 0, 0};  // the cube fraction of a fixed axis
  int64_t P[3] = {1, 1, 1};       // extents in pixels
  int Q = 1;
  bool owns = false;              // every fixed axis' layer lies in this block
  std::vector<int32_t> groups;    // listed groups, ascending (empty where !owns)
  int64_t units = 0;              // waves' (chunk of 64 cubes, class) units; gw = 1: (listed cube, in-cube pixel) threads
  int64_t grid = 0;               // blocks of FRAME_THREADS threads along x (0: nothing to launch)
  std::string err;                // why the frame is refused (then nothing else is valid)
  // the cube fraction of in-cube pixel q along axis a, and q's digit there
  int digit(int q, int a) const { return a == 0 ? q % m[0] : (a == 1 ? q / m[0] % m[1] : q / (m[0] * m[1])); }
  double fraction(int q, int a) const { return fixed[a] ? t_fixed[a] : ((double)digit(q, a) + 0.5) / (double)m[a]; }
};
FramePlan frame_plan(const sg_config& cfg, int gw, int ncls, const sg_frame& fr);
// cls[Q], xi[Q][dim], phi[Q][nd] of the plan's in-cube pixels: locate_point on the unit block of the configuration's cell kind
// (n = 1, h = 1, origin = 0, cube0 = 0) at the pixel's cube fractions, and the receivers' tabulate at those coordinates.
// False (with *err) where a pixel lies in no class.
bool frame_weights(const sg_config& cfg, int degree, const FramePlan& p, int32_t* cls, double* xi, double* phi, std::string* err);
