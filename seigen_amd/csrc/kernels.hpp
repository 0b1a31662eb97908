// Launch interface between the C-ABI host code (api.cpp, transfer.cpp, stages.cpp) and the HIP kernels.
#pragma once
#include <cstdint>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/seigen_hip.h"
#include "mesh_tables.hpp"

namespace sg {

// SG_REGION_FIRST of a 3-D block with neighbours on all six sides = half of the interior + six shell slabs
constexpr int SG_MAX_BOXES = 7;

// Node / facet counts of the P_k simplex element, shared by the three kernel families
// (kernels.hip `Geo`, kernels_lane.hip `LG`, kernels_mfma.hip `MG`).
// TP = 1: the tensor-product element on quadrilaterals (DIM = 2; generic kernels only).
template <int DIM, int P, int TP = 0>
struct ElemDims {
  static constexpr int ND = TP ? (DIM == 3 ? (P + 1) * (P + 1) * (P + 1) : (P + 1) * (P + 1))
                               : (DIM == 1) ? (P + 1) : (DIM == 2) ? (P + 1) * (P + 2) / 2 : (P + 1) * (P + 2) * (P + 3) / 6;
  static constexpr int NF = (DIM == 1) ? 1 : (DIM == 2) ? (P + 1) : (TP ? (P + 1) * (P + 1) : (P + 1) * (P + 2) / 2);
  static constexpr int NFACES = TP ? 2 * DIM : DIM + 1;
  static constexpr int NCLS = TP ? 1 : (DIM == 1) ? 1 : (DIM == 2) ? 2 : 6;
};

// What the MFMA stage kernels need to know about the mesh, laid out for SCALAR loads: everything is uniform over
// a wave (an item is 16 cells of one class), the per-class part is contiguous (one batch of s_load's at an offset
// that depends only on the class), and the per-lane node tables are packed four byte entries to a word - lane
// group q = lane >> 4 extracts row 4 ks + q with one v_bfe.  The first MFMA kernels read these from a copy of
// MeshDev in LDS: about 45 DEPENDENT ds_read / s_waitcnt round trips per item in front of the first trace load
// (tools/wave_sim.py, profiles/r03/kernel_experiments.txt) - the lesson of the 2-D tile kernels' T2Const.
constexpr int MK_KSF = 4;     // facet k-steps at degree 4 (15 facet nodes)
constexpr int MK_KS = 9;      // volume k-steps at degree 4 (35 nodes)
#ifndef SG_GQ_FROM_DEGREE
#define SG_GQ_FROM_DEGREE 4   // G stages with the factorised volume term (mfma_stage_G<.., FACT = 1>) from this degree on, unless SEIGEN_HIP_GQ says otherwise
#endif
struct MfmaClassConst {
  int32_t nb_axis[4], nb_dir[4], nb_cls[4];
  int32_t slot_ord[4];        // ordinal of the matching facet among the neighbour cube's facets on that side
  uint32_t nbw[4][MK_KSF];    // [f][ks] byte q: neighbour ELEMENT node matching my facet node 4 ks + q (MeshDev::nb_node)
  uint32_t nfw[4][MK_KSF];    // same, as position in the neighbour's facet list (MeshDev::nb_fnode)
  int32_t nb_face[4];         // neighbour's local facet (MeshDev::nb_face)
  // What mfma_trace_lines found, in the FIXED axis order (no kernel reads these any more - the F stages read cf_tr / cf_cn
  // below; they stay as the record of the check mfma_class_frame builds on, walked by tools/host_asan_driver.cpp, and cost
  // 288 bytes of a table that is read by scalar loads of the used words only):
  // the stress lines facet f's scaled normal can see: the columns j with (c n)_j != 0 in
  // ascending order ([1] = -1 on a cube-face facet, which has one), offset of the line of T(i, tr_col[c]) in values of the
  // field type [storage 0: full tensor, 1: symmetric][f][3 c + i] (c = 1 repeats c = 0 where there is no second column),
  // and (c n) at those columns (0 for the missing one)
  int32_t tr_col[4][2];
  int32_t tr_line[2][4][6];
  double tr_cn[4][2];
  // F stages: the class in its own axis order (mfma_class_frame).  p: the class's permutation of the axes; register i' of a
  // vector holds component p[i'], register slot (a, b) of a tensor holds T(p[a], p[b]).  Line offsets in values of the field
  // type (slot * 16):
  //   cf_vel[i']: component p[i'] of a velocity node;
  //   cf_own[storage][3 a + b]: T(p[a], p[b]) of a stress node (symmetric storage: the same line for (a, b) and (b, a));
  //   cf_tr[storage][f][c]: the neighbour lines of facet f in the order load_trace_face / load_trace_inner read them -
  //     cube face (f = 0: column p[0], f = 3: column p[2]): c = i' < 3, T(p[i'], column);
  //     inner facet, symmetric storage: the five lines its two columns see, T'(0,0) T'(0,1) T'(1,1) T'(2,0) T'(2,1) on facet 1
  //       (columns 0, 1 of the frame) and the mirror set T'(2,2) T'(2,1) T'(1,1) T'(0,2) T'(0,1) on facet 2 (columns 2, 1);
  //     inner facet, full storage: c = i': T(p[i'], lower column), c = 3 + i': T(p[i'], upper column);
  //     (entries the kernels do not read repeat entry 0).
  // cf_s[m] = 1 / h[p[m]]: J^-1 is the bidiagonal s_r e_p[r] - s_{r+1} e_p[r+1] in this order.
  // cf_cn[f]: (c n)_f at its non-zero columns of the frame, {0} {0, 1} {1, 2} {2} for f = 0 .. 3 (second entry 0 on a cube face).
  int32_t cf_p[3];
  int32_t cf_vel[3];
  int32_t cf_own[2][9];
  int32_t cf_tr[2][4][6];
  double cf_s[3];
  double cf_cn[4][2];
};
// The second rule the F stage kernels are written to (kernels_mfma.hip do_volume, do_lifts), stated once: class k is the
// reference simplex with the axes permuted by p (mesh_tables.cpp class_vertices), so with s_m = 1 / h[p[m]]
//   row r of J^-1 = s_r e_p[r] - s_{r+1} e_p[r+1] (r = 0, 1), s_2 e_p[2] (r = 2), every other entry exactly zero, and
//   (c n)_f = -1/2 grad lambda_f = (s_0 e_p[0]) / 2, -(row f - 1) / 2: non-zero at the frame's columns {0} {0,1} {1,2} {2}.
// Fills cf_* of `kc` for class k from MeshDev::Jinv and MeshDev::cn (after mfma_trace_lines, whose nb_axis rule it relies
// on); throws std::runtime_error if the tables do not have exactly this shape (sg_create then fails).
void mfma_class_frame(const MeshDev& md_host, int k, MfmaClassConst& kc);
// The rule the F stage kernels are written to (kernels_mfma.hip do_lifts), stated once: facets 0 and 3 of every class lie on
// a cube face (nb_axis >= 0) and (c n) has ONE non-zero entry, at nb_axis; facets 1 and 2 are inside the cube (nb_axis < 0)
// and (c n) has TWO; every other entry is exactly zero.  Fills tr_col / tr_line / tr_cn of `kc` for class k; throws
// std::runtime_error if the mesh tables do not have that shape (sg_create then fails: never a flux from a wrong line).
void mfma_trace_lines(const MeshDev& md_host, int k, MfmaClassConst& kc);
// line of T(i, j) in a node's nine slots: slot min * 3 + max in symmetric storage, i * 3 + j in full storage
inline int stress_line_slot(bool sym, int i, int j) { return sym ? (i < j ? i : j) * 3 + (i < j ? j : i) : i * 3 + j; }
struct MfmaConst {
  int32_t n[3];
  int32_t halo_per_cube;
  int32_t has_nbr[6];
  int32_t pad_[2];
  int64_t ncube, ncube_pad;
  uint32_t fw[4][MK_KSF];     // [f][ks] byte q: my element node of facet node 4 ks + q (MeshDev::fnode)
  MfmaClassConst cls[6];
};
MfmaConst mfma_const(const MeshDev& md_host);
// [variant 0: neighbour inside the block, 1: packed remote record, 2: domain boundary (own cell)][class][facet][lane group q][k-step]:
// offset (in values of the field type, before the component) of the neighbour's node that matches my facet node 4 ks + q -
// node * ncomp * 16 in a field, position in the facet list * 3 in a remote record; 3 * 6 * 4 * 4 * 4 entries
void mfma_trace_offsets(const MeshDev& md_host, int ncomp, std::vector<int32_t>& tab);
// [item = cell group * 6 + class][lane 0..15][facet 0..3] (see StageArgs::nbr_tab); (ncube_pad / 16) * 6 * 64 entries
void build_nbr_table(const MeshDev& md_host, std::vector<int32_t>& tab);

// scale * value rounded to double BEFORE anything is added to it: a separable source (weight x pattern) then gives
// bit for bit what a table of the products gives.  (HIP's __dmul_rn is a plain `x * y`, which hipcc contracts with
// a following add into one FMA; an instruction the optimiser cannot see into is not contracted.)
#if defined(__HIPCC__)
__host__ __device__ __forceinline__ double sg_mul_rounded(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  double p;
  asm("v_mul_f64 %0, %1, %2" : "=v"(p) : "v"(a), "v"(b));
  return p;
#else
  return a * b;   // host pass of the compiler only; never executed
#endif
}
#endif

// A source whose time slice is chosen ON THE DEVICE: a captured hipGraph freezes kernel arguments, so a launch that
// is to be replayed step after step reads the step index from a device word (bumped by a one-thread launch at the end
// of every step) instead of getting this step's slice and weight from the host (elastic.py:285-288 re-interpolates
// the source Expression before every step).
struct SrcStep {
  const int64_t* ctr;      // device word: index of the current step; null: the host chose slice and scale
  int64_t nsteps;          // steps the source covers (a step beyond them adds nothing)
  int64_t stride;          // doubles between two time slices of the value table (0: one slice for every step)
  const double* weights;   // separable source: weight per step (device), else null
  int32_t is_static;       // one slice that holds at every step
  int32_t pad_;
};

struct StageArgs {
  const double* in;    // stress for F, velocity for G           [cell][node][comp]
  double* out;         // result, or in-place target of a fused combine
  const double* aux;   // fused combine: second operand (uh1 / sh1)
  const double* uabs;  // F: velocity multiplied by the sponge (elastic.py:207-208)
  const double* ghost[6];  // packed remote facet traces of `in` per block side, or null
  const double* Dt;        // [dim][nd(b)][nd(a)]  transposed Mhat^-1 Shat_r
  const double* Lt;        // [nfaces][nf(b')][nd(a)] transposed facet lifts
  const MeshDev* md;       // device copy
  const MfmaConst* mk;     // MFMA path: device copy of mfma_const(md)
  const int32_t* ftab;     // MFMA path, F stages: trace offsets per (variant, class, facet, lane group) x 4 k-steps (mfma_trace_offsets)
  // MFMA path: where every cell finds its four facet neighbours, tabulated once per block (mfma_tables.cpp
  // build_nbr_table): nbr_tab[(item * 16 + lane) * 4 + f] = the neighbour's cell slot (cell group * 16 * 6 ... see
  // there), -1 on the domain boundary, -2 - s for slot s of the packed remote trace of that block side.  Replaces
  // the per-item recomputation (cube coordinates by division, neighbour class / axis / direction look-ups, bounds
  // tests): 256 B per item read with one 16-byte load per lane, against 76 KB of cell data.
  const int32_t* nbr_tab;
  int32_t all_active;      // the launch covers the whole block (no region boxes to test)
  int32_t tensor;          // generic path: quadrilateral cells (ElemDims<2, P, 1>) / hexahedra
  const double* fragV;     // MFMA path: volume operator fragments (mfma_tables.hpp), else null
  const double* fragL;     // MFMA path: facet-lift operator fragments
  const double* fragQ;     // MFMA path, G stages with the factorised volume term (mfma_stage_G<.., FACT = 1>): the Q tiles; fragV = the P_r tiles
  unsigned long long* dbg; // diagnostic builds (-DSG_STAMPS): per-phase cycle sums, else null
  const int32_t* sponge_slot;  // [cell] -> slot or -1 (null: no sponge)
  const double* sponge_B;      // [slot][nd(a)][nd(b)]
  const double* sponge_sigma;  // 2-D tile and 3-D MFMA kernels: [cell] 0 = no sponge; a value = sigma is CONSTANT over the cell, the sponge term is
                               // sigma u_i at the node itself and the cell has no slot; NaN = sigma varies: sponge_slot / sponge_B
  const void* sponge_pre;      // 3-D MFMA kernels: [slot][nd][dim] = B_slot u_abs of the cell, computed before the stage (launch_sponge_pre)
  const double* lam;           // per-cell (per_cell=1) or null
  const double* mu;
  double lam0, mu0;
  double c_self, c_aux, c_new;  // mode 1, F stages: out = c_self*out + c_aux*aux + c_new*rhs;  G stages: out = c_self*out + c_new*rhs
                                // (no second operand: the one fused G stage, S1, gets dt sh1 + dt^3/24 sh2 as ONE G, stages.cpp)
  // F, mode 1, per-cell density: rho2[cell][2] = {factor replacing c_self, factor multiplying c_aux and c_new}
  // (reference update: {rho, 1}; physical update: {1, 1/rho}); null: the scalars above
  const double* rho2;
  int32_t mode;                 // 0: out = rhs; 1: fused (see c_self ..); 2 (F stages): fused without the self term, out = c_aux*aux + c_new*rhs
  int32_t per_cell;
  int32_t box_o[3], box_n[3];   // region of cubes covered by this launch (generic kernel: one box per launch)
  // MFMA / lane kernels: one launch covers up to SG_MAX_BOXES disjoint boxes (a boundary shell + half an interior); `spread` deals
  // the items round-robin over all waves instead of one contiguous range per XCD, because a shell's
  // active items are a few contiguous runs that would otherwise land on one XCD
  int32_t nbox;
  int32_t boxes_o[SG_MAX_BOXES][3], boxes_n[SG_MAX_BOXES][3];
  int32_t spread;
  const int32_t* item_list;  // a region of a split stage: its active items (cell group * ncls + class), else null
  int32_t nlist;
  int32_t sym;                  // MFMA path: stress fields are symmetric, touch only the i <= j lines
  int32_t grid_blocks;          // MFMA path: size of the persistent grid (a multiple of 8)
  int32_t f32;                  // MFMA path: fields, halo buffers and operator tables are float (sg_config.dtype = 1)
  // MFMA path, whole-block launches: items are dealt to the XCDs in chunks of this many consecutive items, round-robin
  // (0: one contiguous eighth of the items per XCD).  With a chunk of 1/8 of a z-layer all XCDs sweep the block layer by
  // layer together, so the z-neighbour traces and the own rows of the next layer meet in the Infinity Cache.
  int32_t order_chunk;
  int32_t nitems;               // MFMA path: items of this launch (the item list's length, or cell groups x classes)
  // MFMA path, G stages with the factorised volume term at degree 4 (one kernel object, two forms): 1 = eight-wave blocks whose
  // lifts read the own traces out of a wave-private LDS stash, 0 = the form before it (four-wave blocks; SEIGEN_HIP_GSTASH=0)
  int32_t gstash;
  int32_t reserved_;            // unused: keeps every later member, and the tile kernels' T2Const behind StageArgs, at its kernarg offset
  // 2-D tile path, G stages: the sparse nodal source (elastic.py:217-218) added inside the stage kernel instead of
  // by a launch of its own.  src_slot[item] = slot of an item (16 cells of one class) that holds source nodes, or -1;
  // src_idx[slot][node][cell] = row of that node in this step's value table src_vals[row][dim*dim], or -1.
  const int32_t* src_slot;
  const int32_t* src_idx;
  const double* src_vals;
  double src_scale;          // factor on src_vals (a separable source's weight of this step, else 1)
  double src_coef;           // ... and on the scaled, rounded value as it enters the right-hand side (stage S1: dt + dt^3/24, else 1)
  SrcStep src_step;          // graph replay: slice and weight from the device-side step counter (ctr != null)
  int32_t src_bump;          // 2-D tile path, first stage of a step (an F stage): bump that counter (one thread)
};

// Name of a kernel as rocprofv3 prints it ("void sg::mfma_stage_G<double, 4, 0, 1, 1>(sg::StageArgs)"), from the host-side
// handle of the instantiation (kernels.hip: dladdr + demangling) - the library names its kernels itself, nobody re-derives
// template arguments from switches.
std::string kernel_name_of(const void* host_fn);

// A run-time value as a compile-time constant: f(std::integral_constant<int, V>()) for the V among V0, Vs... that equals v,
// a zero of f's result type where none does.  Every family's choice of a stage kernel is a nest of these.
template <int V0, int... Vs, typename F>
auto sg_pick(int v, F&& f) {
  decltype(f(std::integral_constant<int, V0>())) r{};
  auto take = [&](auto c) { return v == c.value && ((r = f(c)), true); };
  (void)(take(std::integral_constant<int, V0>()) || ... || take(std::integral_constant<int, Vs>()));
  return r;
}
inline int any_ghost(const StageArgs& a, int nsides) {   // blocks without neighbour blocks never meet a packed remote trace
  int g = 0;
  for (int sd = 0; sd < nsides; ++sd) g |= a.ghost[sd] != nullptr;
  return g;
}

// A stage kernel is CHOSEN first and launched second.  stage_kernel_*: the host-side handle of the instantiation that a launch
// with these arguments runs - read from kind (0 = F, velocity RHS; 1 = G, stress RHS), the degree and a.mode, a.sym, a.f32,
// a.tensor, whether a.ghost[] / a.fragQ are set - or null where the family has no such kernel; nothing is launched or asked of
// the runtime.  launch_stage_*: sizes the grid and launches the handle it is given.  kernel_name_of names the same handle.
const void* stage_kernel_generic(int kind, int dim, int P, const StageArgs& a);
int launch_stage(const void* kernel, int dim, int P, const StageArgs& a, void* stream);

// MFMA path (3-D, degree >= 3; fields in the gw = 16 interleaved layout)
int mfma_blocks_per_cu(int P, int f32);
int prepare_stage_mfma();   // once per handle, outside any stream capture: the dynamic LDS of the degree-4 G kernels' stash form; 0 on success
const void* stage_kernel_mfma(int kind, int P, const StageArgs& a);
int launch_stage_mfma(const void* kernel, const StageArgs& a, void* stream);

// lane-per-cell path (1-D / 2-D; fields in the gw = 64 interleaved layout; a.Dt = E[r][a][b],
// a.Lt = L[f][a][b'] row-major; a.tensor: hexahedra, sum-factorised, a.Dt = {D1, lift1})
const void* stage_kernel_lane(int kind, int dim, int P, const StageArgs& a);
int launch_stage_lane(const void* kernel, const StageArgs& a, long nitems, void* stream);
// hexahedra DQ_3 / DQ_4 with the lines of a cube in registers and the x lines on the matrix pipe (kernels_hexm.hip; fields
// in the gw = 16 interleaved layout; a.Dt = hexm_table(): line operators E_k, trace lifts, x-pass A operands)
int hexm_blocks_per_cu(int P);
std::vector<double> hexm_table(int P, const double* D1, const double* lift1, const MeshDev& md_host);
const void* stage_kernel_hexm(int kind, int P, const StageArgs& a);
int launch_stage_hexm(const void* kernel, int P, const StageArgs& a, long nitems, void* stream);

// 2-D MFMA tile path (P1..P4; fields in the gw = 16 interleaved layout; a.fragV / a.fragL = tile2d_frags_*).
// T2Const is the part of MeshDev these kernels use, passed by value in the kernarg segment so that no load
// depends on another one (kernels_tile2d.hip): sizes, class constants, neighbour rules, and the node
// permutations packed four byte entries to a word (entry q of word [ks] = row 4 ks + q).
// (facet arrays hold four entries: quadrilateral cells have four facets, triangles use the first three)
struct T2Class {            // everything that depends on the triangle class, contiguous: one batch of scalar loads
  double Jinv[2][2], cn[4][2];
  int32_t nb_axis[4], nb_dir[4], nb_cls[4];
  int32_t slot_ord[4];      // ordinal of the matching facet among the neighbour cube's facets on that side
  uint32_t tfw[4][2];       // neighbour ELEMENT node matching my facet node (MeshDev::nb_node)
  uint32_t tgw[4][2];       // same, as position in the neighbour's facet list (MeshDev::nb_fnode)
};
struct T2Const {
  int32_t n0, n1, ncube, ngroups;
  int32_t has_nbr[4];
  int32_t halo_per_cube;
  int32_t gpr;              // groups of 16 squares that cover at least one row of the block (+1: a group may straddle rows)
  double inv_n0;            // 1 / n0
  uint32_t tpw[4][2];       // my element node of facet node (MeshDev::fnode)
  T2Class cls[2];
};
T2Const tile2d_const(const MeshDev& md_host);
const void* stage_kernel_tile2d(int kind, int P, const StageArgs& a);
// resident: the blocks of four waves the device holds of `kernel` (asked by the caller, outside any stream capture) - the
// persistent grid where a.grid_blocks names none
int launch_stage_tile2d(const void* kernel, int resident, const StageArgs& a, const T2Const& c, long nitems, void* stream);

// host layout [cell][node][comp] <-> device layout (MeshDev::gw) for `ncells` cells from `cell0`
// dir = 0: staging -> field, 1: field -> staging
// sym = 1 (stress field in symmetric mode): a download mirrors the lower triangle from the upper;
// flag (device int, may be null): set to 1 by an upload whose tensors are not exactly symmetric
// f32 = 1: the field is float (sg_config.dtype = 1); the staging side is double either way
int launch_layout(const MeshDev& md_host, int ncomp, int dir, void* field, double* staging, int64_t cell0,
                  int64_t ncells, int sym, int* flag, int f32, void* stream);
// copy the upper triangle over the lower one in a whole stress field (leaving symmetric mode)
int launch_mirror(const MeshDev& md_host, void* field, int f32, void* stream);

// facet traces of a field on `nside` block sides -> one packed device buffer per side, one launch
// (sym = 1: a stress field stored in symmetric mode; lower-triangle values come from their mirrors)
int launch_pack(const MeshDev* md_dev, const MeshDev& md_host, const void* field, int ncomp, int nside,
                const int* sides, void* const* outs, int sym, int f32, void* stream);

// what pack_kernel (kernels.hip) takes by value: the sides of one launch, their send buffers and the facet tables
struct PackArgs {
  int nside;
  int side[6];
  void* out[6];
  int start[7];          // element ranges of the sides within the launch
  int n2[6];             // boundary cubes of each side
  int n[3], nd, nf, ncls, hpc, dim, gw;
  signed char side_cls[6][2], side_face[6][2];
  unsigned char fnode[MAX_FACES][MAX_NF + 1];
};

// field[off[k] + c*gw] += coef * values[k][c] at the sparse source nodes (off = device offset of comp 0)
// (values are scaled by `scale` and rounded first: a separable source's weight of this step)
int launch_source(void* field, int ncomp, int gw, int64_t nnz, const int64_t* offs, const double* values, double coef,
                  double scale, const SrcStep& ss, int f32, void* stream);
// sp[slot][a][i] = sum_b B[slot][a][b] u_abs[cell of slot][b][i] for the cells with a sponge matrix of their own (one block per
// cell), queued before the F stage's launches (StageArgs::sponge_pre)
// (slots: the list of slots to work on, or null = slots 0 .. nslots-1)
// (lines: sp in the layout of the fields, slot = item * gw + w - the 3-D MFMA family)
int launch_sponge_pre(const void* uabs, const double* B, const int32_t* cells, const int32_t* mats, const int32_t* slots, void* sp,
                      int32_t nslots, int nd, int dim, int ncls, int gw, int lines, int f32, void* stream);
// the same sp[slot][a][i] for the cells whose sigma is affine in the reference coordinates: B_e = s_0 I + sum_k s_k X_k with the
// element-constant X[k][a][j] (row a in ELL form: column col[a][j], or j itself where col is null), coef[slot][dim + 1] = s;
// items[n] = (cube group) * ncls + class of the n-th item that holds such a cell, item_slots[n][gw] its cells' slots (-1: none)
int launch_sponge_pre_affine(const void* uabs, const double* X, const int32_t* col, int W, const int32_t* items, const int32_t* item_slots,
                             const double* coef, void* sp, int32_t nitems, int nd, int dim, int gw, int lines, int f32, int grid, void* stream);
// (gw * nd <= SG_SPONGE_AFFINE_MAX_ROWS: the kernel's rounds of (cell, node) rows per thread; checked at set-up, sg_set_absorption)
constexpr int SG_SPONGE_AFFINE_MAX_ROWS = 8 * 256;
size_t sponge_pre_affine_lds(int W, int has_col, int nd, int dim, int gw);
// once, at set-up and outside any stream capture: allow that much dynamic LDS; returns the launch's grid on a device of ncu
// CUs (the `grid` of launch_sponge_pre_affine), <= 0 on failure
int prepare_sponge_pre_affine(int dim, int f32, size_t lds, int ncu);
// ... on the matrix pipe for the 3-D MFMA family in double (kernels_mfma.hip): fragX = mfma_frags_dense of the three X_k
int prepare_sponge_affine_mfma(int P, int ncu);   // once, at set-up: the blocks a device of ncu CUs holds (the launch's `grid`)
int launch_sponge_affine_mfma(int P, const void* uabs, const double* fragX, const int32_t* items, const int32_t* item_slots,
                              const double* coef, void* sp, int32_t nitems, int grid, void* stream);
// the device-side step counter of SrcStep: *ctr = value (add = 0) or *ctr += value (add = 1), one thread
int launch_step_counter(int64_t* ctr, int64_t value, int add, void* stream);

// Receiver samples (kernels_recv.hip): after step s (counted from the arming call) with s % every == 0, sample
// j = s / every - 1 of receiver r, component q: trace[j][r][q] = sum_a phi[r][a] field[node a][c] over a ascending, in
// double with fma (q < nu: the velocity, c = q; else the stress, c = q - nu, the (i > j) entries from their mirrors in
// symmetric mode).  Field offsets as in every layout: ((item * nd + a) * ncomp_field + c) * gw + lane.
struct RecvArgs {
  const int64_t* ctr;      // graph replay: *ctr + 1 is the step that just ended; null: `step`
  int64_t step;
  int64_t every, capacity; // (a sample index beyond the capacity is not written)
  const int64_t* item;     // [nown]
  const int32_t* lane;     // [nown]
  const double* phi;       // [nown][nd]
  double* trace;           // [capacity][nown][ncomp]
  int64_t nown;
  int32_t ncomp, nu;       // components per receiver, of which the first nu are the velocity's
  int32_t dim, nd, gw, sym;
};
int launch_receivers(const void* u, const void* s, const RecvArgs& a, int f32, void* stream);

// The monitor's sample (kernels_measure.hip; seigen_hip.h sg_measure / sg_set_monitor): { U2, S2, T2, EK, ES } of the block
// from u and s, in two passes - one partial per chunk of SG_MONITOR_CHUNK_ITEMS consecutive items, then one workgroup.
// After step s with s % every == 0 (s from *ctr + 1 under graph replay) the sample goes to out[s / every - 1]; a one-shot
// names step = every = capacity = 1.
namespace measure {
constexpr int MAX_COMP = 12;   // dim velocity components + dim^2 stress components
struct Args {
  const int64_t* ctr;      // graph replay: *ctr + 1 is the step that just ended; null: `step`
  int64_t step;
  int64_t every, capacity; // (a sample index beyond the capacity is not written)
  const double* Mtri;      // the reference mass matrix, row a: b = 0 .. a; nd (nd + 1) / 2 values
  const double* w;         // [cell][3] = (wk, ws, wt) in host cell order cube * ncls + cls, or null: w0 for every cell
  double w0[3];
  double detj;             // |det J| of every cell of the block
  double* partial;         // [nchunks][5]
  double* out;             // [capacity][5]
  int64_t nitems, ncube, nchunks;
  int32_t nd, dim, gw, ncls;
  int32_t ips;             // pass1_lds: items of a chunk worked on at a time (measure_items_per_sweep)
  int32_t ncomp;           // the components read, in this order: the velocity's, then the stress's (i <= j only in symmetric storage)
  int32_t comp[MAX_COMP];  // ... the component's index in its field
  int32_t diag[MAX_COMP];  // ... a diagonal stress component: joins the trace t
  double mult[MAX_COMP];   // ... and how often its form counts (2: an off-diagonal one in symmetric storage)
};
}  // namespace measure
// items of a chunk that the LDS-staged pass 1 holds at a time - 4, 2 or 1 (gw = 64: 1) - or 0: none fits.  The staging is
// sized for 64 KB per workgroup, 2 * nd * ips * gw doubles: every layout the library has fits (gw = 64 up to nd = 64,
// gw = 16 up to nd = 256); a layout beyond that is refused by sg_measure / sg_set_monitor ("no kernel for this element")
int measure_items_per_sweep(int nd, int gw);
// once per handle, outside any stream capture: allow pass 1 its dynamic LDS; 0 on success
int prepare_measure(int nd, int gw, int ips, int f32);
// both passes on `stream`; a.nchunks = 0 launches nothing
int launch_measure(const void* u, const void* s, const measure::Args& a, int f32, void* stream);

// The per-cell correlation of two handles' fields (kernels_xcorr.hip; seigen_hip.h sg_correlate): acc[cell][k] +=
// wd[k] * B_k of the cell, k = uu, ss, tt; one launch, no sum across cells.
namespace xcorr {
constexpr int MAX_COMP = 12;   // dim velocity components + dim^2 stress components
struct Args {
  const void* ua;          // handle a: velocity and stress
  const void* sa;
  const void* ub;          // handle b
  const void* sb;
  const double* M;         // xcorr_lds: the reference mass matrix [nd][nd]; xcorr_mfma: its A tiles (hostlogic.hpp xcorr_mass_tiles)
  double* acc;             // [ncells][3] in host cell order cube * ncls + cls
  double wd[3];            // w[k] * |det J|
  int64_t nitems, ncube;
  int32_t nd, dim, gw, ncls;
  int32_t ipw;             // xcorr_lds: items a workgroup of 64 lanes works on (xcorr_items_per_group)
  int32_t ncomp;           // hostlogic.hpp xcorr_components, in that order
  int32_t comp_a[MAX_COMP], comp_b[MAX_COMP];
  int32_t diag[MAX_COMP];
  double mult[MAX_COMP];
};
}  // namespace xcorr
// the matrix-pipe form takes this layout (the 3-D simplices at P3 / P4 in the gw = 16 layout)
inline bool xcorr_has_mfma(int dim, int nd, int gw, int tensor) { return gw == 16 && dim == 3 && !tensor && (nd == 20 || nd == 35); }
// items a workgroup of the LDS-staged form holds at a time, 4 nd ipw gw doubles in at most 64 KB and ipw gw <= 64 lanes; 0: none fits
int xcorr_items_per_group(int nd, int gw);
size_t xcorr_lds_bytes(int nd, int gw, int ipw);
// once per handle: allow the LDS-staged form its dynamic LDS (returns 1), or ask how many blocks of the matrix-pipe form a
// device of ncu CUs holds - its persistent grid, the `grid` of launch_xcorr; <= 0 on failure
int prepare_xcorr(int nd, int gw, int ipw, int mfma, int f32, int ncu);
// one launch on `stream`: the matrix-pipe form (mfma != 0; a.M = the A tiles) or the LDS-staged one (a.M = [nd][nd])
int launch_xcorr(const xcorr::Args& a, int mfma, int f32, int grid, void* stream);

// Point injectors (kernels_inject.hip; seigen_hip.h sg_inject / sg_set_injectors): at the end of step s (counted from the
// arming call; s from *ctr + 1 under graph replay) with s <= nsteps, entry k = s - 1 of the series is added.  One thread per
// (cell with points g, node a, component q): v = sum_r fma(amp[k][r][q], psi[r][a], v) from zero over the rows r = start[g] ..
// start[g + 1] - 1 in that order, then field = field + v in double, rounded once (q < nu: the velocity, c = q; else the
// stress, c = q - nu; in symmetric storage the i > j lines are left alone).  Field offsets as in every layout:
// ((item * nd + a) * ncomp_field + c) * gw + lane.  A cell appears in one group only: no two threads share a word.
namespace inject {
struct Args {
  const int64_t* ctr;      // graph replay: *ctr + 1 is the step that just ended; null: `step`
  int64_t step;
  int64_t nsteps;          // entries of the series (a step beyond them adds nothing)
  const int64_t* item;     // [ngroups]
  const int32_t* lane;     // [ngroups]
  const int64_t* start;    // [ngroups + 1]
  const double* psi;       // [nown][nd]
  const double* amp;       // [nsteps][nown][ncomp]
  int64_t ngroups, nown;
  int32_t ncomp, nu;       // components per point, of which the first nu are the velocity's
  int32_t dim, nd, gw, sym;
};
}  // namespace inject
int launch_inject(void* u, void* s, const inject::Args& a, int f32, void* stream);

// Spectra (kernels_spectra.hip; seigen_hip.h sg_set_spectra): at the end of step s (counted from the arming call; s from
// *ctr + 1 under graph replay) with s % every == 0 and j = s / every - 1 < nsamples, every word x of the field's n words
// enters acc[f][part][idx] = fma(w[j][f][part], x, acc[f][part][idx]) - but the words of the lines (idx / gw) % ncomp = i * dim + j
// with i > j where sym is set (a stress field in symmetric storage).  One flat pass over the field, of at most `grid` blocks.
namespace spectra {
struct Args {
  const int64_t* ctr;      // graph replay: *ctr + 1 is the step that just ended; null: `step`
  int64_t step;
  int64_t every, nsamples; // (a sample beyond the series adds nothing)
  const double* w;         // [nsamples][nfreq][2]
  double* acc;             // [nfreq][2][n]
  int64_t n;               // words of the field as allocated (the layout's padding included)
  int32_t nfreq;
  int32_t gw, ncomp, dim;  // the line of a word (only looked at where sym is set)
  int32_t sym;
  int32_t vec_line;        // the words of a 16-byte access lie on one line (gw is a multiple of their number)
};
}  // namespace spectra
int launch_spectra(const void* field, const spectra::Args& a, int f32, int grid, void* stream);

// Peak maps (kernels_peak.hip; seigen_hip.h sg_set_peaks): at the end of step s (counted from the arming call; s from
// *ctr + 1 under graph replay) with s % every == 0 and j = s / every - 1 < nsamples, every node word w = (item * nd + a) * gw +
// lane of the n forms m = sum_c x_c x_c over the lines ((item * nd + a) * ncomp + c) * gw + lane of `field` in double, each
// product and sum rounded on its own - in symmetric storage (sym, ncomp = dim^2) the i <= j lines, an off-diagonal one as
// 2 (x x) - and if (m > val[w]) { val[w] = m; idx[w] = j; }.  One flat pass over the node words, of at most `grid` blocks.
// The kernels take pointers and built-in scalars only.
int launch_peak_update(const void* field, double* val, int32_t* idx, const int64_t* ctr, int64_t step, int64_t every, int64_t nsamples,
                       int64_t n, int gw, int ncomp, int dim, int sym, int f32, int grid, void* stream);
// val / idx in that layout -> out_val (float where c32) / out_idx [cell][node], cell = cube * ncls + cls, the cubes of the
// layout's padding (cube >= ncube) dropped; either output may be null
int launch_peak_gather(const double* val, const int32_t* idx, void* out_val, int c32, int32_t* out_idx, int64_t n, int gw, int nd, int ncls,
                       int64_t ncube, int grid, void* stream);

// Device transfers (kernels_xfer.hip; seigen_hip.h sg_get_field_dev / sg_set_field_dev / sg_get_spectrum_dev): `ncells` cells
// from `cell0` between a buffer in the layout of the fields (`field`: float where f32) and the caller's device buffer
// [cell][node][comp] (`buf`: float where c32), by the plan of hostlogic.hpp xfer_plan (item0, units, slices, rows_per_slice,
// pitch, grid, lds_bytes).  dir = 0: buf -> field, 1: field -> buf.  sym and flag as launch_layout's.
int launch_xfer(int gw, int ncls, int nd, int ncomp, int dim, int dir, void* field, void* buf, int64_t cell0, int64_t ncells,
                int sym, int* flag, int f32, int c32, int64_t item0, int64_t units, int slices, int rows_per_slice, int pitch,
                int grid, size_t lds_bytes, void* stream);

// Frames (kernels_frame.hip; seigen_hip.h sg_get_frame_dev): one field rastered on the pixel lattice of hostlogic.hpp FramePlan.
// In-cube pixel q = j0 + m0 * (j1 + m1 * j2) of cube (c0, c1, c2) is output pixel p_a = fixed[a] ? 0 : c_a * m[a] + j_a and
//   out[c * stride[0] + p2 * stride[1] + p1 * stride[2] + p0 * stride[3]] = sum_a phi[q][a] field[cell(cube, cls[q])][a][c']
// over a ascending, in double with fma from zero (c' = c, or the mirror of an (i > j) stress entry where sym).
// What a frame specification fixes for every launch lives on the device beside its tables (the kernels take plain pointers
// and scalars: nothing by value but those):
struct FrameSpec {
  int64_t ngroups;         // the listed groups of gw cubes
  int64_t units;           // gw > 1: (chunk of 64 / gw listed groups, class); gw = 1: (listed cube, in-cube pixel)
  int64_t ncube;
  int32_t n[3], m[3], fixed[3], layer[3];   // (n, m = 1 beyond dim)
  int32_t Q, nd, ncls, gw, dim, pad_;
};
struct FrameTablePtrs {    // device pointers, gathered for the launch wrapper
  const FrameSpec* spec;
  const int32_t* cls;      // [Q] the class of in-cube pixel q
  const int32_t* order;    // [Q] the in-cube pixels sorted by class (ascending q within a class)
  const int32_t* cstart;   // [ncls + 1] the pixels of class k are order[cstart[k] .. cstart[k + 1] - 1]
  const double* phi;       // [Q][nd]
  const int32_t* groups;   // [ngroups] ascending
};
// field: the buffer of a field with ncomp components (float where f32), out: the caller's (float where c32), stride = comp,
// axis 2, axis 1, axis 0 in elements; gw, units and grid (blocks of 256 threads along x; the grid's y is the component) are
// the plan's
int launch_frame(const void* field, void* out, const FrameTablePtrs& t, int gw, int64_t units, int ncomp, int sym,
                 const int64_t stride[4], int f32, int c32, int grid, void* stream);

// The gradient (kernels_grad.hip; seigen_hip.h sg_get_gradient_dev): the kind's ncomp values of the broken gradient of the
// velocity buffer `field` (float where f32) at every node of `ncells` cells from `cell0`, into the caller's
// out[cell][node][ncomp] (float where c32), by the plan of hostlogic.hpp grad_plan.  What a launch hands its kernel, scalar by scalar:
struct GradArgs {
  int64_t item0, units;        // gw > 1: (item, slice) units from item0; gw = 1: chunks of 256 (cell, node) threads
  int64_t cell0, ncells;
  int32_t slices, nodes_per_slice, pitch, out_offset;   // out_offset: bytes from the LDS base to the image of the values
  int32_t gw, ncls, nd, dim, ncomp, kind;
  int32_t n1;                  // tensor-product cells: P + 1, and C is the 1-D matrix [n1][n1]; simplices: 0, C dense [dim][nd][nd]
  int32_t pad_;
};
// C and J (J[cls][3][3]) are device tables of the handle (handle.hpp GradTables)
int launch_grad(const void* field, void* out, const double* C, const double* J, const GradArgs& a, int f32, int c32, int grid,
                size_t lds_bytes, void* stream);

// Gauges (kernels_gauge.hip; seigen_hip.h sg_set_gauges / sg_probe_gradient): the kind's ncomp values of the broken gradient of
// the velocity buffer `field` (float where f32) at the owned points.  After step s (counted from the arming call; s from
// *ctr + 1 under graph replay) with s % every == 0 and j = s / every - 1 < capacity, for gauge g in the cell of class cls[g]:
//   t_r[i] = sum_a D[g][r][a] * (double)field[((item[g] * nd + a) * dim + i) * gw + lane[g]]   fma from zero over a ascending
//   G_ij   = sum_r J[cls[g]][r][j] * t_r[i]                                                    fma from zero over r ascending
// and out[j][g][c] the kind's combination (kernels_grad.hip combine: the same operations in the same order).  A one-shot names
// ctr = null, step = every = capacity = 1.
namespace gauge {
constexpr int MAX_VALUES = 375;   // nd * dim of the largest element (125 nodes, 3 components): a wave's LDS slab
constexpr int GRID_CAP = 1024;    // blocks of four waves; the grid strides over the gauges beyond it
struct Args {
  const int64_t* ctr;      // graph replay: *ctr + 1 is the step that just ended; null: `step`
  int64_t step;
  int64_t every, capacity; // (a sample index beyond the capacity is not written)
  const int64_t* item;     // [nown]
  const int32_t* lane;     // [nown]
  const int32_t* cls;      // [nown]
  const double* D;         // [nown][dim][nd]
  const double* J;         // [ncls][3][3]
  double* out;             // [capacity][nown][ncomp]
  int64_t nown;
  int32_t ncomp, kind;
  int32_t dim, nd, gw, pad_;
};
}  // namespace gauge
int launch_gauges(const void* field, const gauge::Args& a, int f32, void* stream);


}  // namespace sg
