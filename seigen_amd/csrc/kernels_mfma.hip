// MFMA stage kernels for 3-D, degree >= 3 (gfx950, FP64).
//
// Layout (mesh_tables.hpp): 16 cubes' cells of one simplex class are interleaved
// so that the 16 values of one (node, component) form one 128-byte line.  One
// wavefront owns one such 16-cell group at a time.  The dense element-local
// contractions of seigen/elastic.py:204-219 (+ the element mass inverse,
// :358-367) become v_mfma_f64_16x16x4_f64 products
//
//     [reference operator tile 16x4]  x  [4 nodes x 16 cells]  ->  [16 rows x 16 cells]
//
// with the cells on the MFMA N (column) axis: lane l holds column (l & 15) =
// cell, and k / row-quad (l >> 4).  The B operand rows and the accumulator
// rows are exactly the 128-byte lines of the layout, so operands are loaded
// from and results stored to HBM/L2 directly in fragment form - no LDS staging
// of cell data.  The operator tiles live in LDS in lane order (mfma_tables.cpp).
// The nd % 16 rows left over by the 16-row tiles use v_mfma_f64_4x4x4_4b_f64 (MFMA4 below).
//
// Loads are software-pipelined by hand (PF k-steps ahead): hipcc otherwise issues
// each B operand right before the MFMA that consumes it and waits for it.
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace sg {

// The kernels are written once for the field type R: double (the parity and headline mode) or float
// (the second mode of SURVEY 8d: FP32 storage and arithmetic, 32 B per DoF-update).  What differs:
//   double: v_mfma_f64_16x16x4_f64 (C/D row = 4 reg + (lane >> 4)) for full 16-row tiles and
//           v_mfma_f64_4x4x4_4b_f64 for the nd % 16 rows left over;
//   float:  v_mfma_f32_16x16x4_f32 (C/D row = 4 (lane >> 4) + reg) for every row tile, the last one
//           zero-padded (gfx950 has no 4-row f32 shape with K = 4).  The operator tiles of the float
//           tables have their rows permuted (mfma_tables.cpp) so that register `reg` of lane group q
//           holds node 16 t + 4 reg + q in both cases and everything below is type-independent.
template <typename R>
struct RT;
template <>
struct RT<double> {
  typedef double v4 __attribute__((ext_vector_type(4)));
  static constexpr bool SMALL = true;
  static __device__ __forceinline__ v4 big(double a, double b, v4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
  // 4 rows x 16 cells (four 4x4 blocks), same B register as the large shape; lane l of the result holds
  // row (l >> 4) of cell (l & 15).  About 1/6 of the issue time of the large shape (mfma_tables.hpp).
  static __device__ __forceinline__ double small(double a, double b, double c) { return __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, c, 0, 0, 0); }
};
template <>
struct RT<float> {
  typedef float v4 __attribute__((ext_vector_type(4)));
  static constexpr bool SMALL = false;
  static __device__ __forceinline__ v4 big(float a, float b, v4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
  static __device__ __forceinline__ float small(float, float, float c) { return c; }  // never reached (NSM = 0)
};

// Resident blocks per CU every instantiation of a (type, degree) must fit (launch bound) and the persistent grid is
// sized for (mfma_blocks_per_cu): registers and LDS allow exactly two at degrees 3 and 4 (a third block at degree 3 measured
// slower); the low orders are memory-bound and light (12 / 28 KB of tiles) and want more waves in flight.  One number for
// both: a grid sized for more blocks than a fused instantiation can hold runs a second, partly empty round.
template <typename R, int P>
constexpr int mfma_resident_blocks() {
  return sizeof(R) == 4 ? 3 : (P == 1 ? 4 : (P == 2 ? 3 : 2));   // float kernels: at most 168 VGPRs and half the table bytes
}

template <int P, typename R>
struct MG {
  static constexpr int ND = ElemDims<3, P>::ND;
  static constexpr int NF = ElemDims<3, P>::NF;
  static constexpr int KS = (ND + 3) / 4;
  static constexpr int KSF = (NF + 3) / 4;
  static constexpr int MTF = RT<R>::SMALL ? ND / 16 : (ND + 15) / 16;        // 16-row tiles over the nodes
  static constexpr int NSM = RT<R>::SMALL ? (ND % 16 + 3) / 4 : 0;            // 4-row tiles (4x4x4 MFMA) over the remaining rows
  static constexpr int MTT = MTF + NSM;
  static constexpr int MTFA = MTF > 0 ? MTF : 1;     // array extent (degrees 1 and 2 have no full tile)
  static constexpr int NSMA = NSM > 0 ? NSM : 1;
  static constexpr int S4 = (ND + 3) / 4;
  static constexpr int NFRAG_F = MTT * 3 * KS;
  static constexpr int NFRAG_G = 3 * MTT * KS;
  static constexpr int NFRAG_L = 4 * MTT * KSF;
  // factorised G volume (mfma_tables.hpp MfmaFactGeom): rank of the D_r = dim P_{p-1}, row tiles of Q, k-steps over the rank
  static constexpr int RK = (P >= 2) ? ElemDims<3, (P >= 2 ? P - 1 : 1)>::ND : 1;
  static constexpr int QLT = RK / 16;
  static constexpr int QST = (RK % 16 + 3) / 4;
  static constexpr int KR = (RK + 3) / 4;
  static constexpr int NFRAG_Q = (QLT + QST) * KS;
  static constexpr int NFRAG_P = 3 * MTT * KR;
};

// G stages at degree 4 in double, factorised volume term (FACT = 1): ONE block of eight waves per CU instead of two of four,
// so that the waves share one copy of the operator tiles and the LDS that frees holds a wave-private copy ("stash") of
// the own cell's rows, from which the lifts take their own traces (stage_G_body).  The form before it - four-wave blocks,
// own traces from memory - stays in the same kernel objects for comparisons (mfma_stage_G, SEIGEN_HIP_GSTASH=0); degree 3
// has only that form.
template <typename R, int P, int FACT>
constexpr bool g_stash() {
  return sizeof(R) == 8 && P == 4 && FACT == 1;
}
// Operator tiles of a stash kernel in LDS: the 16-row tiles as they come (64 doubles in lane order), then the 4-row
// tiles COMPACT: the A operand of the 4x4x4 shape is one 4x4 tile replicated over the four blocks of cells (lane l holds
// A[l & 3][l >> 4], mfma_tables.hpp), so 16 doubles hold it - entry (l & 3) + 4 (l >> 4), read by every lane with one
// broadcast ds_read_b64.  Tables of NOUT operators x (LT large + ST small row tiles) x NKS k-steps, fragment order
// ((o * (LT + ST) + t) * NKS + ks) in memory.
template <int NOUT, int LT, int ST, int NKS>
struct CompactTiles {
  static constexpr int NL = NOUT * LT * NKS * 64, NS = NOUT * ST * NKS * 16, N = NL + NS;
  static constexpr int at(int o, int t, int ks) {
    return t < LT ? ((o * LT + t) * NKS + ks) * 64 : NL + ((o * ST + (t - LT)) * NKS + ks) * 16;
  }
};
constexpr int G_STASH_SLOTS = 36;    // node rows a wave stashes per component: 35 nodes + the clamped row of the last k-step
constexpr int G_STASH_WAVES = 8;
// Dynamic LDS of a g_stash kernel, in bytes from its start: the MeshDev copy, (STASH) the facet-node offsets, the P_r, Q and
// lift tiles, (STASH) the eight stashes.  At degree 4:
//   STASH = 1   4 320 + 256 + 41 472 (71 tiles x 512 + 40 x 128) + 8 x 13 824 = 156 640 of the CU's 163 840: one block
//   STASH = 0   4 320 + 56 832 (111 tiles x 512)                              =  61 152: two blocks
template <typename R, int P, int STASH>
struct GLds {
  using M = MG<P, R>;
  static constexpr int STW = 3 * G_STASH_SLOTS * 16;
  static constexpr int OFF_FO = ((int)sizeof(MeshDev) + 15) / 16 * 16;
  static constexpr int OFF_AV = OFF_FO + (STASH ? 64 * (int)sizeof(int) : 0);
  static constexpr int OFF_Q = OFF_AV + (int)sizeof(R) * (STASH ? CompactTiles<3, M::MTF, M::NSM, M::KR>::N : M::NFRAG_P * 64);
  static constexpr int OFF_AL = OFF_Q + (int)sizeof(R) * (STASH ? CompactTiles<1, M::QLT, M::QST, M::KS>::N : M::NFRAG_Q * 64);
  static constexpr int OFF_ST = OFF_AL + (int)sizeof(R) * (STASH ? CompactTiles<4, M::MTF, M::NSM, M::KSF>::N : M::NFRAG_L * 64);
  static constexpr int BYTES = OFF_ST + (STASH ? G_STASH_WAVES * STW * (int)sizeof(R) : 0);
};

// Streaming accesses: old values of the fused combine and all results are touched once per launch; the
// non-temporal hint keeps them from displacing the cell data that the neighbours' lift phases are about to ask
// the L2 for: fabric reads -4 % (F) to -23 % (G<4,0>), step time -2 %.  (The same hint on the trace loads
// themselves changes no traffic and costs time; variants are tools/experiments/kernels_mfma_switches.patch.)
#define LD_STREAM(p) __builtin_nontemporal_load(p)
#define ST_STREAM(p, v) __builtin_nontemporal_store((v), (p))
// A wave raises its issue priority for its MFMA phases (volume, lifts) and drops it for the epilogue,
// so that the other wave of the SIMD cannot hold up matrix instructions with its loads and stores
// (+1 % on the step).
#define SG_PRIO(p) __builtin_amdgcn_s_setprio(p)
// Issue priorities per phase, one hex digit each: 0xVLE = volume, lifts, epilogue; per kernel (F / G, plain / fused).
// The lift phase is the one that waits for memory (neighbour traces) and has little matrix work per load; the volume
// phase has matrix work in abundance.  With the lifts ABOVE the volume a wave in its lifts gets its few matrix
// instructions issued the moment their operands arrive and the SIMD's other wave fills the gaps from its volume
// phase, instead of both waves queueing at equal priority: round 2's 0x330 -> 0x120 is 2-4 % on the step
// (profiles/r03/priority_sweep.txt: plain stages 1.22-1.28 -> 1.17-1.20 ms; the fused G stage does not care; the
// fused F stage, bandwidth-bound, wants the opposite order once the neighbours come from the table: 0x320).
// Round 5: stage UTEMP (F, MODE 2: reads u1 beside its result) sides with the fused F stage, 1.284 -> 1.270 ms; the fused G
// stage (S1 = s0 + g(w)) still does not care (0x320 / 0x210: +2 % on that stage).
constexpr int SG_PRIO_F0 = 0x120, SG_PRIO_F1 = 0x320, SG_PRIO_F2 = 0x320, SG_PRIO_G0 = 0x120, SG_PRIO_G1 = 0x120;
#define SG_PRIO_VOL ((PRIO3 >> 8) & 3)
#define SG_PRIO_LIFT ((PRIO3 >> 4) & 3)
#define SG_PRIO_EPI (PRIO3 & 3)
#define MFMA64(a, b, c) RT<R>::big((a), (b), (c))
#define MFMA4(a, b, c) RT<R>::small((a), (b), (c))

// Diagnostic build only (-DSG_STAMPS, SEIGEN_HIP_STAMPS=1): cycle stamps at the phase boundaries
// of an item, summed per wave in scalars and added to A.dbg at the end.  Never in the shipped build.
#ifdef SG_STAMPS
#define STAMP(t)                                                                   \
  do {                                                                             \
    __builtin_amdgcn_sched_barrier(0);                                             \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");       \
    __builtin_amdgcn_sched_barrier(0);                                             \
  } while (0)
#define STAMP_DECL unsigned long long st0 = 0, st1 = 0, st2 = 0, st3 = 0, st4 = 0, sta = 0, stb = 0, sacc[4] = {0, 0, 0, 0}, ssub[3] = {0, 0, 0}, sitems = 0
#define STAMP_ACC                                                                  \
  do {                                                                             \
    sacc[0] += st1 - st0;                                                          \
    sacc[1] += st2 - st1;                                                          \
    sacc[2] += st3 - st2;                                                          \
    sacc[3] += st4 - st3;                                                          \
    if (sta) { ssub[0] += sta - st2; ssub[1] += stb - sta; ssub[2] += st3 - stb; } \
    sitems += 1;                                                                   \
  } while (0)
#define STAMP_FLUSH                                                                \
  do {                                                                             \
    if (A.dbg && lane == 0) {                                                      \
      for (int z = 0; z < 4; ++z) atomicAdd(&A.dbg[z], sacc[z]);                   \
      atomicAdd(&A.dbg[4], sitems);                                                \
      for (int z = 0; z < 3; ++z) atomicAdd(&A.dbg[5 + z], ssub[z]);               \
    }                                                                              \
  } while (0)
#else
#define STAMP(t) do { } while (0)
#define STAMP_DECL
#define STAMP_ACC do { } while (0)
#define STAMP_FLUSH do { } while (0)
#endif

// Symmetric-stress mode (SYM = 1): every stress field of the run is symmetric (g always produces
// a symmetric tensor, elastic.py:211-219; transfer.cpp checks what the user uploads), so only the six
// lines (i <= j) of each node are read and written; the other three keep their slots but are
// never touched.  Same results, 1/3 less stress traffic.
// F reads a node's tensor in its class's own axis order (kernels.hpp mfma_class_frame): T[3 a + b] = T(p[a], p[b]), the
// line of slot (a, b) at the wave-uniform offset ol[3 a + b] from the wave-uniform base pu, the lane `lane_off` of it.
// (lane_at: a 64-bit scalar base and the lane's offset in BYTES as an unsigned 32-bit value is the one address form that
// costs no vector instruction - global_load v, v_off, s[base:base+1]; an element index would be widened and shifted per load)
template <typename R>
__device__ __forceinline__ const R* lane_at(const R* pu, unsigned lane_off) {
  return reinterpret_cast<const R*>(reinterpret_cast<const char*>(pu) + lane_off * (unsigned)sizeof(R));
}
// (a base that went through an opaque scalar is typed as global memory explicitly: the optimiser can no longer infer it)
template <typename R>
__device__ __forceinline__ __attribute__((address_space(1))) R* lane_at_g(__attribute__((address_space(1))) R* pu, unsigned lane_off) {
  typedef __attribute__((address_space(1))) char gchar;
  return (__attribute__((address_space(1))) R*)((gchar*)pu + lane_off * (unsigned)sizeof(R));
}
template <int SYM, typename R>
__device__ __forceinline__ void load_tensor(const R* pu, unsigned lane_off, const int (&ol)[9], R (&T)[9]) {
  if (SYM) {
    T[0] = *lane_at(pu + ol[0], lane_off);
    T[1] = *lane_at(pu + ol[1], lane_off);
    T[2] = *lane_at(pu + ol[2], lane_off);
    T[4] = *lane_at(pu + ol[4], lane_off);
    T[5] = *lane_at(pu + ol[5], lane_off);
    T[8] = *lane_at(pu + ol[8], lane_off);
    T[3] = T[1];
    T[6] = T[2];
    T[7] = T[5];
  } else {
#pragma unroll
    for (int c = 0; c < 9; ++c) T[c] = *lane_at(pu + ol[c], lane_off);
  }
}
__device__ __forceinline__ constexpr bool upper(int ij) { return (ij / 3) <= (ij % 3); }

// Neighbour stress at one facet node: only the lines the facet's scaled normal can see.  The flux is (c n)_j T_ij, and on
// the Kuhn classes (c n) has one non-zero entry on the facets that lie on a cube face (facets 0 and 3, column a = nb_axis)
// and two on the facets inside the cube (1 and 2); which ones is a property of (class, facet), tabulated on the host
// and checked at create (mfma_tables.cpp mfma_trace_lines, MfmaClassConst::tr_*).  A line that only ever meets an exact
// zero is not loaded.
// The lines are read in the class's own axis order (kernels.hpp mfma_class_frame, MfmaClassConst::cf_tr): row i' of the
// result is component p[i'], and WHICH lines a facet sees is then the same for every class - the class is in the offsets.
//   cube face: three loads, T[i'] = T(p[i'], a).  tl[i'] = offset of that line, uniform over the wave.  GHOST = 1: a lane
//     whose neighbour lives in another block reads the packed remote trace instead, whose record IS g_i = T(i, a)
//     (kernels.hip pack_one): offset gp[i'] = p[i'].  Remote records exist on these facets only.
//   else, symmetric storage: the five lines the facet's two columns see, T'(x,x) T'(x,1) T'(1,1) T'(z,x) T'(z,1) with
//     x = 0, z = 2 on facet 1 and x = 2, z = 0 on facet 2 (T' = the tensor in the frame).  (Picking five of the six lines
//     in the FIXED axis order took selected offsets and a selection of the flux rows and measured slower than the sixth
//     load, profiles/r10/f_trace_lines_variants.txt; in the frame there is nothing to select.)
//   else, full storage: six loads, T[3 c + i'] = T(p[i'], column c of the two).
// The loads stay unconditional and only their offsets are selected: a branch around them costs the F stages a factor
// two (the hand-pipelined load/MFMA interleaving is lost).
// cube face: p = the lane's neighbour (or its remote record, or its own cell on the domain boundary) at the facet node
template <int GHOST, typename R>
__device__ __forceinline__ void load_trace_face(const R* p, bool ghost, const int (&tl)[6], const int (&gp)[3], R (&T)[6]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) T[i] = p[GHOST ? (ghost ? gp[i] : tl[i]) : tl[i]];
}
// inner facet: the neighbour is another cell of the SAME cube, i.e. the same 16 lanes of another item of this cell group:
// the base of its line c is wave-uniform (pl[c], an opaque scalar each - see line_of in mfma_stage_F) and a lane adds only
// its own offset (node and cell) - no vector address arithmetic.
template <int SYM, typename R>
__device__ __forceinline__ void load_trace_inner(const __attribute__((address_space(1))) R* const (&pl)[6], unsigned lane_off, R (&T)[6]) {
#pragma unroll
  for (int c = 0; c < (SYM ? 5 : 6); ++c) T[c] = *lane_at_g(pl[c], lane_off);
}

// wave-uniform test on the bits (scalar compare and branch; there is no scalar f64 compare)
__device__ __forceinline__ bool uniform_nonzero(double c) {
  return (__builtin_bit_cast(unsigned long long, c) << 1) != 0ull;
}
__device__ __forceinline__ bool uniform_nonzero(float c) { return (__builtin_bit_cast(unsigned, c) << 1) != 0u; }

struct LaneGeo {
  long c;      // linear cube index of this lane's cell
  int cc[3];   // cube coordinates
  bool valid;  // a real cube (not layout padding)
  bool active; // valid and inside the launch's region
};

typedef __attribute__((address_space(4))) const MfmaConst cMfmaConst;
typedef __attribute__((address_space(4))) const MfmaClassConst cMfmaClassConst;

// (MD: the scalar-load copy of the mesh constants, MfmaConst, or the MeshDev copy in LDS)
template <typename MD>
__device__ __forceinline__ LaneGeo lane_geo(const MD& md, const StageArgs& A, long g, int w) {
  LaneGeo L;
  L.c = g * 16 + w;
  L.valid = L.c < md.ncube;
  // 32-bit arithmetic: a block has far fewer than 2^31 cubes (288 GB hold about 2^24 of them at
  // degree 1), and the 64-bit divisions this replaces are some hundred instructions each
  const unsigned cl = L.valid ? (unsigned)L.c : 0u;
  const unsigned n0 = (unsigned)md.n[0], n1 = (unsigned)md.n[1];
  const unsigned t = cl / n0, z = t / n1;
  L.cc[0] = (int)(cl - t * n0);
  L.cc[1] = (int)(t - z * n1);
  L.cc[2] = (int)z;
  bool in = false;
  for (int bx = 0; bx < A.nbox; ++bx) {
    bool ib = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) ib = ib && (L.cc[a] >= A.boxes_o[bx][a]) && (L.cc[a] < A.boxes_o[bx][a] + A.boxes_n[bx][a]);
    in = in || ib;
  }
  L.active = L.valid && in;
  return L;
}

// Where this lane finds its neighbour's trace across facet f.
template <typename R>
struct NbrRef {
  const R* p;  // base pointer of the neighbour cell (or ghost slot)
  int cstride;      // stride between (node, comp) entries: 16 in a field, 1 in a packed ghost buffer
  bool ghost;
  bool physical;    // domain boundary: no neighbour (p then points at the own cell)
};

// Whole-block launches test no region boxes: the cube coordinates (two integer divisions per lane) are not needed
__device__ __forceinline__ LaneGeo lane_geo_all(long ncube, long g, int w) {
  LaneGeo L;
  L.c = g * 16 + w;
  L.valid = L.c < ncube;
  L.cc[0] = L.cc[1] = L.cc[2] = 0;
  L.active = L.valid;
  return L;
}

// The four neighbours of this lane's cell from the block's table (StageArgs::nbr_tab): one 16-byte load per lane
typedef int nbr4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ nbr4 load_nbr4(const StageArgs& A, long item, int w) {
  return *reinterpret_cast<const nbr4*>(A.nbr_tab + (item * 16 + w) * 4);
}
// e: table entry of facet f; side: block side the facet crosses (wave-uniform; only used for a remote trace)
template <int ND, int NF, int NC, typename R_>
__device__ __forceinline__ NbrRef<R_> nbr_from_entry(const StageArgs& A, int e, int side, const R_* own_base) {
  NbrRef<R_> R;
  const R_* const fin = reinterpret_cast<const R_*>(A.in);
  R.cstride = 16;
  R.ghost = e < -1;
  R.physical = e == -1;
  const long slot = e < 0 ? 0 : e;
  const R_* pin = fin + ((slot >> 4) * (long)ND) * NC * 16 + (slot & 15);
  R.p = e < 0 ? own_base : pin;
  if (__any(R.ghost)) {        // blocks with neighbour blocks only, and there only the shell items
    if (R.ghost) {
      R.p = reinterpret_cast<const R_*>(A.ghost[side]) + (long)(-2 - e) * NF * 3;
      R.cstride = 1;
    }
  }
  return R;
}

// XCD-aware work split: blocks with equal blockIdx % 8 share an XCD (and its L2), so each
// label gets one contiguous range of items; a different placement only changes speed.
struct ItemRange {
  long lo, hi, step;
  long chunk, xcd, nitems;  // chunk > 0: `it` counts the XCD's own items; item_of() maps to the global item
};
__device__ __forceinline__ ItemRange item_range(long nitems, int wave, int spread, long chunk) {
  ItemRange r;
  const long wpb = blockDim.x >> 6;   // waves per block (4)
  r.chunk = 0;
  r.xcd = 0;
  r.nitems = nitems;
  if (spread) {  // boundary shells: round-robin over every wave of the grid (over the item list if given)
    r.lo = (long)blockIdx.x * wpb + wave;
    r.hi = nitems;
    r.step = (long)gridDim.x * wpb;
    return r;
  }
  const long nblk = gridDim.x;
  const long xcd = blockIdx.x % 8;
  const long slot = blockIdx.x / 8;
  const long blocks_here = (nblk - xcd + 7) / 8;
  r.step = blocks_here * wpb;
  if (chunk > 0) {
    // chunks xcd, xcd + 8, ... of `chunk` consecutive items each
    const long nchunks = (nitems + chunk - 1) / chunk;
    const long mine = (nchunks - xcd + 7) / 8;
    r.chunk = chunk;
    r.xcd = xcd;
    r.lo = slot * wpb + wave;
    r.hi = mine > 0 ? mine * chunk : 0;
    return r;
  }
  const long ipx = (nitems + 7) / 8;
  r.lo = xcd * ipx + slot * wpb + wave;
  r.hi = (xcd + 1) * ipx < nitems ? (xcd + 1) * ipx : nitems;
  return r;
}
// global item of loop index `it`, or -1 (past the end of the last chunk)
__device__ __forceinline__ long item_of(const ItemRange& r, long it) {
  if (r.chunk == 0) return it;
  const long c = it / r.chunk;
  const long item = (c * 8 + r.xcd) * r.chunk + (it - c * r.chunk);
  return item < r.nitems ? item : -1;
}

// Operator tiles and mesh tables into LDS, once per block.  All of a thread's loads are issued
// before the first one is consumed (a plain copy loop compiles to load / wait / write per element:
// 33 dependent L2 round trips, about 20 us of every launch).
template <int N, typename R, int NT = 256>
__device__ __forceinline__ void copy_to_lds(R* dst, const R* __restrict__ src) {
  constexpr int PER = (N + NT - 1) / NT;
  R v[PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int i = threadIdx.x + j * NT;
    v[j] = (i < N) ? src[i] : R(0);
  }
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int i = threadIdx.x + j * NT;
    if (i < N) dst[i] = v[j];
  }
}

// A fragment table into its CompactTiles form (all loads first, as above)
template <typename CT, int NOUT, int LT, int ST, int NKS, typename R, int NT>
__device__ __forceinline__ void copy_compact(R* dst, const R* __restrict__ src) {
  constexpr int PER = (CT::N + NT - 1) / NT;
  R v[PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int i = threadIdx.x + j * NT;
    int s = 0;
    if (i < CT::NL) {
      const int fr = i >> 6, o = fr / (LT * NKS), rem = fr - o * (LT * NKS);   // rem = t * NKS + ks, t < LT
      s = (o * (LT + ST) * NKS + rem) * 64 + (i & 63);
    } else {
      const int i2 = i - CT::NL, fr = i2 >> 4, c = i2 & 15, o = fr / (ST * NKS), rem = fr - o * (ST * NKS);
      s = (o * (LT + ST) * NKS + LT * NKS + rem) * 64 + (c & 3) + 16 * (c >> 2);     // lane (c & 3) + 16 (c >> 2) holds A[c & 3][c >> 2]
    }
    v[j] = (i < CT::N) ? src[s] : R(0);
  }
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int i = threadIdx.x + j * NT;
    if (i < CT::N) dst[i] = v[j];
  }
}

template <int NV, int NL, typename R, int NT = 256>
__device__ __forceinline__ void load_tables(R* sAV, R* sAL, const StageArgs& A) {
  copy_to_lds<NV * 64, R, NT>(sAV, reinterpret_cast<const R*>(A.fragV));
  copy_to_lds<NL * 64, R, NT>(sAL, reinterpret_cast<const R*>(A.fragL));
  __syncthreads();
}

template <int NV, int NL, typename R>
__device__ __forceinline__ void load_tables(R* sAV, R* sAL, MeshDev* sMd, const StageArgs& A) {
  const int* src = reinterpret_cast<const int*>(A.md);
  int* dst = reinterpret_cast<int*>(sMd);
  constexpr int NI = (int)(sizeof(MeshDev) / sizeof(int)), PERI = (NI + 255) / 256;
  int w[PERI];
#pragma unroll
  for (int j = 0; j < PERI; ++j) {
    const int i = threadIdx.x + j * 256;
    w[j] = (i < NI) ? src[i] : 0;
  }
  copy_to_lds<NV * 64>(sAV, reinterpret_cast<const R*>(A.fragV));
  copy_to_lds<NL * 64>(sAL, reinterpret_cast<const R*>(A.fragL));
#pragma unroll
  for (int j = 0; j < PERI; ++j) {
    const int i = threadIdx.x + j * 256;
    if (i < NI) dst[i] = w[j];
  }
  __syncthreads();
}


// (c n)_j T_ij for one row i of a tensor, in ONE fixed order of operations (not left to the contraction heuristics: a
// facet's flux must not depend on which instantiation - whole block, shell, ghost-reading - a launch happens to use).
template <typename R>
__device__ __forceinline__ R ndot(R c0, R c1, R c2, R t0, R t1, R t2) {
  R r = c0 * t0;
  r = __builtin_fma(c1, t1, r);
  r = __builtin_fma(c2, t2, r);
  return r;
}
template <>
__device__ __forceinline__ float ndot<float>(float c0, float c1, float c2, float t0, float t1, float t2) {
  float r = c0 * t0;
  r = __builtin_fmaf(c1, t1, r);
  r = __builtin_fmaf(c2, t2, r);
  return r;
}
__device__ __forceinline__ double fma_of(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ float fma_of(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

// Row i' of facet f's flux, wf (c n)_j T_ij, out of the lines load_trace_face / load_trace_inner left in T: the terms of the facet's non-zero
// columns alone - the lower column's product first, the other one added by an fma.  wc: wf (c n) at those columns in
// ascending order (MfmaClassConst::cf_cn; wf = +-1, so the products are exact and formed once per facet).
template <int SYM, typename R>
__device__ __forceinline__ R trace_flux(const int f, int i, const R (&wc)[2], const R (&T)[6]) {
  if (f == 0 || f == 3) return wc[0] * T[i];
  if (SYM) {  // T'(i', x) and T'(i', 1) are neighbours in the five lines: rows x, 1, z start at 0, 1, 3
    const int x = f == 1 ? 0 : 2;
    const int a = i == x ? 0 : (i == 1 ? 1 : 3);
    if (f == 1) return fma_of(wc[1], T[a + 1], wc[0] * T[a]);
    return fma_of(wc[1], T[a], wc[0] * T[a + 1]);
  }
  return fma_of(wc[1], T[3 + i], wc[0] * T[i]);
}


// --------------------------------------------------------------------------------------------
//  G: sh_ij = lam d_ij W_kk + mu (W_ij + W_ji),  W_ik = -Jinv_rk (D_r u_i) + sum_f (c n)_k L_f u^_i
//  Row tile t of every D_r leaves node a = 4 m + q in lane-group q (m = 4 t + reg for a large
//  tile, m = 4*MTF + s for small tile s), so the three D_r u_i of one node meet in the same lane;
//  only W_ii and W_ij + W_ji are accumulated (6 * S4 values).
// --------------------------------------------------------------------------------------------
// (FACT: the factorised volume term.  STASH: the lifts' own traces out of the wave's LDS stash, eight waves to a block.
//  DYN: the LDS is the launch's dynamic allocation, laid out by GLds - the two forms of a g_stash kernel need 61 KB and
//  153 KB and must not both be charged to every block; every other instantiation keeps its static arrays.)
template <typename R, int P, int MODE, int SYM, bool FACT, bool STASH, bool DYN>
__device__ __forceinline__ void stage_G_body(const StageArgs& A) {
  using M = MG<P, R>;
  constexpr int NT = STASH ? 512 : 256;
  typedef typename RT<R>::v4 d4;
  constexpr int PRIO3 = MODE ? SG_PRIO_G1 : SG_PRIO_G0;
  constexpr int ND = M::ND, NF = M::NF, KS = M::KS, KSF = M::KSF, MTF = M::MTF, NSM = M::NSM, MTT = M::MTT, S4 = M::S4;
  // B-operand prefetch distance, in k-steps.  A float k-step is 96 matrix cycles per component against 144 in
  // double, so the same latency needs more k-steps in flight (measured: G<float,4,0> 1.10 -> 0.97 ms with 6, 0.94 with 8,
  // which costs the fused kernel more than it gains)
  constexpr int PF = sizeof(R) == 4 ? 6 : 4;
  constexpr int QLT = M::QLT, QST = M::QST, KR = M::KR;
  // operator tiles in LDS: the row tiles of the three D_r (E_r: with the own-trace half of the flux folded in), or
  // (FACT) those of the P_r in their place (A.fragV) and the Q tiles beside them
  // STASH: one copy for eight waves, the 4-row tiles compact (CompactTiles); beside them every wave's stash of its cell
  // group's own rows, [component][node slot][16 cells], and the stash offsets of the facet nodes per (facet, lane group) x
  // four k-steps (GLds has the byte counts).
  using CP = CompactTiles<3, MTF, NSM, KR>;
  using CQ = CompactTiles<1, QLT, QST, KS>;
  using CL = CompactTiles<4, MTF, NSM, KSF>;
  using LY = GLds<R, P, STASH>;
  constexpr int STW = LY::STW;          // doubles of one wave's stash
  R *sAV = nullptr, *sQ = nullptr, *sAL = nullptr, *sSt = nullptr;
  MeshDev* sMdp = nullptr;
  int* sFo = nullptr;
  if constexpr (DYN) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sg_dyn_lds[];
    sMdp = reinterpret_cast<MeshDev*>(sg_dyn_lds);
    sFo = reinterpret_cast<int*>(sg_dyn_lds + LY::OFF_FO);
    sAV = reinterpret_cast<R*>(sg_dyn_lds + LY::OFF_AV);
    sQ = reinterpret_cast<R*>(sg_dyn_lds + LY::OFF_Q);
    sAL = reinterpret_cast<R*>(sg_dyn_lds + LY::OFF_AL);
    sSt = reinterpret_cast<R*>(sg_dyn_lds + LY::OFF_ST);
  } else {
    __shared__ R sAV_[(FACT ? M::NFRAG_P : M::NFRAG_G) * 64];
    __shared__ R sQ_[FACT ? M::NFRAG_Q * 64 : 1];
    __shared__ R sAL_[M::NFRAG_L * 64];
    __shared__ MeshDev sMd_;
    sAV = sAV_, sQ = sQ_, sAL = sAL_, sMdp = &sMd_;
  }
  MeshDev& sMd = *sMdp;
  if constexpr (STASH) {
    static_assert(ND <= G_STASH_SLOTS && 4 * KS <= G_STASH_SLOTS, "a stash slot per B row of the Q pass");
    copy_to_lds<(int)(sizeof(MeshDev) / sizeof(int)), int, NT>(reinterpret_cast<int*>(&sMd), reinterpret_cast<const int*>(A.md));
    copy_compact<CQ, 1, QLT, QST, KS, R, NT>(sQ, reinterpret_cast<const R*>(A.fragQ));
    copy_compact<CP, 3, MTF, NSM, KR, R, NT>(sAV, reinterpret_cast<const R*>(A.fragV));
    copy_compact<CL, 4, MTF, NSM, KSF, R, NT>(sAL, reinterpret_cast<const R*>(A.fragL));
    if (threadIdx.x < 64) {   // entry (f * 4 + q) * 4 + ks: byte offset of my element node of facet node 4 ks + q (padded rows: node of facet node 0, as in request)
      const int f = threadIdx.x >> 4, bq4 = 4 * (threadIdx.x & 3) + ((threadIdx.x >> 2) & 3);
      sFo[threadIdx.x] = (int)A.md->fnode[f][bq4 < NF ? bq4 : 0] * 16 * (int)sizeof(R);
    }
    __syncthreads();
  } else {
    if constexpr (FACT) copy_to_lds<M::NFRAG_Q * 64>(sQ, reinterpret_cast<const R*>(A.fragQ));
    load_tables<(FACT ? M::NFRAG_P : M::NFRAG_G), M::NFRAG_L>(sAV, sAL, &sMd, A);
  }

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int q = lane >> 4, w = lane & 15;
  // uniform reads of class constants: constant address space => s_load (scalar cache)
  typedef __attribute__((address_space(4))) const MeshDev cMeshDev;
  const cMeshDev* md = (const cMeshDev*)(unsigned long long)A.md;
  const R* __restrict__ in = reinterpret_cast<const R*>(A.in);
  R* __restrict__ out = reinterpret_cast<R*>(A.out);
  const R c_self = (R)A.c_self, c_new = (R)A.c_new;
  const long ngroups = sMd.ncube_pad >> 4;
  const ItemRange ir = item_range(A.item_list ? (long)A.nlist : ngroups * 6, wave, A.spread, A.order_chunk);

  STAMP_DECL;
  for (long it = ir.lo; it < ir.hi; it += ir.step) {
    STAMP(st0);
    const long iti = item_of(ir, it);
    if (iti < 0) continue;
    const long item = A.item_list ? (long)A.item_list[iti] : iti;
    const long g = item / 6;
    const int k = (int)(item - g * 6);
    const LaneGeo L = A.all_active ? lane_geo_all(sMd.ncube, g, w) : lane_geo(sMd, A, g, w);
    const nbr4 nbe = load_nbr4(A, item, w);
    if (!__any(L.active)) continue;
    const R* own = in + ((g * 6 + k) * (long)ND) * 3 * 16 + w;
    // B row of this lane at k-step ks = node 4 ks + q: one pointer per item plus compile-time
    // offsets (a table of per-k-step offsets is item-invariant, gets hoisted out of the item loop
    // as 64-bit values and spilled; every reload then waits for ALL loads in flight).  Only the last
    // k-step can run past ND; those rows meet all-zero operator columns, so any finite value will
    // do there: clamp instead of branching.
    int qo = q * 3 * 16;
    asm volatile("" : "+v"(qo));
    const R* ownq = own + qo;
    const R* ownl = (4 * (KS - 1) + q < ND) ? ownq + (KS - 1) * 4 * 3 * 16 : own;
    auto brow = [&](int ks) { return (ks == KS - 1) ? ownl : ownq + ks * 4 * 3 * 16; };
    // operator tiles are item-invariant: an opaque lane offset keeps the compiler from hoisting
    // all of them into registers (and, unlike a laundered pointer, keeps the reads ds_read_b64)
    int lo = lane;
    asm volatile("" : "+v"(lo));
    // STASH: a lane's entry of a compact 4-row tile; where it writes its B rows of the Q pass (k-step ks, lane group q = node
    // slot 4 ks + q: the four lane groups write four consecutive 128-byte rows) and reads the own trace of a facet node.
    // The stash belongs to the wave: writer and reader are the same wave, whose LDS operations stay in order, so no barrier
    // stands between the Q pass and the lifts or between two items - the lgkmcnt wait in front of a read's use is all.
    const int lo4 = (lo & 3) + ((lo >> 4) << 2);
    R* const stw = sSt + (STASH ? wave * STW : 0) + lo;
    const char* const str = reinterpret_cast<const char*>(sSt + (STASH ? wave * STW : 0) + (lo & 15));
    auto tile = [&](const R* tab, int full, int at, int t, int nlarge) { return STASH ? tab[at + (t < nlarge ? lo : lo4)] : tab[full * 64 + lo]; };

    R Jm[3][3], cnf[4][3];  // class constants (wave-uniform)
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int j = 0; j < 3; ++j) Jm[r][j] = (R)(-md->Jinv[k][r][j]);
#pragma unroll
    for (int f = 0; f < 4; ++f)
#pragma unroll
      for (int j = 0; j < 3; ++j) cnf[f][j] = (R)md->cn[k][f][j];

    R Sd[3][S4], So[3][S4];  // W_ii and W_ij + W_ji for (0,1), (0,2), (1,2)
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int m = 0; m < S4; ++m) Sd[i][m] = So[i][m] = R(0);

    constexpr int NB = 2;   // trace buffers: facet f in nx[f % NB], the next NB - 1 facets on their way
    constexpr int NBO = (FACT && !STASH) ? NB : 1;
    R nx[NB][KSF][3], nxo[NBO][KSF][3];   // nxo (FACT without a stash): the own traces of the same facet nodes
    auto request = [&](int f, R (&dst)[KSF][3], R (&dso)[KSF][3]) {
      const NbrRef<R> NR = nbr_from_entry<ND, NF, 3>(A, nbe[f], 2 * sMd.nb_axis[k][f] + (sMd.nb_dir[k][f] > 0 ? 1 : 0), own);
#pragma unroll
      for (int ks = 0; ks < KSF; ++ks) {
        const int bb = (4 * ks + q < NF) ? 4 * ks + q : 0;  // padded rows meet zero lift columns
        const int on = sMd.fnode[f][bb];
        const int nn = NR.ghost ? sMd.nb_fnode[k][f][bb] : (NR.physical ? on : sMd.nb_node[k][f][bb]);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          dst[ks][i] = NR.p[(nn * 3 + i) * NR.cstride];
          // FACT: u^ = 1/2 (own + neighbour) (own + own on a boundary facet), the 1/2 being part of the lift tiles.
          // Two loads per value: the own rows were read a phase ago and come out of the L2 - or (STASH) no second load: the
          // lifts read the own value out of the wave's stash when they need it.
          if constexpr (FACT && !STASH) dso[ks][i] = own[(on * 3 + i) * 16];
        }
      }
    };
    SG_PRIO(SG_PRIO_VOL);
    STAMP(st1);
    // W_ik += Jm[r][k] (D_r u_i) for the row tiles of one reference direction.  On the Kuhn classes J^-1 has five
    // non-zeros out of nine: the zero columns are skipped with a scalar branch (the class is uniform over the wave)
    auto fold_dir = [&](int r, const d4 (&acc)[M::MTFA][3], const R (&accs)[M::NSMA][3]) {
#pragma unroll
      for (int kk = 0; kk < 3; ++kk) {
        const R c = Jm[r][kk];
        if (uniform_nonzero(c)) {
#pragma unroll
          for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int t = 0; t < MTF; ++t)
#pragma unroll
              for (int reg = 0; reg < 4; ++reg) {
                if (4 * t + reg >= S4) continue;  // padded rows of the last float tile
                if (i == kk)
                  Sd[i][4 * t + reg] += c * acc[t][i][reg];
                else
                  So[i + kk - 1][4 * t + reg] += c * acc[t][i][reg];
              }
#pragma unroll
            for (int t = 0; t < NSM; ++t) {
              if (i == kk)
                Sd[i][4 * MTF + t] += c * accs[t][i];
              else
                So[i + kk - 1][4 * MTF + t] += c * accs[t][i];
            }
          }
        }
      }
      // pin the folds here: LLVM otherwise sinks these FMA chains down to the epilogue (their
      // only use), which keeps every accumulator tile live and spills
#pragma unroll
      for (int m = 0; m < S4; ++m)
#pragma unroll
        for (int i = 0; i < 3; ++i) asm volatile("" : "+v"(Sd[i][m]), "+v"(So[i][m]));
    };
    // one k-step of a direction's row tiles: acc += tile(r, t, ks) x b
    auto tiles_step = [&](int nks, int r, int ks, const R (&b)[3], d4 (&acc)[M::MTFA][3], R (&accs)[M::NSMA][3]) {
#pragma unroll
      for (int t = 0; t < MTT; ++t) {
        const R a = tile(sAV, (r * MTT + t) * nks + ks, CP::at(r, t, ks), t, MTF);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          if (t < MTF)
            acc[t < MTF ? t : 0][i] = MFMA64(a, b[i], acc[t < MTF ? t : 0][i]);
          else
            accs[t < MTF ? 0 : t - MTF][i] = MFMA4(a, b[i], accs[t < MTF ? 0 : t - MTF][i]);
        }
      }
    };
    auto clear_acc = [&](d4 (&acc)[M::MTFA][3], R (&accs)[M::NSMA][3]) {
#pragma unroll
      for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int t = 0; t < MTF; ++t) acc[t][i] = d4{0, 0, 0, 0};
#pragma unroll
        for (int t = 0; t < NSM; ++t) accs[t][i] = R(0);
      }
    };
    if constexpr (!FACT) {
      // ---- volume: B = the cells' own nodal values, straight from memory, PF k-steps ahead.
      //      One pass over the k-steps per reference direction r with all row tiles of D_r live:
      //      one load of a B row feeds 3*MTT MFMAs, and the cell data are read three times (twice
      //      through L1/L2); 3*MTF accumulator tiles + 3*NSM values are live next to Sd/So.
      constexpr int NS = 3 * KS;
      R bq[PF][3];
#pragma unroll
      for (int s = 0; s < PF; ++s)
#pragma unroll
        for (int i = 0; i < 3; ++i) bq[s][i] = brow(s % KS)[i * 16];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        d4 acc[M::MTFA][3];
        R accs[M::NSMA][3];
        clear_acc(acc, accs);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const int s = r * KS + ks;
          R b[3];
#pragma unroll
          for (int i = 0; i < 3; ++i) b[i] = bq[s % PF][i];
          if (s + PF < NS) {
#pragma unroll
            for (int i = 0; i < 3; ++i) bq[s % PF][i] = brow((s + PF) % KS)[i * 16];
          }
          tiles_step(KS, r, ks, b, acc, accs);
        }
        fold_dir(r, acc, accs);
      }
    } else {
      // ---- volume, FACTORISED (double, degrees 3 and 4; mfma_tables.hpp): the three D_r of a degree-p element
      //      differentiate, so they have rank dim P_{p-1} and share their row space: D_r = P_r Q.  y_i = Q u_i once
      //      (one pass over the own rows, PF k-steps ahead), then per reference direction z = P_r y_i with the results
      //      of the first product as B operands of the second as they are (accumulator register `reg` of a large tile
      //      = k-step `reg`; a small tile's value = its k-step): 8640 matrix cycles per 16 cells at degree 4 instead
      //      of 11664.  The price: the own-trace half of the central flux cannot stay folded into rank-deficient
      //      tiles, so the lifts take 1/2 (own + neighbour) and load the own traces as well (request).
      d4 yl[QLT > 0 ? QLT : 1][3];
      R ys[QST > 0 ? QST : 1][3];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int t = 0; t < QLT; ++t) yl[t][i] = d4{0, 0, 0, 0};
#pragma unroll
        for (int t = 0; t < QST; ++t) ys[t][i] = R(0);
      }
      R bq[PF][3];
#pragma unroll
      for (int s = 0; s < PF && s < KS; ++s)
#pragma unroll
        for (int i = 0; i < 3; ++i) bq[s][i] = brow(s)[i * 16];
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        R b[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) b[i] = bq[ks % PF][i];
        if (ks + PF < KS) {
#pragma unroll
          for (int i = 0; i < 3; ++i) bq[ks % PF][i] = brow(ks + PF)[i * 16];
        }
        if constexpr (STASH) {   // the own rows pass through the registers once, here: keep them for the lifts
#pragma unroll
          for (int i = 0; i < 3; ++i) stw[(i * G_STASH_SLOTS + 4 * ks) * 16] = b[i];
        }
#pragma unroll
        for (int t = 0; t < QLT + QST; ++t) {
          const R a = tile(sQ, t * KS + ks, CQ::at(0, t, ks), t, QLT);
#pragma unroll
          for (int i = 0; i < 3; ++i) {
            if (t < QLT)
              yl[t < QLT ? t : 0][i] = MFMA64(a, b[i], yl[t < QLT ? t : 0][i]);
            else
              ys[t < QLT ? 0 : t - QLT][i] = MFMA4(a, b[i], ys[t < QLT ? 0 : t - QLT][i]);
          }
        }
      }
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        d4 acc[M::MTFA][3];
        R accs[M::NSMA][3];
        clear_acc(acc, accs);
#pragma unroll
        for (int ks = 0; ks < KR; ++ks) {
          R b[3];
#pragma unroll
          for (int i = 0; i < 3; ++i) b[i] = (ks < 4 * QLT) ? yl[(ks / 4) < QLT ? ks / 4 : 0][i][ks % 4] : ys[(ks - 4 * QLT) >= 0 && (ks - 4 * QLT) < QST ? ks - 4 * QLT : 0][i];
          tiles_step(KR, r, ks, b, acc, accs);
        }
        fold_dir(r, acc, accs);
      }
    }

    STAMP(st2);
    // ---- facet lifts.  u^ = avg(u) on interior facets, own trace on the boundary
    //      (elastic.py:213-216).  Plain tiles: the own half of avg(u) is part of the volume tiles (E_r,
    //      mfma_tables.cpp), so the lift carries 1/2 u- on interior facets and the missing
    //      1/2 u+ on boundary facets: in both cases half of whatever np[f] points at
    //      (a boundary lane's neighbour pointer is its own cell); the 1/2 is in the lift tiles.
    //      FACT: 1/2 (own + that).
    //      Register budget: the facet's KSF*3 B values stay resident while the row tiles are
    //      accumulated one at a time (3 accumulators instead of 3*MTT); the next facet's values are
    //      requested before the last tile pass.  Row tile t covers the row-quads m = 4t .. 4t+3
    //      (large) or the single row-quad m = 4*MTF + (t - MTF) (small).
    {
#pragma unroll
      for (int f0 = 0; f0 < NB - 1; ++f0) request(f0, nx[f0], nxo[f0 % NBO]);
      SG_PRIO(SG_PRIO_LIFT);
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        R(&flf)[KSF][3] = nx[f % NB];
        if constexpr (STASH) {
          // the facet's four node offsets of this lane group: one ds_read_b128 (item-invariant, but sixteen registers if kept)
          const nbr4 fo = *reinterpret_cast<const nbr4*>(&sFo[f * 16 + (lo >> 4) * 4]);
#pragma unroll
          for (int ks = 0; ks < KSF; ++ks)
#pragma unroll
            for (int i = 0; i < 3; ++i)
              flf[ks][i] += *reinterpret_cast<const R*>(str + fo[ks] + i * G_STASH_SLOTS * 16 * (int)sizeof(R));
        } else if constexpr (FACT) {
#pragma unroll
          for (int ks = 0; ks < KSF; ++ks)
#pragma unroll
            for (int i = 0; i < 3; ++i) flf[ks][i] += nxo[f % NBO][ks][i];
        }
#pragma unroll
        for (int t = 0; t < MTT; ++t) {
          // next facet's traces: asked for a whole facet ahead
          if (t == 0 && f + NB - 1 < 4) request(f + NB - 1, nx[(f + NB - 1) % NB], nxo[(f + NB - 1) % NBO]);
          // W_ik += (c n)_f,k (L_f u^_i): half of the normal components of a Kuhn class are zero
          auto fold = [&](int m0, int nm, const R (&v)[3][4]) {
#pragma unroll
            for (int kk = 0; kk < 3; ++kk) {
              const R c = cnf[f][kk];
              if (uniform_nonzero(c)) {
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                  for (int j = 0; j < 4; ++j)
                    if (j < nm && m0 + j < S4) {
                      if (i == kk)
                        Sd[i][m0 + j] += c * v[i][j];
                      else
                        So[i + kk - 1][m0 + j] += c * v[i][j];
                    }
              }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (j < nm && m0 + j < S4) {
#pragma unroll
                for (int i = 0; i < 3; ++i) asm volatile("" : "+v"(Sd[i][m0 + j]), "+v"(So[i][m0 + j]));
              }
          };
          if (t < MTF) {
            d4 tmp[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) tmp[i] = d4{0, 0, 0, 0};
#pragma unroll
            for (int ks = 0; ks < KSF; ++ks) {
              const R a = tile(sAL, (f * MTT + t) * KSF + ks, CL::at(f, t, ks), t, MTF);
#pragma unroll
              for (int i = 0; i < 3; ++i) tmp[i] = MFMA64(a, flf[ks][i], tmp[i]);
            }
            {
              R v[3][4];
#pragma unroll
              for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) v[i][reg] = tmp[i][reg];
              fold(4 * t, 4, v);
            }
          } else {
            R tmp[3] = {R(0), R(0), R(0)};
#pragma unroll
            for (int ks = 0; ks < KSF; ++ks) {
              const R a = tile(sAL, (f * MTT + t) * KSF + ks, CL::at(f, t, ks), t, MTF);
#pragma unroll
              for (int i = 0; i < 3; ++i) tmp[i] = MFMA4(a, flf[ks][i], tmp[i]);
            }
            {
              const R v[3][4] = {{tmp[0], 0, 0, 0}, {tmp[1], 0, 0, 0}, {tmp[2], 0, 0, 0}};
              fold(4 * MTF + (t - MTF), 1, v);
            }
          }
        }
      }
    }

    SG_PRIO(SG_PRIO_EPI);
    STAMP(st3);
    // ---- stress and epilogue (MODE 1: s = c_self*s + c_new*rhs in place - the rhs being G(dt u1 + dt^3/24 utemp),
    //      which is dt sh1 + dt^3/24 sh2 of elastic.py:348-352 in one application of the linear g, stages.cpp)
    //      vmcnt counts loads and stores together and the two kinds complete out of order with
    //      each other, so any wait for a load (or a scratch reload) with stores in flight becomes a
    //      wait for every store's acknowledgement.  Hence: finish ALL loads first, building the
    //      results in place in Sd/So, and issue the item's stores back to back at the very end.
    {
      const long e = (L.valid ? L.c : 0) * 6 + k;
      const R lam = (R)(A.per_cell ? A.lam[e] : A.lam0);
      const R mu = (R)(A.per_cell ? A.mu[e] : A.mu0);
      const long obase = ((g * 6 + k) * (long)ND) * 9 * 16 + w;
      // row-quad m of this lane = node 4 m + q: per-item base + compile-time offsets (see brow)
      int qo9 = q * 9 * 16;
      asm volatile("" : "+v"(qo9));
      const long ob_q = obase + qo9;
      const long ob_l = (4 * (S4 - 1) + q < ND) ? ob_q + (long)(S4 - 1) * 4 * 9 * 16 : obase;
      auto orow = [&](int m) { return (m == S4 - 1) ? ob_l : ob_q + (long)m * 4 * 9 * 16; };
      if constexpr (SYM || MODE == 0) {
        constexpr int NL = SYM ? 6 : 9;  // SYM: the lines (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)
        constexpr int PDE = 4;           // row-quads of old values in flight (MODE 1)
        R po[PDE][6];
        auto line = [](int c) { return SYM ? (c < 3 ? c : (c < 5 ? c + 1 : 8)) : c; };
        auto fetch_old = [&](int m) {
          const long o1 = orow(m);
#pragma unroll
          for (int c = 0; c < 6; ++c) po[m % PDE][c] = LD_STREAM(&out[o1 + line(c) * 16]);
        };
        if (MODE == 1) {
#pragma unroll
          for (int m = 0; m < PDE && m < S4; ++m) fetch_old(m);
        }
#pragma unroll
        for (int m = 0; m < S4; ++m) {
          const R tr = lam * (Sd[0][m] + Sd[1][m] + Sd[2][m]);
#pragma unroll
          for (int i = 0; i < 3; ++i) {
            Sd[i][m] = R(2) * mu * Sd[i][m] + tr;
            So[i][m] = mu * So[i][m];
          }
          if (MODE == 1) {
            // line order of the six slots: Sd0 So0 So1 Sd1 So2 Sd2
            Sd[0][m] = c_self * po[m % PDE][0] + c_new * Sd[0][m];
            So[0][m] = c_self * po[m % PDE][1] + c_new * So[0][m];
            So[1][m] = c_self * po[m % PDE][2] + c_new * So[1][m];
            Sd[1][m] = c_self * po[m % PDE][3] + c_new * Sd[1][m];
            So[2][m] = c_self * po[m % PDE][4] + c_new * So[2][m];
            Sd[2][m] = c_self * po[m % PDE][5] + c_new * Sd[2][m];
            if (m + PDE < S4) fetch_old(m + PDE);
          }
#pragma unroll
          for (int i = 0; i < 3; ++i) asm volatile("" : "+v"(Sd[i][m]), "+v"(So[i][m]));
        }
#pragma unroll
        for (int m = 0; m < S4; ++m) {
          const int a = 4 * m + q;
          const long o = orow(m);
          if (L.active && a < ND) {
            ST_STREAM(&out[o + 0 * 16], Sd[0][m]);
            ST_STREAM(&out[o + 1 * 16], So[0][m]);
            ST_STREAM(&out[o + 2 * 16], So[1][m]);
            ST_STREAM(&out[o + 4 * 16], Sd[1][m]);
            ST_STREAM(&out[o + 5 * 16], So[2][m]);
            ST_STREAM(&out[o + 8 * 16], Sd[2][m]);
            if (!SYM) {
              ST_STREAM(&out[o + 3 * 16], So[0][m]);
              ST_STREAM(&out[o + 6 * 16], So[1][m]);
              ST_STREAM(&out[o + 7 * 16], So[2][m]);
            }
          }
        }
        (void)NL;
      } else {
        // full-tensor in-place combine (asymmetric user data, rare): nine results per node
#pragma unroll
        for (int m = 0; m < S4; ++m) {
          const int a = 4 * m + q;
          const long o = orow(m);
          const R tr = lam * (Sd[0][m] + Sd[1][m] + Sd[2][m]);
          R s[9];
          s[0] = R(2) * mu * Sd[0][m] + tr;
          s[4] = R(2) * mu * Sd[1][m] + tr;
          s[8] = R(2) * mu * Sd[2][m] + tr;
          s[1] = s[3] = mu * So[0][m];
          s[2] = s[6] = mu * So[1][m];
          s[5] = s[7] = mu * So[2][m];
#pragma unroll
          for (int ij = 0; ij < 9; ++ij) s[ij] = c_self * out[o + ij * 16] + c_new * s[ij];
          if (L.active && a < ND) {
#pragma unroll
            for (int ij = 0; ij < 9; ++ij) out[o + ij * 16] = s[ij];
          }
        }
      }
    }
    STAMP(st4);
    STAMP_ACC;
  }
  STAMP_FLUSH;
}

// A g_stash instantiation holds BOTH forms and the launch picks one by its block: 512 threads and GLds<.., 1>::BYTES of dynamic
// LDS run the stash form, 256 threads and GLds<.., 0>::BYTES the form before it (launch_stage_mfma, StageArgs::gstash) - one
// kernel object and one name per (MODE, SYM), two bodies that share nothing but the arguments.  The branch is on a scalar.
template <typename R, int P, int MODE, int SYM, int FACT>
__global__ __launch_bounds__((g_stash<R, P, FACT>() ? 512 : 256), (g_stash<R, P, FACT>() ? 1 : mfma_resident_blocks<R, P>())) void mfma_stage_G(StageArgs A) {
  if constexpr (g_stash<R, P, FACT>()) {
    if (blockDim.x == 512)
      stage_G_body<R, P, MODE, SYM, true, true, true>(A);
    else
      stage_G_body<R, P, MODE, SYM, true, false, true>(A);
  } else {
    stage_G_body<R, P, MODE, SYM, FACT != 0, false, false>(A);
  }
}

// --------------------------------------------------------------------------------------------
//  F: uh_i = -sum_r D_r (Jinv_rj T_ij) + sum_f L_f [ (c n)_j {T_ij} ] - sponge
// --------------------------------------------------------------------------------------------
template <typename R, int P, int MODE, int SYM, int GHOST>
__global__ __launch_bounds__(256, (mfma_resident_blocks<R, P>())) void mfma_stage_F(StageArgs A) {
  using M = MG<P, R>;
  typedef typename RT<R>::v4 d4;
  constexpr int PRIO3 = MODE == 1 ? SG_PRIO_F1 : (MODE == 2 ? SG_PRIO_F2 : SG_PRIO_F0);
  constexpr int ND = M::ND, NF = M::NF, KS = M::KS, KSF = M::KSF, MTF = M::MTF, NSM = M::NSM, MTT = M::MTT;
  __shared__ R sAV[M::NFRAG_F * 64];
  __shared__ R sAL[M::NFRAG_L * 64];
  // where a lane finds the nodes of a neighbour's trace: offsets of the four facet k-steps per (variant: interior /
  // remote record / domain boundary, class, facet, lane group), tabulated on the host (mfma_tables.cpp
  // mfma_trace_offsets) - one ds_read_b128 per facet instead of three batches of scalar loads, a byte extraction and a
  // multiplication per k-step, and a dozen SGPRs fewer (the neighbour set-up took 4.6 k of an item's 53 k cycles)
  __shared__ nbr4 sFt[3 * 6 * 4 * 4];
  {
    const nbr4* src = reinterpret_cast<const nbr4*>(A.ftab);
    for (int i = threadIdx.x; i < 3 * 6 * 4 * 4; i += 256) sFt[i] = src[i];
  }
  load_tables<M::NFRAG_F, M::NFRAG_L>(sAV, sAL, A);
  const cMfmaConst& mk = *(const cMfmaConst*)(unsigned long long)A.mk;

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int q = lane >> 4, w = lane & 15;
  const R* __restrict__ in = reinterpret_cast<const R*>(A.in);
  const R* __restrict__ aux = reinterpret_cast<const R*>(A.aux);
  R* __restrict__ out = reinterpret_cast<R*>(A.out);
  const R c_self = (R)A.c_self, c_aux = (R)A.c_aux, c_new = (R)A.c_new;
  const long ngroups = mk.ncube_pad >> 4;
  const ItemRange ir = item_range(A.item_list ? (long)A.nlist : ngroups * 6, wave, A.spread, A.order_chunk);

  STAMP_DECL;
  for (long it = ir.lo; it < ir.hi; it += ir.step) {
    STAMP(st0);
    const long iti = item_of(ir, it);
    if (iti < 0) continue;
    const long item = A.item_list ? (long)A.item_list[iti] : iti;
    const long g = item / 6;
    const int k = (int)(item - g * 6);
    const LaneGeo L = A.all_active ? lane_geo_all(mk.ncube, g, w) : lane_geo(mk, A, g, w);
    const cMfmaClassConst& kc = mk.cls[k];
    const nbr4 nbe = load_nbr4(A, item, w);
    if (!__any(L.active)) continue;
    const R* own = in + ((g * 6 + k) * (long)ND) * 9 * 16 + w;
    // B rows: a wave-uniform base (the item's first line; the class's line offset is added to it, in scalars) and the
    // lane's offset from it - node 4 ks + q, cell w.  Opaque per item, as in mfma_stage_G.
    const R* ownu = in + ((g * 6 + k) * (long)ND) * 9 * 16;
    int qo = q * 9 * 16 + w;
    asm volatile("" : "+v"(qo));
    const int qol = (4 * (KS - 1) + q < ND) ? qo + (KS - 1) * 4 * 9 * 16 : w;
    auto brow = [&](int ks) { return (unsigned)((ks == KS - 1) ? qol : qo + ks * 4 * 9 * 16); };
    int lo = lane;
    asm volatile("" : "+v"(lo));

    // The item works in its class's own axis order (kernels.hpp mfma_class_frame): accumulator i' is velocity component
    // p[i'], tensor slot (a, b) is T(p[a], p[b]).  J^-1 and the facets' non-zero columns are then the same for every class;
    // the class enters through the scale factors sm, the values of (c n) and the wave-uniform line offsets below.
    R sm[3];
    int vl[3], ol[9];
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      sm[m] = (R)kc.cf_s[m];
      vl[m] = kc.cf_vel[m];
    }
#pragma unroll
    for (int c = 0; c < 9; ++c) ol[c] = kc.cf_own[SYM ? 1 : 0][c];

    // rows 16t + 4reg + q in acc[i][t][reg] (large tiles), row 16*MTF + 4s + q in accs[i][s] (small)
    d4 acc[3][M::MTFA];
    R accs[3][M::NSMA];
    const long e = (L.valid ? L.c : 0) * 6 + k;
    // output rows: like the B rows a wave-uniform base per component line (component p[i'] at vl[i']) and the lane's offset
    const long ubu = ((g * 6 + k) * (long)ND) * 3 * 16;
    int qo3 = q * 3 * 16 + w;
    asm volatile("" : "+v"(qo3));
    const long ub_q = ubu + qo3;
    // (opaque scalars: left to itself the optimiser re-associates base + lane + line and adds the line per lane and access;
    //  formed where a group of accesses starts, not per item: six scalar pairs held through the item spill in the float kernels)
    typedef __attribute__((address_space(1))) R gR;
    auto line_of = [&](const R* field, int i) {
      const gR* l = (const gR*)(field + (ubu + vl[i]));
      asm volatile("" : "+s"(l));
      return l;
    };
    // Fused combine u = c_self u + c_aux uh1 + c_new rhs (MODE 1), EARLY form: the old values are requested at the
    // START of the item, together with the first own rows, and enter the accumulators as (c_self u + c_aux uh1) / c_new;
    // the matrix products add rhs on top and the epilogue only scales by c_new and stores - no loads, no second
    // memory latency at the end of the item (the epilogue of F<4,1> took 10 k of an item's 67 k cycles against 2.8 k in
    // F<4,0>).  Rounding: the sum is formed at the scale of u / c_new, i.e. with the absolute error the final u carries
    // anyway.  c_new = 0 (dt = 0) keeps the late form.
    // (double only: in float u / c_new could leave the exponent range for small dt)
    // MODE 2: the same without the self term, out = c_aux aux + c_new rhs (stage UTEMP leaves w = dt u1 + dt^3/24 utemp,
    // stages.cpp): no old value of `out` is read.
    constexpr bool FUSED = MODE >= 1, SELF = MODE == 1;
    const bool early = FUSED && sizeof(R) == 8 && uniform_nonzero(c_new);
    R cs = c_self, ca = c_aux, cn = c_new;
    if (MODE == 1 && A.rho2 != nullptr) {  // per-cell density (kernels.hpp)
      cs = (R)A.rho2[2 * e];
      ca *= (R)A.rho2[2 * e + 1];
      cn *= (R)A.rho2[2 * e + 1];
    }
    // Sponge of this lane's cell (the block further down): a sigma that is constant over the cell enters as -sigma u_abs at
    // the node.  In the fused stages u_abs IS one of the combine's operands - `out` in stage U1, `aux` in stage UTEMP - so
    // the term is a change of that operand's coefficient, no load and no arithmetic of its own.
    // (the plain stage asks for its sigma where it uses it, further down: asked here it changes the register allocation of
    // the whole item and costs the stage 3 % - without any sponge set)
    R sig = (R)0;
    bool sig_folded = false;
    if (FUSED && A.sponge_sigma != nullptr && L.active) {
      sig = (R)A.sponge_sigma[e];
      if (sig == sig && sig != (R)0) {
        if (SELF && A.uabs == A.out) {
          cs -= cn * sig;
          sig_folded = true;
        } else if (A.uabs == A.aux) {
          ca -= cn * sig;
          sig_folded = true;
        }
      }
    }
    // old values of the in-place combine: every one of the item requested before the first is used
    R po[M::MTFA][4][3], pa[M::MTFA][4][3], pos[M::NSMA][3], pas[M::NSMA][3];
    auto fetch_old = [&]() {
      const gR *outl[3], *auxl[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        outl[i] = SELF ? line_of(out, i) : nullptr;
        auxl[i] = line_of(aux, i);
      }
#pragma unroll
      for (int t = 0; t < MTF; ++t)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          // the last float tile is zero-padded: its rows beyond ND read a valid address and are not stored
          const bool row_ok = RT<R>::SMALL || (16 * t + 4 * reg + q < ND);
          const unsigned o = (unsigned)(row_ok ? qo3 + (16 * t + 4 * reg) * 3 * 16 : w);
#pragma unroll
          for (int i = 0; i < 3; ++i) {
            po[t][reg][i] = SELF ? LD_STREAM(lane_at_g(outl[i], o)) : R(0);
            pa[t][reg][i] = LD_STREAM(lane_at_g(auxl[i], o));
          }
        }
#pragma unroll
      for (int t = 0; t < NSM; ++t) {
        const int a = 16 * MTF + 4 * t + q;
        const unsigned o = (unsigned)((a < ND) ? qo3 + (16 * MTF + 4 * t) * 3 * 16 : w);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          pos[t][i] = SELF ? LD_STREAM(lane_at_g(outl[i], o)) : R(0);
          pas[t][i] = LD_STREAM(lane_at_g(auxl[i], o));
        }
      }
    };
    if (early) {
      fetch_old();
      const R icn = R(1) / cn;
#pragma unroll
      for (int t = 0; t < MTF; ++t)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg)
#pragma unroll
          for (int i = 0; i < 3; ++i) acc[i][t][reg] = SELF ? (cs * po[t][reg][i] + ca * pa[t][reg][i]) * icn : (ca * pa[t][reg][i]) * icn;
#pragma unroll
      for (int t = 0; t < NSM; ++t)
#pragma unroll
        for (int i = 0; i < 3; ++i) accs[i][t] = SELF ? (cs * pos[t][i] + ca * pas[t][i]) * icn : (ca * pas[t][i]) * icn;
    } else {
#pragma unroll
      for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int t = 0; t < MTF; ++t) acc[i][t] = d4{0, 0, 0, 0};
#pragma unroll
        for (int t = 0; t < NSM; ++t) accs[i][t] = R(0);
      }
    }

    SG_PRIO(SG_PRIO_VOL);
    STAMP(st1);
    auto do_volume = [&]() {
      // ---- volume: K runs over (m, node); B = s_m T_i,p[m], one own line times one scalar (the tiles are the E'_m of
      //      mfma_tables.cpp mfma_frags_F)
      {
        constexpr int PFV = sizeof(R) == 4 ? 2 : 1;  // k-steps of own tensors in flight ahead of the MFMAs
        R Tq[PFV][9];
#pragma unroll
        for (int s0 = 0; s0 < PFV && s0 < KS; ++s0) load_tensor<SYM>(ownu, brow(s0), ol, Tq[s0]);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          R T[9];
#pragma unroll
          for (int c = 0; c < 9; ++c) T[c] = Tq[ks % PFV][c];
          if (ks + PFV < KS) {
            load_tensor<SYM>(ownu, brow(ks + PFV), ol, Tq[ks % PFV]);
          }
#pragma unroll
          for (int r = 0; r < 3; ++r) {
            R Tt[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) Tt[i] = sm[r] * T[i * 3 + r];
#pragma unroll
            for (int t = 0; t < MTT; ++t) {
              const R a = sAV[(t * 3 * KS + KS * r + ks) * 64 + lo];
#pragma unroll
              for (int i = 0; i < 3; ++i) {
                if (t < MTF)
                  acc[i][t < MTF ? t : 0] = MFMA64(a, Tt[i], acc[i][t < MTF ? t : 0]);
                else
                  accs[i][t < MTF ? 0 : t - MTF] = MFMA4(a, Tt[i], accs[i][t < MTF ? 0 : t - MTF]);
              }
            }
          }
        }
      }

    };
    auto do_lifts = [&]() {
      // ---- facet lifts of (c n)_j {T_ij}; no ds term in f => zero flux on the boundary
      //      (elastic.py:206).  The own half of {T} is part of the volume tiles (E_r), so the lift
      //      carries +1/2 (c n).T- on interior facets and -1/2 (c n).T+ on boundary facets (which
      //      cancels the folded half): wf * (c n).T of whatever np[f] points at, the 1/2 being part
      //      of the lift tiles.
      // facet k-steps of neighbour traces in flight (three in double, in the registers the unseen lines freed, leave the
      // step where it is: profiles/r10/f_trace_lines_variants.txt)
      constexpr int PFL = sizeof(R) == 4 ? 3 : 2;
      auto cube_face = [](int f) { return f == 0 || f == 3; };
      // cube faces (slot f / 3): the lane's neighbour and whether it is a remote record; inner facets (slot f - 1): the line
      // bases of the neighbour item of this cell group
      const R* np[2];
      bool gh[2];
      const gR* npl[2][6];
      R wc[4][2];   // wf (c n) at the facet's columns; wf = -1 on the domain boundary (cube faces only)
      int noff[4][KSF];   // the lane's offset of the facet node at k-step ks (inner facets: its cell w included)
      // the lines each facet's normal can see and the entries of a remote record, in the frame: wave-uniform
      int tl[4][6], gp[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) gp[i] = kc.cf_p[i];
#pragma unroll
      for (int f = 0; f < 4; ++f) {
#pragma unroll
        for (int c = 0; c < 6; ++c) tl[f][c] = kc.cf_tr[SYM ? 1 : 0][f][c];
        int var = 0;
        if (cube_face(f)) {
          const NbrRef<R> NR = nbr_from_entry<ND, NF, 9>(A, nbe[f], 2 * kc.nb_axis[f] + (kc.nb_dir[f] > 0 ? 1 : 0), own);
          np[f / 3] = NR.p;
          gh[f / 3] = GHOST && NR.ghost;
          const R wf = NR.physical ? R(-1) : R(1);
          wc[f][0] = wf * (R)kc.cf_cn[f][0];
          wc[f][1] = R(0);
          var = NR.ghost ? 1 : (NR.physical ? 2 : 0);
        } else {
          // (layout-padding lanes, whose table entries say "domain boundary", read the neighbour item's padding like every
          // other lane: allocated, and nothing of theirs is stored)
          wc[f][0] = (R)kc.cf_cn[f][0];
          wc[f][1] = (R)kc.cf_cn[f][1];
        }
        const nbr4 o4 = sFt[((var * 6 + k) * 4 + f) * 4 + q];
#pragma unroll
        for (int ks = 0; ks < KSF; ++ks) noff[f][ks] = cube_face(f) ? o4[ks] : o4[ks] + w;
      }
      R nq[PFL][6];
      // k-step ks of facet f into T.  The line bases of an inner facet are formed as opaque scalars (see line_of) when its
      // first k-step is requested - all of them held from the set-up on are ten scalar pairs more than the float kernels have
      auto request = [&](int f, int ks, R (&T)[6]) {
        if (cube_face(f)) {
          load_trace_face<GHOST>(np[f / 3] + noff[f][ks], gh[f / 3], tl[f], gp, T);
          return;
        }
        if (ks == 0) {
          const R* const nbu = in + ((g * 6 + kc.nb_cls[f]) * (long)ND) * 9 * 16;
#pragma unroll
          for (int c = 0; c < (SYM ? 5 : 6); ++c) {
            npl[f - 1][c] = (const gR*)(nbu + tl[f][c]);
            asm volatile("" : "+s"(npl[f - 1][c]));
          }
        }
        load_trace_inner<SYM>(npl[f - 1], (unsigned)noff[f][ks], T);
      };
      STAMP(sta);   // diagnostic builds: end of the neighbour set-up
      {
        constexpr int NS = 4 * KSF;
#pragma unroll
        for (int s = 0; s < PFL; ++s) request(s / KSF, s % KSF, nq[s]);
#pragma unroll
        for (int f = 0; f < 4; ++f) {
          if (f == 1) STAMP(stb);   // diagnostic builds: end of facet 0
#pragma unroll
          for (int ks = 0; ks < KSF; ++ks) {
            const int s = f * KSF + ks;
            R fl[3];
#pragma unroll
            for (int i = 0; i < 3; ++i)
              fl[i] = trace_flux<SYM>(f, i, wc[f], nq[s % PFL]);
            if (s + PFL < NS) {
              request((s + PFL) / KSF, (s + PFL) % KSF, nq[s % PFL]);
            }
#pragma unroll
            for (int t = 0; t < MTT; ++t) {
              const R a = sAL[((f * MTT + t) * KSF + ks) * 64 + lo];
#pragma unroll
              for (int i = 0; i < 3; ++i) {
                if (t < MTF)
                  acc[i][t < MTF ? t : 0] = MFMA64(a, fl[i], acc[i][t < MTF ? t : 0]);
                else
                  accs[i][t < MTF ? 0 : t - MTF] = MFMA4(a, fl[i], accs[i][t < MTF ? 0 : t - MTF]);
              }
            }
          }
        }
      }

    };
    do_volume();
    STAMP(st2);
    SG_PRIO(SG_PRIO_LIFT);
    do_lifts();

    SG_PRIO(SG_PRIO_EPI);
    STAMP(st3);
    // ---- sponge: -M^-1 int sigma phi_a phi_b u_abs[b][i] (elastic.py:207-208) on the lanes whose cell carries sigma.
    // A sigma that is one value on all nodes of the cell - the piecewise-constant sponges of the reference's problem
    // scripts - makes that -sigma u_abs at the node itself (StageArgs::sponge_sigma holds the value).  A varying one has a
    // matrix B_e (sponge_sigma = NaN, sponge_slot): B_e u_abs of those cells is computed by a launch of its own before the
    // stage (StageArgs::sponge_pre, kernels.hip sponge_pre_kernel) - a matrix loop here would hold the whole wave for the
    // sake of one lane, and an item that straddles the edge of a sponge strip has such a lane.  Either way a lane reads
    // one value per row and component: same loads, different base, stride and factor.  With the in-place combine u_abs
    // may be `out`: every lane of a cell sits in this wave and the wave runs in program order, so the reads below precede
    // the writes of the epilogue (and the pre-pass ran before the stage).
    if (A.sponge_sigma != nullptr) {
      if (!FUSED && L.active) sig = (R)A.sponge_sigma[e];
      int slot = -1;
      if (sig != sig) slot = A.sponge_slot[e];
      const bool sp_here = sig != (R)0 && !sig_folded;      // (NaN != 0: the lanes with a matrix count)
      if (__any(sp_here)) {
        if (sp_here) {
          constexpr int NR = 4 * MTF + NSM;     // row-quads of this lane: node 4 r + q
          const bool dense = slot >= 0;
          // (the pre-pass results are lines like the fields': slot = their item * 16 + the cell's column)
          const R* pb = dense ? reinterpret_cast<const R*>(A.sponge_pre) + ((long)(slot >> 4) * ND * 3 + q * 3) * 16 + (slot & 15)
                              : reinterpret_cast<const R*>(A.uabs) + ub_q;
          constexpr int es = 16;
          const R sc = dense ? (R)1 : sig;
          R uo[NR][3];
#pragma unroll
          for (int r = 0; r < NR; ++r) {
            const int o = (4 * r + q < ND) ? 4 * r * 3 * es : 0;
#pragma unroll
            for (int i = 0; i < 3; ++i) uo[r][i] = pb[o + vl[i]];      // (es = 16: component p[i'] of the node)
          }
#pragma unroll
          for (int r = 0; r < NR; ++r)
#pragma unroll
            for (int i = 0; i < 3; ++i)
              if (4 * r + q < ND) {
                const R v = sc * uo[r][i];
                if (r < 4 * MTF)
                  acc[i][r >> 2][r & 3] -= v;
                else
                  accs[i][r - 4 * MTF] -= v;
              }
        }
      }
    }

    // ---- epilogue (MODE 1: u = c_self*u + c_aux*uh1 + c_new*rhs in place, elastic.py:341-345).
    //      All loads first (results built in place in the accumulators), all stores last: see G.
    if (FUSED && early) {
#pragma unroll
      for (int t = 0; t < MTF; ++t)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg)
#pragma unroll
          for (int i = 0; i < 3; ++i) acc[i][t][reg] = cn * acc[i][t][reg];
#pragma unroll
      for (int t = 0; t < NSM; ++t)
#pragma unroll
        for (int i = 0; i < 3; ++i) accs[i][t] = cn * accs[i][t];
    } else if (FUSED) {
      // one memory latency per item instead of one per row tile (the lifts' registers are free by now)
      fetch_old();
#pragma unroll
      for (int t = 0; t < MTF; ++t)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg)
#pragma unroll
          for (int i = 0; i < 3; ++i) {
            R v = SELF ? cs * po[t][reg][i] + ca * pa[t][reg][i] + cn * acc[i][t][reg] : ca * pa[t][reg][i] + cn * acc[i][t][reg];
            asm volatile("" : "+v"(v));
            acc[i][t][reg] = v;
          }
#pragma unroll
      for (int t = 0; t < NSM; ++t)
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          accs[i][t] = SELF ? cs * pos[t][i] + ca * pas[t][i] + cn * accs[i][t] : ca * pas[t][i] + cn * accs[i][t];
          asm volatile("" : "+v"(accs[i][t]));
        }
    }
    if (L.active) {
      gR* outl[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) outl[i] = (gR*)line_of(out, i);
#pragma unroll
      for (int t = 0; t < MTF; ++t)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const unsigned o = (unsigned)(qo3 + (16 * t + 4 * reg) * 3 * 16);
          if (RT<R>::SMALL || (16 * t + 4 * reg + q < ND)) {
#pragma unroll
            for (int i = 0; i < 3; ++i) ST_STREAM(lane_at_g(outl[i], o), acc[i][t][reg]);
          }
        }
#pragma unroll
      for (int t = 0; t < NSM; ++t) {
        const int a = 16 * MTF + 4 * t + q;
        if (a < ND) {
          const unsigned o = (unsigned)(qo3 + (16 * MTF + 4 * t) * 3 * 16);
#pragma unroll
          for (int i = 0; i < 3; ++i) ST_STREAM(lane_at_g(outl[i], o), accs[i][t]);
        }
      }
    }
    STAMP(st4);
    STAMP_ACC;
  }
  STAMP_FLUSH;
}

// --------------------------------------------------------------------------------------------
//  Sponge of the cells whose sigma is affine in the reference coordinates (kernels.hpp launch_sponge_pre_affine has the
//  family-independent form): sp[slot][a][i] = s_0 u_i[a] + sum_k s_k (X_k u_i)[a] with the element-constant X_k as row
//  tiles in LDS and the cells' own values as B operands straight from their lines - the first product of a G stage with
//  other matrices; the per-cell coefficients s_k scale the accumulator COLUMNS (a lane's cell) as the results come out,
//  and s_0 u needs no load: accumulator row 4 m + q of a lane is the node of its B operand at k-step m.
// --------------------------------------------------------------------------------------------
template <int P>
__global__ __launch_bounds__(512) void sponge_affine_mfma(const double* __restrict__ uabs, const double* __restrict__ fragX,
                                                          const int32_t* __restrict__ items, const int32_t* __restrict__ item_slots,
                                                          const double* __restrict__ coef, double* __restrict__ sp, int nitems) {
  using M = MG<P, double>;
  typedef RT<double>::v4 d4;
  constexpr int ND = M::ND, KS = M::KS, MTF = M::MTF, NSM = M::NSM, MTT = M::MTT, S4 = M::S4;
  static_assert(KS == S4, "k-step m and row-quad m name the same nodes");
  __shared__ double sX[3 * MTT * KS * 64];
  copy_to_lds<3 * MTT * KS * 64, double, 512>(sX, fragX);
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int q = lane >> 4, w = lane & 15;
  // A unit of work is ONE velocity component of one item: 9 B rows, 9 + 9 accumulator values - 108 registers at degree 4, so
  // four waves per SIMD hide the unit's two dependent load latencies (slots -> coefficients, rows) behind each other's matrix
  // work.  (A wave per whole item - 27 rows, 81 accumulators, two waves per SIMD - took 0.50 ms per launch for 48 000 items
  // whose matrix work is 0.07 ms; the same wave with the next item's operands requested ahead spilled and took 0.9 ms.)
  const long nunits = (long)nitems * 3;
  for (long un = (long)blockIdx.x * 8 + wave; un < nunits; un += (long)gridDim.x * 8) {
    const long n = un / 3;
    const int i = (int)(un - n * 3);
    const int sl = item_slots[n * 16 + w];
    double sc[4] = {0.0, 0.0, 0.0, 0.0};
    if (sl >= 0) {
#pragma unroll
      for (int k = 0; k < 4; ++k) sc[k] = coef[(long)sl * 4 + k];
    }
    const double* own = uabs + ((long)items[n] * ND * 3 + i) * 16 + w;
    double ub[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) ub[ks] = own[((4 * ks + q < ND) ? 4 * ks + q : 0) * 3 * 16];      // padded rows meet zero operator columns
    int lo = lane;      // opaque: keeps the item-invariant tile reads inside the loop (they would not fit the registers)
    asm volatile("" : "+v"(lo));
    double r[S4];
#pragma unroll
    for (int m = 0; m < S4; ++m) r[m] = sc[0] * ub[m];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      d4 acc[M::MTFA];
      double accs[M::NSMA];
#pragma unroll
      for (int t = 0; t < MTF; ++t) acc[t] = d4{0, 0, 0, 0};
#pragma unroll
      for (int t = 0; t < NSM; ++t) accs[t] = 0.0;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int t = 0; t < MTT; ++t) {
          const double a = sX[((k * MTT + t) * KS + ks) * 64 + lo];
          if (t < MTF)
            acc[t < MTF ? t : 0] = RT<double>::big(a, ub[ks], acc[t < MTF ? t : 0]);
          else
            accs[t < MTF ? 0 : t - MTF] = RT<double>::small(a, ub[ks], accs[t < MTF ? 0 : t - MTF]);
        }
      const double sk = sc[1 + k];
#pragma unroll
      for (int t = 0; t < MTF; ++t)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) r[4 * t + reg] += sk * acc[t][reg];
#pragma unroll
      for (int t = 0; t < NSM; ++t) r[4 * MTF + t] += sk * accs[t];
    }
    // line layout (slot = item' * 16 + w): whole 128-byte lines; the columns of cells without an affine sigma belong to
    // nobody or to the matrix pre-pass (another kernel, same stream): masked
    if (sl >= 0) {
      double* rec = sp + ((long)(sl >> 4) * ND * 3 + i) * 16 + w;
#pragma unroll
      for (int m = 0; m < S4; ++m) {
        const int a = 4 * m + q;
        if (a < ND) rec[a * 3 * 16] = r[m];
      }
    }
  }
}

// blocks of eight waves a device of ncu CUs holds of the degree's instantiation (registers and the tiles' LDS decide - two per
// CU at degree 4).  sg_set_absorption asks at set-up, i.e. outside any stream capture.
int prepare_sponge_affine_mfma(int P, int ncu) {
  if (P < 1 || P > 4) return -1;
  int per_cu = 0;
  const void* k = P == 1 ? (const void*)sponge_affine_mfma<1> : P == 2 ? (const void*)sponge_affine_mfma<2>
                : P == 3 ? (const void*)sponge_affine_mfma<3> : (const void*)sponge_affine_mfma<4>;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k, 512, 0) != hipSuccess || per_cu <= 0) per_cu = 2;
  return per_cu * ncu;
}

int launch_sponge_affine_mfma(int P, const void* uabs, const double* fragX, const int32_t* items, const int32_t* item_slots,
                              const double* coef, void* sp, int32_t nitems, int grid, void* stream) {
  if (nitems <= 0) return 0;
  // a persistent grid of exactly the resident blocks (`grid`): more would run a second, partly empty round
  long blocks = ((long)nitems * 3 + 7) / 8;
  if (blocks > grid) blocks = grid;
  const dim3 dgrid((unsigned)blocks), block(512);
  hipStream_t s = (hipStream_t)stream;
  switch (P) {
    case 1: hipLaunchKernelGGL(sponge_affine_mfma<1>, dgrid, block, 0, s, (const double*)uabs, fragX, items, item_slots, coef, (double*)sp, nitems); break;
    case 2: hipLaunchKernelGGL(sponge_affine_mfma<2>, dgrid, block, 0, s, (const double*)uabs, fragX, items, item_slots, coef, (double*)sp, nitems); break;
    case 3: hipLaunchKernelGGL(sponge_affine_mfma<3>, dgrid, block, 0, s, (const double*)uabs, fragX, items, item_slots, coef, (double*)sp, nitems); break;
    case 4: hipLaunchKernelGGL(sponge_affine_mfma<4>, dgrid, block, 0, s, (const double*)uabs, fragX, items, item_slots, coef, (double*)sp, nitems); break;
    default: return -1;
  }
  return (int)hipGetLastError();
}

int mfma_blocks_per_cu(int P, int f32) {
  if (f32) return mfma_resident_blocks<float, 4>();
  return P == 1 ? mfma_resident_blocks<double, 1>() : (P == 2 ? mfma_resident_blocks<double, 2>() : mfma_resident_blocks<double, 4>());
}

// F stages: MODE = a.mode (0 / 1 / 2) and GHOST; G stages: MODE = (a.mode != 0) and FACT, the factorised volume term
// (StageArgs::fragQ; a.fragV then holds the P_r tiles), which exists in double from degree 3 on
const void* stage_kernel_mfma(int kind, int P, const StageArgs& a) {
  return sg_pick<0, 1>(a.f32 != 0, [&](auto f32) {
    using R = std::conditional_t<decltype(f32)::value, float, double>;
    return sg_pick<1, 2, 3, 4>(P, [&](auto p) {
      constexpr int PP = decltype(p)::value, HAS_FACT = sizeof(R) == 8 && PP >= 3;
      return sg_pick<0, 1>(a.sym != 0, [&](auto sym) {
        constexpr int SYM = decltype(sym)::value;
        if (kind == 0)
          return sg_pick<0, 1, 2>(a.mode == 0 || a.mode == 2 ? a.mode : 1, [&](auto mode) {
            return sg_pick<0, 1>(any_ghost(a, 6), [&](auto ghost) {
              return (const void*)&mfma_stage_F<R, PP, decltype(mode)::value, SYM, decltype(ghost)::value>;
            });
          });
        return sg_pick<0, 1>(a.mode != 0, [&](auto mode) {
          return sg_pick<0, HAS_FACT>(HAS_FACT && a.fragQ != nullptr, [&](auto fact) {
            return (const void*)&mfma_stage_G<R, PP, decltype(mode)::value, SYM, decltype(fact)::value>;
          });
        });
      });
    });
  });
}

static_assert(GLds<double, 4, 1>::BYTES == 156640 && GLds<double, 4, 1>::BYTES <= 160 * 1024, "stash form: one block per CU");
static_assert(GLds<double, 4, 0>::BYTES == 61152 && 2 * GLds<double, 4, 0>::BYTES <= 160 * 1024, "form without a stash: two blocks per CU");

// the G kernels of degree 4 that hold two forms (g_stash): these take their LDS from the launch
static bool two_form_kernel(const void* kernel) {
  for (int v = 0; v < 4; ++v) {
    const void* k = sg_pick<0, 1>(v & 1, [&](auto mode) {
      return sg_pick<0, 1>(v >> 1, [&](auto sym) { return (const void*)&mfma_stage_G<double, 4, decltype(mode)::value, decltype(sym)::value, 1>; });
    });
    if (k == kernel) return true;
  }
  return false;
}

// once per handle of the MFMA family, outside any stream capture: allow the stash form its dynamic LDS (more than the 64 KB
// a launch may ask for unprepared); 0 on success
int prepare_stage_mfma() {
  for (int v = 0; v < 4; ++v) {
    const void* k = sg_pick<0, 1>(v & 1, [&](auto mode) {
      return sg_pick<0, 1>(v >> 1, [&](auto sym) { return (const void*)&mfma_stage_G<double, 4, decltype(mode)::value, decltype(sym)::value, 1>; });
    });
    if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, GLds<double, 4, 1>::BYTES) != hipSuccess) return -1;
  }
  return 0;
}

int launch_stage_mfma(const void* kernel, const StageArgs& a, void* stream) {
  // persistent grid, at most 2 blocks of four waves per CU; a multiple of 8 (one item range per XCD label)
  // ... and no more blocks than there are items for their waves (small blocks - the reference's own 3-D sweeps run
  // N <= 8 - are launch-bound: every block copies the operator tiles into LDS before its first item)
  // a.grid_blocks counts slots of FOUR waves whatever the kernel: an eight-wave block of the stash form takes two (the same
  // waves on the same CUs, blockIdx % 8 still the XCD), and there are at least eight blocks, so that every XCD label has one
  const bool two = two_form_kernel(kernel), stash = two && a.gstash;
  const unsigned wpb = stash ? 8u : 4u;
  const unsigned lds = two ? (unsigned)(stash ? GLds<double, 4, 1>::BYTES : GLds<double, 4, 0>::BYTES) : 0u;
  unsigned nblk = (unsigned)(a.grid_blocks > 0 ? a.grid_blocks : 512);
  if (stash) nblk = nblk / 16u * 8u > 8u ? nblk / 16u * 8u : 8u;
  if (a.nitems > 0 && !a.spread) {
    const unsigned need = (((unsigned)a.nitems + wpb - 1u) / wpb + 7u) / 8u * 8u;
    nblk = need < nblk ? need : nblk;
  }
  void* args[] = {const_cast<StageArgs*>(&a)};
  (void)hipLaunchKernel(kernel, dim3(nblk), dim3(wpb * 64u), args, lds, (hipStream_t)stream);
  return (int)hipGetLastError();
}

}  // namespace sg
