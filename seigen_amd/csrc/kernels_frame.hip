// Frames (include/seigen_hip.h sg_get_frame_dev): one field rastered on a pixel lattice commensurate with the block's cubes
// (hostlogic.hpp FramePlan; kernels.hpp FrameSpec).  Every cube holds the same Q in-cube pixels, and pixel q has the same class
// and reference coordinates in every cube: the weights are one table phi[Q][nd], and
//   out[c][pixel] = sum_a phi[q][a] * (double)field[cell(cube, cls[q])][a][c]
// over a ascending with fma from zero in double, rounded once where the caller's type is float - the receivers' sum
// (kernels_recv.hip), the same bits in both kernels here and on every layout.
//
// lanes (gw = 16, 64): a wave takes 64 cubes - 64 / gw listed groups, lane w of a group its cube w - of one class k and one
//   component c (the grid's y) at a time.  Node a of the 64 cells is the words ((item * nd + a) * ncomp + c) * gw + w, item =
//   group * ncls + k: whole contiguous lines, 128 bytes of doubles per group of 16, 512 per group of 64.  The wave walks the
//   pixels of class k eight at a time: eight sums per lane in registers, one load of a nodal line for the eight, four lines in
//   flight.  Unit, class and pixel are wave-uniform (the wave index goes through readfirstlane), so the specification, order[],
//   cstart[] and phi[q][a] are scalar loads; the tables are __restrict__ kernel arguments for that.  Padding lanes
//   (cube >= ncube), lanes beyond the list and cubes outside a slice's layer load and store nothing.  The stores of a wave are
//   m[0] elements apart along x: plain stores (DESIGN.md "Frames").
// flat (gw = 1): a thread per (listed cube, in-cube pixel), pixel fastest; the weights are a per-thread read of the table.
// The grid's x strides over the units beyond its cap.  All index arithmetic is 64-bit.
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace sg {
namespace frame {

static constexpr int CHUNK = 8;   // pixels a wave sums side by side

// the line of output component c that holds its value: the mirror of an (i > j) stress entry in symmetric storage
__device__ __forceinline__ int source_line(int c, int dim, int ncomp, int sym) {
  if (!sym || ncomp != dim * dim) return c;
  const int i = c / dim, j = c - i * dim;
  return i > j ? j * dim + i : c;
}

// offset of in-cube pixel q of cube (c0, c1, c2) in the caller's buffer, component excluded
__device__ __forceinline__ int64_t pixel_offset(const FrameSpec& S, int q, int c0, int c1, int c2, int64_t s2, int64_t s1, int64_t s0) {
  const int j0 = q % S.m[0], j1 = q / S.m[0] % S.m[1], j2 = q / (S.m[0] * S.m[1]);
  const int64_t p0 = S.fixed[0] ? 0 : (int64_t)c0 * S.m[0] + j0;
  const int64_t p1 = S.fixed[1] ? 0 : (int64_t)c1 * S.m[1] + j1;
  const int64_t p2 = S.fixed[2] ? 0 : (int64_t)c2 * S.m[2] + j2;
  return p2 * s2 + p1 * s1 + p0 * s0;
}

// F: the block's word type, C: the caller's; sc, s2, s1, s0: the strides of the component and of axes 2, 1, 0 in elements
template <typename F, typename C>
__global__ __launch_bounds__(256) void lanes(const F* __restrict__ field, C* __restrict__ out, const FrameSpec* __restrict__ spec,
                                             const int32_t* __restrict__ order, const int32_t* __restrict__ cstart,
                                             const double* __restrict__ phi, const int32_t* __restrict__ groups, int ncomp, int sym,
                                             int64_t sc, int64_t s2, int64_t s1, int64_t s0) {
  const FrameSpec S = *spec;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int wl = threadIdx.x & 63;
  const int gw = S.gw, per_wave = 64 / gw, w = wl & (gw - 1), sub = wl / gw;
  const int c = blockIdx.y, cin = source_line(c, S.dim, ncomp, sym);
  const int nd = S.nd;
  const int64_t node_step = (int64_t)ncomp * gw;
  C* const o = out + (int64_t)c * sc;
  for (int64_t unit = (int64_t)blockIdx.x * 4 + wave; unit < S.units; unit += (int64_t)gridDim.x * 4) {
    const int64_t chunk = unit / S.ncls;
    const int k = (int)(unit - chunk * S.ncls);
    const int64_t e = chunk * per_wave + sub;
    bool active = e < S.ngroups;
    const int64_t group = active ? (int64_t)groups[e] : 0;
    const int64_t cube = group * gw + w;
    active = active && cube < S.ncube;
    const int c0 = (int)(cube % S.n[0]), c1 = (int)(cube / S.n[0] % S.n[1]), c2 = (int)(cube / ((int64_t)S.n[0] * S.n[1]));
    active = active && (!S.fixed[0] || c0 == S.layer[0]) && (!S.fixed[1] || c1 == S.layer[1]) && (!S.fixed[2] || c2 == S.layer[2]);
    const F* const base = field + (((group * S.ncls + k) * nd) * ncomp + cin) * gw + w;
    const int q0 = cstart[k], q1 = cstart[k + 1];
    for (int qb = q0; qb < q1; qb += CHUNK) {
      int qs[CHUNK];
#pragma unroll
      for (int j = 0; j < CHUNK; ++j) qs[j] = order[min(qb + j, q1 - 1)];   // (beyond the class: its last pixel again, not stored)
      if (!active) continue;
      double v[CHUNK];
#pragma unroll
      for (int j = 0; j < CHUNK; ++j) v[j] = 0.0;
      // four nodal lines in flight; the sums still take their terms in ascending a
      int a = 0;
      for (; a + 4 <= nd; a += 4) {
        double x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) x[u] = (double)base[(a + u) * node_step];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int j = 0; j < CHUNK; ++j) v[j] = fma(phi[(int64_t)qs[j] * nd + a + u], x[u], v[j]);
      }
      for (; a < nd; ++a) {
        const double x = (double)base[a * node_step];
#pragma unroll
        for (int j = 0; j < CHUNK; ++j) v[j] = fma(phi[(int64_t)qs[j] * nd + a], x, v[j]);
      }
#pragma unroll
      for (int j = 0; j < CHUNK; ++j)
        if (qb + j < q1) o[pixel_offset(S, qs[j], c0, c1, c2, s2, s1, s0)] = (C)v[j];
    }
  }
}

template <typename F, typename C>
__global__ __launch_bounds__(256) void flat(const F* __restrict__ field, C* __restrict__ out, const FrameSpec* __restrict__ spec,
                                            const int32_t* __restrict__ cls, const double* __restrict__ phi,
                                            const int32_t* __restrict__ groups, int ncomp, int sym, int64_t sc, int64_t s2, int64_t s1,
                                            int64_t s0) {
  const FrameSpec S = *spec;
  const int c = blockIdx.y, cin = source_line(c, S.dim, ncomp, sym);
  const int nd = S.nd;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < S.units; idx += (int64_t)gridDim.x * 256) {
    const int64_t e = idx / S.Q;
    const int q = (int)(idx - e * S.Q);
    if (e >= S.ngroups) continue;
    const int64_t cube = groups[e];
    if (cube >= S.ncube) continue;
    const int c0 = (int)(cube % S.n[0]), c1 = (int)(cube / S.n[0] % S.n[1]), c2 = (int)(cube / ((int64_t)S.n[0] * S.n[1]));
    const F* const base = field + ((cube * S.ncls + cls[q]) * nd) * ncomp + cin;
    const double* const ph = phi + (int64_t)q * nd;
    double v = 0.0;
    for (int a = 0; a < nd; ++a) v = fma(ph[a], (double)base[(int64_t)a * ncomp], v);
    out[(int64_t)c * sc + pixel_offset(S, q, c0, c1, c2, s2, s1, s0)] = (C)v;
  }
}

}  // namespace frame

int launch_frame(const void* field, void* out, const FrameTablePtrs& t, int gw, int64_t units, int ncomp, int sym,
                 const int64_t stride[4], int f32, int c32, int grid, void* stream) {
  if (grid <= 0 || units <= 0 || ncomp <= 0) return 0;
  const dim3 g((unsigned)grid, (unsigned)ncomp), block(256);
  if (gw == 1) {
    // (the generic family has double blocks only)
    if (f32) return -1;
#define SG_FRAME_FLAT(CT)                                                                                                          \
  hipLaunchKernelGGL((frame::flat<double, CT>), g, block, 0, (hipStream_t)stream, (const double*)field, (CT*)out, t.spec, t.cls, t.phi, \
                     t.groups, ncomp, sym, stride[0], stride[1], stride[2], stride[3])
    if (c32) SG_FRAME_FLAT(float);
    else SG_FRAME_FLAT(double);
#undef SG_FRAME_FLAT
    return (int)hipGetLastError();
  }
  if (gw != 16 && gw != 64) return -1;
#define SG_FRAME_LANES(FT, CT)                                                                                                    \
  hipLaunchKernelGGL((frame::lanes<FT, CT>), g, block, 0, (hipStream_t)stream, (const FT*)field, (CT*)out, t.spec, t.order, t.cstart, \
                     t.phi, t.groups, ncomp, sym, stride[0], stride[1], stride[2], stride[3])
  if (f32 && c32) SG_FRAME_LANES(float, float);
  else if (f32) SG_FRAME_LANES(float, double);
  else if (c32) SG_FRAME_LANES(double, float);
  else SG_FRAME_LANES(double, double);
#undef SG_FRAME_LANES
  return (int)hipGetLastError();
}

}  // namespace sg
