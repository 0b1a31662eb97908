// Gauges (include/seigen_hip.h sg_set_gauges / sg_probe_gradient): the broken gradient of the velocity - or its divergence, curl
// or symmetric part - at a few physical points, taken inside the time loop at the end of every `every`-th step, or once behind
// everything queued.  The arithmetic is kernels.hpp gauge::Args's: the gradient's (kernels_grad.hip) with the dense row at the
// point's reference coordinates in place of the row at a node.
//
// One wave per owned gauge, four waves a block, the grid striding over the gauges.  A gauge reads nd * dim nodal values of one
// cell, each on a line of its own in the interleaved layouts; one thread walking them (the shape of receiver_sample) would make
// every load wait for the one before it.  Here
//   load     the 64 lanes fetch the nd * dim values - word t = a * dim + i of the cell at (item * nd * dim + t) * gw + lane - and the
//            dim * nd weights of the gauge as independent loads, ceil(nd * dim / 64) a lane, into the wave's own LDS slab, as doubles;
//   chain    lane (r, i) runs t_r[i] over a ascending from the slab with fma from zero;
//   map      lane (i, j) forms G_ij over r ascending with fma from zero;
//   store    lane c forms component c of the kind and writes it.
// The phases of a wave meet at the block's barriers: a slab is read by other lanes than wrote it, never by another wave.  The
// order of every sum is fixed and there are no atomics: the samples are bitwise the same under graph replay and eager launches,
// for one sg_step(n) and n calls of sg_step(1), for host-driven stages, in every layout and on a split block.  A step that is
// not a sample step costs one launch whose threads exit at once.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.hpp"

namespace sg {
namespace gauge {

constexpr int SLAB = 2 * MAX_VALUES + 18;   // values, weights, t[dim][dim], G[dim][dim]

// component c of the kind from G[i * dim + j], in the order and with the roundings the header states
__device__ __forceinline__ double combine(const double* G, int dim, int kind, int c) {
#pragma clang fp contract(off)
  if (kind == 0) return G[c];
  if (kind == 1) {
    double s = G[0];
    for (int i = 1; i < dim; ++i) s = s + G[i * dim + i];
    return s;
  }
  if (kind == 2) {
    if (dim == 2) return G[2] - G[1];
    if (c == 0) return G[7] - G[5];
    if (c == 1) return G[2] - G[6];
    return G[3] - G[1];
  }
  const int i = c / dim, j = c - i * dim;
  if (i == j) return G[c];
  const double s = G[i * dim + j] + G[j * dim + i];
  return 0.5 * s;
}

// the scalars are kernels.hpp gauge::Args member by member (the kernels take pointers and built-in scalars only)
template <typename T>
__global__ __launch_bounds__(256) void sample(const T* __restrict__ u, const int64_t* ctr, int64_t step_by_value, int64_t every,
                                              int64_t capacity, const int64_t* __restrict__ item, const int32_t* __restrict__ lane_of,
                                              const int32_t* __restrict__ cls, const double* __restrict__ D, const double* __restrict__ J,
                                              double* __restrict__ out, int64_t nown, int ncomp, int kind, int dim_, int nd_, int gw) {
  const Args A{ctr, step_by_value, every, capacity, item, lane_of, cls, D, J, out, nown, ncomp, kind, dim_, nd_, gw, 0};
  __shared__ double lds[4][SLAB];
  const int64_t step = A.ctr != nullptr ? *A.ctr + 1 : A.step;
  if (step <= 0 || step % A.every != 0) return;
  const int64_t j = step / A.every - 1;
  if (j >= A.capacity) return;
  const int wave = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int dim = A.dim, nd = A.nd, nv = nd * dim, dd = dim * dim;
  double* const ul = lds[wave];
  double* const dl = ul + MAX_VALUES;
  double* const tl = dl + MAX_VALUES;
  double* const gl = tl + 9;
  // (the trip count is the block's: every wave meets every barrier, with a gauge or without)
  for (int64_t first = (int64_t)blockIdx.x * 4; first < A.nown; first += (int64_t)gridDim.x * 4) {
    const int64_t g = first + wave;
    const bool active = g < A.nown;
    if (active) {
      const int64_t word0 = A.item[g] * nv, lane = A.lane[g];
      const double* const Dg = A.D + g * nv;
      for (int t = l; t < nv; t += 64) {
        ul[t] = (double)u[(word0 + t) * A.gw + lane];
        dl[t] = Dg[t];
      }
    }
    __syncthreads();
    if (active && l < dd) {
      const int r = l / dim, i = l - r * dim;
      const double* const row = dl + r * nd;
      double acc = 0.0;
      for (int a = 0; a < nd; ++a) acc = fma(row[a], ul[a * dim + i], acc);
      tl[r * dim + i] = acc;
    }
    __syncthreads();
    if (active && l < dd) {
      const int i = l / dim, jj = l - i * dim;
      const double* const Jk = A.J + A.cls[g] * 9;
      double acc = 0.0;
      for (int r = 0; r < dim; ++r) acc = fma(Jk[r * 3 + jj], tl[r * dim + i], acc);
      gl[i * dim + jj] = acc;
    }
    __syncthreads();
    if (active && l < A.ncomp) A.out[(j * A.nown + g) * A.ncomp + l] = combine(gl, dim, A.kind, l);
  }
}

}  // namespace gauge

int launch_gauges(const void* field, const gauge::Args& a, int f32, void* stream) {
  if (a.nown <= 0) return 0;
  if (a.dim < 1 || a.dim > 3 || a.nd < 1 || a.nd * a.dim > gauge::MAX_VALUES || a.gw < 1) return -1;
  if (a.ncomp < 1 || a.ncomp > a.dim * a.dim || a.kind < 0 || a.kind > 3) return -1;
  const dim3 grid((unsigned)std::min<int64_t>((a.nown + 3) / 4, gauge::GRID_CAP)), block(256);
#define SG_GAUGE_ARGS \
  a.ctr, a.step, a.every, a.capacity, a.item, a.lane, a.cls, a.D, a.J, a.out, a.nown, a.ncomp, a.kind, a.dim, a.nd, a.gw
  if (f32)
    hipLaunchKernelGGL(gauge::sample<float>, grid, block, 0, (hipStream_t)stream, (const float*)field, SG_GAUGE_ARGS);
  else
    hipLaunchKernelGGL(gauge::sample<double>, grid, block, 0, (hipStream_t)stream, (const double*)field, SG_GAUGE_ARGS);
#undef SG_GAUGE_ARGS
  return (int)hipGetLastError();
}

}  // namespace sg
