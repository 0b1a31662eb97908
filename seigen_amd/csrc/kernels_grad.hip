// The gradient (include/seigen_hip.h sg_get_gradient_dev): the broken gradient of a velocity field at the nodes, and the
// divergence, curl and symmetric strain rate made of it.  For the cell of class k, node a, velocity component i:
//   t_r[a][i] = sum_b C_r[a][b] * (double)u[b][i]      over b ascending with fma from zero - simplices over the dense row,
//                                                      tensor-product cells over the n1 = P + 1 nodes of the line through a
//                                                      along axis r, b = a + (be - a_r) * n1^r, with the 1-D matrix C1[a_r][be]
//   G_ij[a]   = sum_r J[k][r][j] * t_r[a][i]           over r ascending with fma from zero
// and the kind's values by combine() below, every operation rounded on its own (no contraction).  One arithmetic, node_values(),
// in both kernels: the bits do not depend on the layout.
//
// lanes (gw = 16, 64): a workgroup of four waves takes a UNIT - (item = group * ncls + class, slice of nodes_per_slice output
//   nodes; hostlogic.hpp grad_plan) - in three phases:
//   load     the item's velocity block [row = node * dim + comp][lane < gw], one contiguous run of nd * dim * gw words, into an
//            LDS image of doubles [row][pitch = gw + 1]: thread t moves word t, t + 256, ... - whole 128-byte (gw = 16) or
//            512-byte (gw = 64) lines, as xfer::tiled reads them;
//   compute  thread (lane w = t & (gw - 1), sub = t / gw) walks the slice's nodes a0 + sub, a0 + sub + 256 / gw, ...: the sums
//            from the image (a lane-fastest walk: stride 1 in w, the threads of a wave that share w read one word), the values
//            into a second image [(a - a0) * ncomp + c][pitch] behind the first;
//   store    a wave takes one cell's run of nr * ncomp words at a time, 64 consecutive words per pass, converted (C)v: the
//            second half of xfer::tiled.
//   A lane whose cell lies outside the range, or is layout padding, is neither read nor written in any phase.
// flat (gw = 1): a thread per (cell, node) of the range, node fastest; nodal values and tables are per-thread reads.
// The grid strides over the units (chunks of 256 threads) beyond its cap.  All index arithmetic is 64-bit.
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace sg {
namespace grad {

// the kind's values from G, in the order and with the roundings the header states
template <int DIM>
__device__ __forceinline__ void combine(const double (&G)[DIM][DIM], int kind, double (&v)[DIM * DIM]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int c = 0; c < DIM * DIM; ++c) v[c] = 0.0;
  if (kind == 0) {
#pragma unroll
    for (int i = 0; i < DIM; ++i)
#pragma unroll
      for (int j = 0; j < DIM; ++j) v[i * DIM + j] = G[i][j];
  } else if (kind == 1) {
    double s = G[0][0];
#pragma unroll
    for (int i = 1; i < DIM; ++i) s = s + G[i][i];
    v[0] = s;
  } else if (kind == 2) {
    if constexpr (DIM == 3) {
      v[0] = G[2][1] - G[1][2];
      v[1] = G[0][2] - G[2][0];
      v[2] = G[1][0] - G[0][1];
    } else if constexpr (DIM == 2) {
      v[0] = G[1][0] - G[0][1];
    }
  } else {
#pragma unroll
    for (int i = 0; i < DIM; ++i)
#pragma unroll
      for (int j = 0; j < DIM; ++j) {
        const double s = G[i][j] + G[j][i];
        v[i * DIM + j] = i == j ? G[i][i] : 0.5 * s;
      }
  }
}

// the values of node a; u(b, i) delivers nodal value (b, i) of the cell as a double
template <int DIM, typename Load>
__device__ __forceinline__ void node_values(const GradArgs& A, const double* __restrict__ Ctab, const double* __restrict__ Jk, int a,
                                            Load u, double (&v)[DIM * DIM]) {
  double t[DIM][DIM];   // [r][i]
#pragma unroll
  for (int r = 0; r < DIM; ++r)
#pragma unroll
    for (int i = 0; i < DIM; ++i) t[r][i] = 0.0;
  const int nd = A.nd;
  if (A.n1 == 0) {
    const double* const row = Ctab + (int64_t)a * nd;
    const int64_t plane = (int64_t)nd * nd;
    for (int b = 0; b < nd; ++b) {
      double x[DIM];
#pragma unroll
      for (int i = 0; i < DIM; ++i) x[i] = u(b, i);
#pragma unroll
      for (int r = 0; r < DIM; ++r) {
        const double c = row[r * plane + b];
#pragma unroll
        for (int i = 0; i < DIM; ++i) t[r][i] = fma(c, x[i], t[r][i]);
      }
    }
  } else {
    const int n1 = A.n1;
    int stride = 1;
#pragma unroll
    for (int r = 0; r < DIM; ++r) {
      const int ar = a / stride % n1, base = a - ar * stride;
      const double* const row = Ctab + ar * n1;
      for (int be = 0; be < n1; ++be) {
        const double c = row[be];
        const int b = base + be * stride;
#pragma unroll
        for (int i = 0; i < DIM; ++i) t[r][i] = fma(c, u(b, i), t[r][i]);
      }
      stride *= n1;
    }
  }
  double G[DIM][DIM];
#pragma unroll
  for (int i = 0; i < DIM; ++i)
#pragma unroll
    for (int j = 0; j < DIM; ++j) {
      double g = 0.0;
#pragma unroll
      for (int r = 0; r < DIM; ++r) g = fma(Jk[r * 3 + j], t[r][i], g);
      G[i][j] = g;
    }
  combine<DIM>(G, A.kind, v);
}

template <typename F, typename C, int DIM>
__device__ __forceinline__ void lanes_body(const F* __restrict__ field, C* __restrict__ out, const double* __restrict__ Ctab,
                                           const double* __restrict__ Jtab, const GradArgs& A, unsigned char* lds_raw) {
  double* const img = reinterpret_cast<double*>(lds_raw);
  double* const val = reinterpret_cast<double*>(lds_raw + A.out_offset);
  const int gw = A.gw, gw_shift = gw == 16 ? 4 : 6, pitch = A.pitch, ncomp = A.ncomp, nd = A.nd, ncls = A.ncls;
  const int tid = threadIdx.x, wave = tid >> 6, wl = tid & 63;
  const int w = tid & (gw - 1), sub = tid >> gw_shift, nsub = 256 >> gw_shift;
  const int rows_in = nd * DIM;
  for (int64_t unit = blockIdx.x; unit < A.units; unit += gridDim.x) {
    const int64_t item = A.item0 + unit / A.slices;
    const int a0 = (int)(unit % A.slices) * A.nodes_per_slice;
    const int nr = min(A.nodes_per_slice, nd - a0);
    const int64_t group = item / ncls;
    const int cls = (int)(item % ncls);
    // the cell of lane w is ((group << gw_shift) + w) * ncls + cls; in the range for rel = cell - cell0 in 0 .. ncells - 1
    const int64_t rel0 = (group << gw_shift) * ncls + cls - A.cell0;
    const F* const dev0 = field + item * rows_in * gw;
    for (int t = tid; t < rows_in << gw_shift; t += 256) {
      const int r = t >> gw_shift, wt = t & (gw - 1);
      const int64_t rel = rel0 + (int64_t)wt * ncls;
      if (rel < 0 || rel >= A.ncells) continue;
      img[r * pitch + wt] = (double)dev0[t];
    }
    __syncthreads();
    const int64_t relw = rel0 + (int64_t)w * ncls;
    if (relw >= 0 && relw < A.ncells) {
      const double* const Jk = Jtab + cls * 9;
      const double* const mine = img + w;
      for (int la = sub; la < nr; la += nsub) {
        double v[DIM * DIM];
        node_values<DIM>(A, Ctab, Jk, a0 + la, [&](int b, int i) { return mine[(b * DIM + i) * pitch]; }, v);
        double* const o = val + (int64_t)la * ncomp * pitch + w;
#pragma unroll
        for (int c = 0; c < DIM * DIM; ++c)
          if (c < ncomp) o[c * pitch] = v[c];
      }
    }
    __syncthreads();
    for (int wt = wave; wt < gw; wt += 4) {
      const int64_t rel = rel0 + (int64_t)wt * ncls;
      if (rel < 0 || rel >= A.ncells) continue;
      C* const run = out + (rel * nd + a0) * ncomp;
      for (int r = wl; r < nr * ncomp; r += 64) run[r] = (C)val[r * pitch + wt];
    }
    __syncthreads();   // the images are free for the next unit
  }
}

// F: the block's word type, C: the caller's; the scalars are kernels.hpp GradArgs member by member (the kernels take pointers
// and built-in scalars only)
template <typename F, typename C>
__global__ __launch_bounds__(256) void lanes(const F* __restrict__ field, C* __restrict__ out, const double* __restrict__ Ctab,
                                             const double* __restrict__ Jtab, int64_t item0, int64_t units, int64_t cell0, int64_t ncells, int slices,
                                             int nodes_per_slice, int pitch, int out_offset, int gw, int ncls, int nd, int dim, int ncomp,
                                             int kind, int n1) {
  const GradArgs A{item0, units, cell0, ncells, slices, nodes_per_slice, pitch, out_offset, gw, ncls, nd, dim, ncomp, kind, n1, 0};
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  if (A.dim == 3) lanes_body<F, C, 3>(field, out, Ctab, Jtab, A, lds_raw);
  else if (A.dim == 2) lanes_body<F, C, 2>(field, out, Ctab, Jtab, A, lds_raw);
  else lanes_body<F, C, 1>(field, out, Ctab, Jtab, A, lds_raw);
}

template <typename F, typename C, int DIM>
__device__ __forceinline__ void flat_body(const F* __restrict__ field, C* __restrict__ out, const double* __restrict__ Ctab,
                                          const double* __restrict__ Jtab, const GradArgs& A) {
  const int nd = A.nd, ncomp = A.ncomp;
  const int64_t n = A.ncells * nd;
  for (int64_t unit = blockIdx.x; unit < A.units; unit += gridDim.x) {
    const int64_t idx = unit * 256 + threadIdx.x;
    if (idx >= n) continue;
    const int64_t rel = idx / nd, cell = A.cell0 + rel;
    const int a = (int)(idx - rel * nd);
    const F* const base = field + cell * nd * DIM;
    double v[DIM * DIM];
    node_values<DIM>(A, Ctab, Jtab + (int)(cell % A.ncls) * 9, a, [&](int b, int i) { return (double)base[b * DIM + i]; }, v);
    C* const o = out + idx * ncomp;
#pragma unroll
    for (int c = 0; c < DIM * DIM; ++c)
      if (c < ncomp) o[c] = (C)v[c];
  }
}

template <typename F, typename C>
__global__ __launch_bounds__(256) void flat(const F* __restrict__ field, C* __restrict__ out, const double* __restrict__ Ctab,
                                            const double* __restrict__ Jtab, int64_t item0, int64_t units, int64_t cell0, int64_t ncells, int slices,
                                            int nodes_per_slice, int pitch, int out_offset, int gw, int ncls, int nd, int dim, int ncomp,
                                            int kind, int n1) {
  const GradArgs A{item0, units, cell0, ncells, slices, nodes_per_slice, pitch, out_offset, gw, ncls, nd, dim, ncomp, kind, n1, 0};
  if (A.dim == 3) flat_body<F, C, 3>(field, out, Ctab, Jtab, A);
  else if (A.dim == 2) flat_body<F, C, 2>(field, out, Ctab, Jtab, A);
  else flat_body<F, C, 1>(field, out, Ctab, Jtab, A);
}

}  // namespace grad

int launch_grad(const void* field, void* out, const double* C, const double* J, const GradArgs& a, int f32, int c32, int grid,
                size_t lds_bytes, void* stream) {
  if (a.ncells <= 0 || a.units <= 0 || grid <= 0) return 0;
  if (a.dim < 1 || a.dim > 3 || a.ncomp < 1 || a.ncomp > a.dim * a.dim) return -1;
  const dim3 g((unsigned)grid), block(256);
#define SG_GRAD_SCALARS \
  a.item0, a.units, a.cell0, a.ncells, a.slices, a.nodes_per_slice, a.pitch, a.out_offset, a.gw, a.ncls, a.nd, a.dim, a.ncomp, a.kind, a.n1
  if (a.gw == 1) {
    // (the generic family has double blocks only)
    if (f32) return -1;
    if (c32) hipLaunchKernelGGL((grad::flat<double, float>), g, block, 0, (hipStream_t)stream, (const double*)field, (float*)out, C, J, SG_GRAD_SCALARS);
    else hipLaunchKernelGGL((grad::flat<double, double>), g, block, 0, (hipStream_t)stream, (const double*)field, (double*)out, C, J, SG_GRAD_SCALARS);
    return (int)hipGetLastError();
  }
  if (a.gw != 16 && a.gw != 64) return -1;
#define SG_GRAD_LANES(FT, CT) \
  hipLaunchKernelGGL((grad::lanes<FT, CT>), g, block, lds_bytes, (hipStream_t)stream, (const FT*)field, (CT*)out, C, J, SG_GRAD_SCALARS)
  if (f32 && c32) SG_GRAD_LANES(float, float);
  else if (f32) SG_GRAD_LANES(float, double);
  else if (c32) SG_GRAD_LANES(double, float);
  else SG_GRAD_LANES(double, double);
#undef SG_GRAD_LANES
#undef SG_GRAD_SCALARS
  return (int)hipGetLastError();
}

}  // namespace sg
