// Peak maps on the device (include/seigen_hip.h sg_set_peaks): at the end of a sample step, behind the spectra and before the
// injectors, every node of the block compares the squared magnitude of a selected field with its running maximum,
//   m = x_0 x_0;  m = m + (x_c x_c)  over the field's lines c ascending;   if (m > val) { val = m; idx = j; }
// in double, every product and every sum rounded on its own (FP32 blocks convert x first: exact).  The velocity has the lines
// c = 0 .. dim - 1, a stress in full storage all dim^2, a stress in symmetric storage the i <= j ones with an off-diagonal
// line entering as 2 (x x) - the doubling is exact - and the i > j lines, which that storage leaves stale, are not read.
// The comparison is strict: the earliest sample wins a tie, a NaN never enters, a node that never moved keeps idx = -1.
//
// val (double) and idx (int32) have the field's device layout with one component: node word w = (item * nd + a) * gw + lane
// has its lines at ((item * nd + a) * ncomp + c) * gw + lane.  The pass is flat over the node words.  A thread owns 16 bytes
// of each of a node's lines at a time - two doubles or four floats - and the same words of val and idx, where gw is a multiple
// of that (gw = 16, 64); gw = 1 takes the words one by one.  The grid strides over the words with 64-bit indices.  val and idx
// are stored only where some word of the thread exceeded.  A word has one writer and the order of a word's updates is the order
// of the samples: the bits depend only on the field contents.  A step that is no sample step, or one beyond the series, costs
// a launch whose threads exit at once (graph replay: the step comes from the device-side counter).  No atomics, no LDS.
//
// gather moves val and idx to the caller's [cell][node] order, cell = cube * ncls + cls, and drops the padding cubes: a thread
// per device word, contiguous on the device side.  It is a read-out, not part of a step.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.hpp"

namespace sg {
namespace peak {

typedef double d2 __attribute__((ext_vector_type(2)));

template <typename T>
struct Vec;
template <>
struct Vec<double> {
  static constexpr int N = 2;
  typedef double type __attribute__((ext_vector_type(2)));
  typedef int32_t itype __attribute__((ext_vector_type(2)));
};
template <>
struct Vec<float> {
  static constexpr int N = 4;
  typedef float type __attribute__((ext_vector_type(4)));
  typedef int32_t itype __attribute__((ext_vector_type(4)));
};

// the sample of this launch, or -1: no sample step, or beyond the series (as spectra::sample_of)
__device__ __forceinline__ int64_t sample_of(const int64_t* ctr, int64_t step_by_value, int64_t every, int64_t nsamples) {
  const int64_t step = ctr != nullptr ? *ctr + 1 : step_by_value;
  if (step < 1 || step % every != 0) return -1;
  const int64_t j = step / every - 1;
  return j < nsamples ? j : -1;
}

// line c of a field with ncomp lines: 0 - not read (i > j in symmetric storage), 1 - enters as x x, 2 - as 2 (x x)
__device__ __forceinline__ int line_weight(int c, int dim, int sym) {
  if (!sym) return 1;
  const int i = c / dim, j = c % dim;
  return i > j ? 0 : (i < j ? 2 : 1);
}

// the term of one nodal value, rounded product by product
__device__ __forceinline__ double term(double x, int weight) {
  const double t = __dmul_rn(x, x);
  return weight == 2 ? __dmul_rn(2.0, t) : t;
}

// n: the node words; gw = 1 << gw_shift; sym: x is a stress (ncomp = dim^2) in symmetric storage
template <typename T>
__global__ __launch_bounds__(256) void update(const T* __restrict__ x, double* __restrict__ val, int32_t* __restrict__ idx,
                                              const int64_t* ctr, int64_t step, int64_t every, int64_t nsamples, int64_t n,
                                              int gw_shift, int ncomp, int dim, int sym) {
  constexpr int V = Vec<T>::N;
  typedef typename Vec<T>::type vT;
  typedef typename Vec<T>::itype vI;
  const int64_t js = sample_of(ctr, step, every, nsamples);
  if (js < 0) return;
  const int32_t j = (int32_t)js;
  const int64_t gw = (int64_t)1 << gw_shift;
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nthreads = (int64_t)gridDim.x * blockDim.x;
  if (gw % V == 0) {   // the words of a 16-byte access lie on one line
    const int64_t nvec = n / V;   // (n is a multiple of gw)
    for (int64_t i = tid; i < nvec; i += nthreads) {
      const int64_t w0 = i * V, row = w0 >> gw_shift, lane = w0 & (gw - 1);
      const T* const p = x + ((row * ncomp) << gw_shift) + lane;
      double m[V];
      bool first = true;
      for (int c = 0; c < ncomp; ++c) {
        const int weight = line_weight(c, dim, sym);
        if (weight == 0) continue;
        const vT xv = *(const vT*)(p + ((int64_t)c << gw_shift));
#pragma unroll
        for (int k = 0; k < V; ++k) {
          const double t = term((double)xv[k], weight);
          m[k] = first ? t : __dadd_rn(m[k], t);
        }
        first = false;
      }
      d2 v[V / 2];
#pragma unroll
      for (int q = 0; q < V / 2; ++q) v[q] = *(const d2*)(val + w0 + 2 * q);
      bool any = false, up[V];
#pragma unroll
      for (int k = 0; k < V; ++k) {
        up[k] = m[k] > v[k / 2][k % 2];
        any = any || up[k];
      }
      if (!any) continue;
      vI s = *(const vI*)(idx + w0);
#pragma unroll
      for (int k = 0; k < V; ++k)
        if (up[k]) {
          v[k / 2][k % 2] = m[k];
          s[k] = j;
        }
#pragma unroll
      for (int q = 0; q < V / 2; ++q) *(d2*)(val + w0 + 2 * q) = v[q];
      *(vI*)(idx + w0) = s;
    }
    return;
  }
  for (int64_t w = tid; w < n; w += nthreads) {
    const int64_t row = w >> gw_shift, lane = w & (gw - 1);
    const T* const p = x + ((row * ncomp) << gw_shift) + lane;
    double m = 0.0;
    bool first = true;
    for (int c = 0; c < ncomp; ++c) {
      const int weight = line_weight(c, dim, sym);
      if (weight == 0) continue;
      const double t = term((double)p[(int64_t)c << gw_shift], weight);
      m = first ? t : __dadd_rn(m, t);
      first = false;
    }
    if (m > val[w]) {
      val[w] = m;
      idx[w] = j;
    }
  }
}

// device word w = (item * nd + a) * gw + lane -> out[(cube * ncls + cls) * nd + a], item = group * ncls + cls, cube = group * gw +
// lane < ncube; C: the caller's type of the values; either output may be null
template <typename C>
__global__ __launch_bounds__(256) void gather(const double* __restrict__ val, const int32_t* __restrict__ idx, C* __restrict__ out_val,
                                              int32_t* __restrict__ out_idx, int64_t n, int gw_shift, int nd, int ncls, int64_t ncube) {
  const int64_t gw = (int64_t)1 << gw_shift;
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nthreads = (int64_t)gridDim.x * blockDim.x;
  for (int64_t w = tid; w < n; w += nthreads) {
    const int64_t row = w >> gw_shift, lane = w & (gw - 1);
    const int64_t item = row / nd, a = row - item * nd;
    const int64_t group = item / ncls, cls = item - group * ncls;
    const int64_t cube = (group << gw_shift) + lane;
    if (cube >= ncube) continue;
    const int64_t o = (cube * ncls + cls) * nd + a;
    if (out_val != nullptr) out_val[o] = (C)val[w];
    if (out_idx != nullptr) out_idx[o] = idx[w];
  }
}

static int shift_of(int gw) {
  for (int s = 0; s < 31; ++s)
    if (gw == 1 << s) return s;
  return -1;
}

}  // namespace peak

int launch_peak_update(const void* field, double* val, int32_t* idx, const int64_t* ctr, int64_t step, int64_t every, int64_t nsamples,
                       int64_t n, int gw, int ncomp, int dim, int sym, int f32, int grid, void* stream) {
  if (n <= 0) return 0;
  const int gw_shift = peak::shift_of(gw);
  if (gw_shift < 0 || n % gw != 0 || ncomp < 1) return -1;
  const int V = gw % (f32 ? 4 : 2) == 0 ? (f32 ? 4 : 2) : 1;
  const int64_t want = ((n + V - 1) / V + 255) / 256;
  const dim3 g((unsigned)std::max<int64_t>(1, std::min<int64_t>(want, grid > 0 ? grid : 1))), block(256);
  if (ncomp != dim * dim) sym = 0;   // the line rule belongs to a tensor
  if (f32)
    hipLaunchKernelGGL(peak::update<float>, g, block, 0, (hipStream_t)stream, (const float*)field, val, idx, ctr, step, every, nsamples, n,
                       gw_shift, ncomp, dim, sym);
  else
    hipLaunchKernelGGL(peak::update<double>, g, block, 0, (hipStream_t)stream, (const double*)field, val, idx, ctr, step, every, nsamples, n,
                       gw_shift, ncomp, dim, sym);
  return (int)hipGetLastError();
}

int launch_peak_gather(const double* val, const int32_t* idx, void* out_val, int c32, int32_t* out_idx, int64_t n, int gw, int nd, int ncls,
                       int64_t ncube, int grid, void* stream) {
  if (n <= 0 || (out_val == nullptr && out_idx == nullptr)) return 0;
  const int gw_shift = peak::shift_of(gw);
  if (gw_shift < 0 || nd < 1 || ncls < 1) return -1;
  const int64_t want = (n + 255) / 256;
  const dim3 g((unsigned)std::max<int64_t>(1, std::min<int64_t>(want, grid > 0 ? grid : 1))), block(256);
  if (c32)
    hipLaunchKernelGGL(peak::gather<float>, g, block, 0, (hipStream_t)stream, val, idx, (float*)out_val, out_idx, n, gw_shift, nd, ncls, ncube);
  else
    hipLaunchKernelGGL(peak::gather<double>, g, block, 0, (hipStream_t)stream, val, idx, (double*)out_val, out_idx, n, gw_shift, nd, ncls, ncube);
  return (int)hipGetLastError();
}

}  // namespace sg
