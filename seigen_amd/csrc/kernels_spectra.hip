// Running Fourier transforms of the wavefield on the device (include/seigen_hip.h sg_set_spectra): at the end of a sample
// step, behind the recorder and the monitor and before the injectors, every word x of a selected field enters the
// accumulators of all armed frequencies,
//   re[f] = fma(w_re, x, re[f]),   im[f] = fma(w_im, x, im[f]),   (w_re, w_im) = w[sample][f]
// in double (FP32 blocks convert x first: exact).  The accumulators have the field's own device layout, so the pass is flat:
// no cell, node or item is looked at, only the line (idx / gw) % ncomp of a stress word, which tells the i > j lines that
// symmetric storage leaves stale - they are skipped, reads included.
//
// One launch per field and sample reads the field once and updates all 2 nfreq accumulators: (1 + 4 nfreq) words of traffic
// per field word.  A thread owns 16 bytes of the field at a time - two doubles or four floats - and the same words of every
// accumulator, as 16-byte loads and stores; the grid strides over the buffer with 64-bit indices.  A word has one writer, the
// order of a word's updates is the order of the samples: the bits depend only on the field contents and the weights.  A step
// that is no sample step, or one beyond the series, costs a launch whose threads exit at once (graph replay: the step comes
// from the device-side counter).  No atomics, no LDS.
//
// The accumulators are read and written with plain accesses: they are far larger than the L2s and next touched a sample
// later, but on this chip a non-temporal access by-passes the L1 only - the line stays in the L2 either way, and 16-byte
// non-temporal loads measure 0 to 3 % slower than plain ones - so there is nothing to gain.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.hpp"

namespace sg {
namespace spectra {

typedef double d2 __attribute__((ext_vector_type(2)));

template <typename T>
struct Vec;
template <>
struct Vec<double> {
  static constexpr int N = 2;
  typedef double type __attribute__((ext_vector_type(2)));
};
template <>
struct Vec<float> {
  static constexpr int N = 4;
  typedef float type __attribute__((ext_vector_type(4)));
};

// the sample of this launch, or -1: no sample step, or beyond the series
__device__ __forceinline__ int64_t sample_of(const Args& A) {
  const int64_t step = A.ctr != nullptr ? *A.ctr + 1 : A.step;
  if (step < 1 || step % A.every != 0) return -1;
  const int64_t j = step / A.every - 1;
  return j < A.nsamples ? j : -1;
}

__device__ __forceinline__ bool kept(const Args& A, int64_t idx) {
  if (!A.sym) return true;
  const int c = (int)((idx / A.gw) % A.ncomp);
  return c / A.dim <= c % A.dim;
}

template <typename T>
__global__ __launch_bounds__(256) void accumulate(const T* __restrict__ x, Args A) {
  constexpr int V = Vec<T>::N;
  typedef typename Vec<T>::type vT;
  const int64_t j = sample_of(A);
  if (j < 0) return;
  const double* w = A.w + j * A.nfreq * 2;
  const int64_t nvec = A.n / V;
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nthreads = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = tid; i < nvec; i += nthreads) {
    const int64_t idx = i * V;
    bool keep[V];
    bool any = false;
    if (A.vec_line) {   // gw is a multiple of V: the words of a vector lie on one line
      any = kept(A, idx);
#pragma unroll
      for (int k = 0; k < V; ++k) keep[k] = any;
    } else {
#pragma unroll
      for (int k = 0; k < V; ++k) {
        keep[k] = kept(A, idx + k);
        any = any || keep[k];
      }
    }
    if (!any) continue;
    const vT xv = *(const vT*)(x + idx);
    double xd[V];
#pragma unroll
    for (int k = 0; k < V; ++k) xd[k] = (double)xv[k];
    for (int f = 0; f < A.nfreq; ++f) {
#pragma unroll
      for (int part = 0; part < 2; ++part) {
        const double wp = w[2 * f + part];
        double* acc = A.acc + (int64_t)(2 * f + part) * A.n + idx;
        d2 v[V / 2];
#pragma unroll
        for (int p = 0; p < V / 2; ++p) v[p] = *(const d2*)(acc + 2 * p);
#pragma unroll
        for (int k = 0; k < V; ++k)
          if (keep[k]) v[k / 2][k % 2] = fma(wp, xd[k], v[k / 2][k % 2]);
#pragma unroll
        for (int p = 0; p < V / 2; ++p) *(d2*)(acc + 2 * p) = v[p];
      }
    }
  }
  // the words behind the last whole vector (none in the interleaved layouts)
  for (int64_t idx = nvec * V + tid; idx < A.n; idx += nthreads) {
    if (!kept(A, idx)) continue;
    const double xd = (double)x[idx];
    for (int f = 0; f < A.nfreq; ++f)
      for (int part = 0; part < 2; ++part) {
        double* acc = A.acc + (int64_t)(2 * f + part) * A.n + idx;
        *acc = fma(w[2 * f + part], xd, *acc);
      }
  }
}

}  // namespace spectra

int launch_spectra(const void* field, const spectra::Args& a, int f32, int grid, void* stream) {
  if (a.n <= 0 || a.nfreq <= 0) return 0;
  const int V = f32 ? 4 : 2;
  const int64_t want = ((a.n + V - 1) / V + 255) / 256;
  const dim3 g((unsigned)std::max<int64_t>(1, std::min<int64_t>(want, grid > 0 ? grid : 1))), block(256);
  if (f32)
    hipLaunchKernelGGL(spectra::accumulate<float>, g, block, 0, (hipStream_t)stream, (const float*)field, a);
  else
    hipLaunchKernelGGL(spectra::accumulate<double>, g, block, 0, (hipStream_t)stream, (const double*)field, a);
  return (int)hipGetLastError();
}

}  // namespace sg
