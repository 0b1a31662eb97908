// Receiver samples on the device (include/seigen_hip.h sg_set_receivers): the value of the velocity and / or the stress at
// a few physical points, taken inside the time loop at the end of every `every`-th step - what the reference's receiver
// script does by writing a VTU file per step and probing it on the host (tests/explosive_source/uy.py:31-43).
//
// One thread per (owned receiver, component): sum_a phi_a(xi) field[cell][a][c] over the cell's nodes in ascending order,
// in double with fma.  The order is fixed, so the samples are bitwise the same under graph replay and eager launches, for
// one sg_step(n) and n calls of sg_step(1), for host-driven stages, and on a split block (whose fields equal the single
// block's bitwise).  A step that is not a sample step costs one launch whose threads exit at once.  No atomics, no LDS.
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace sg {

template <typename T>
__global__ __launch_bounds__(256) void receiver_sample(const T* __restrict__ u, const T* __restrict__ s, RecvArgs A) {
  const int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (idx >= A.nown * A.ncomp) return;
  const int64_t step = A.ctr != nullptr ? *A.ctr + 1 : A.step;
  if (step <= 0 || step % A.every != 0) return;
  const int64_t j = step / A.every - 1;
  if (j >= A.capacity) return;
  const int64_t r = idx / A.ncomp;
  const int q = (int)(idx - r * A.ncomp);
  const T* f = u;
  int c = q, nc = A.dim;
  if (q >= A.nu) {
    f = s;
    c = q - A.nu;
    nc = A.dim * A.dim;
    const int i = c / A.dim, k = c - i * A.dim;
    if (A.sym && i > k) c = k * A.dim + i;     // symmetric-stress storage: the lower triangle is stale, read the mirror
  }
  const int64_t base = A.item[r] * A.nd;
  const int64_t lane = A.lane[r];
  const double* phi = A.phi + r * A.nd;
  double v = 0.0;
  for (int a = 0; a < A.nd; ++a) v = fma(phi[a], (double)f[((base + a) * nc + c) * A.gw + lane], v);
  A.trace[(j * A.nown + r) * A.ncomp + q] = v;
}

int launch_receivers(const void* u, const void* s, const RecvArgs& a, int f32, void* stream) {
  const int64_t total = a.nown * a.ncomp;
  if (total <= 0) return 0;
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  if (f32)
    hipLaunchKernelGGL(receiver_sample<float>, grid, block, 0, (hipStream_t)stream, (const float*)u, (const float*)s, a);
  else
    hipLaunchKernelGGL(receiver_sample<double>, grid, block, 0, (hipStream_t)stream, (const double*)u, (const double*)s, a);
  return (int)hipGetLastError();
}

}  // namespace sg
