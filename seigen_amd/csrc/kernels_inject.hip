// Point injectors on the device (include/seigen_hip.h sg_inject / sg_set_injectors): force and stress amplitudes added at a
// few physical points inside the time loop, at the end of a step - the transpose of the recorder (kernels_recv.hip).  Where
// that forms sum_a phi_a(xi) field[cell][a][c], this adds amp * psi_a to the same words, psi = Mhat^-1 phi(xi) / |det J|
// (tabulated on the host, hostapi.cpp injector_plan): the L2 projection of amp * delta(x - x_r) onto the element.
//
// One thread per (cell with points, node, component): v = sum_r fma(amp[r][q], psi[r][a], v) from zero over the cell's points
// in the order listed, then field = field + v in double (FP32 blocks convert, add and round once).  The host groups the
// points by cell, so a word has one writer and the order of the sum is fixed: the bits depend only on the field contents, the
// amplitudes and the points - the same under graph replay and eager launches, for one sg_step(n) and n calls of sg_step(1),
// for host-driven stages, and on a split block.  A step beyond the series costs one launch whose threads exit at once.
// No atomics, no LDS.
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace sg {
namespace inject {

template <typename T>
__global__ __launch_bounds__(256) void point_add(T* __restrict__ u, T* __restrict__ s, Args A) {
  const int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t per_group = (int64_t)A.nd * A.ncomp;
  if (idx >= A.ngroups * per_group) return;
  const int64_t step = A.ctr != nullptr ? *A.ctr + 1 : A.step;
  if (step < 1 || step > A.nsteps) return;
  const int64_t g = idx / per_group;
  const int rem = (int)(idx - g * per_group);
  const int a = rem / A.ncomp, q = rem - a * A.ncomp;
  T* f = u;
  int c = q, nc = A.dim;
  if (q >= A.nu) {
    f = s;
    c = q - A.nu;
    nc = A.dim * A.dim;
    // symmetric-stress storage holds the i <= j lines only (the table is symmetric to the bit: the host has checked)
    if (A.sym && c / A.dim > c % A.dim) return;
  }
  const int64_t r0 = A.start[g], r1 = A.start[g + 1];
  const int64_t off = ((A.item[g] * A.nd + a) * nc + c) * A.gw + A.lane[g];
  const double* amp = A.amp + ((step - 1) * A.nown + r0) * A.ncomp + q;
  const double* psi = A.psi + r0 * A.nd + a;
  double v = 0.0;
  for (int64_t r = 0; r < r1 - r0; ++r) v = fma(amp[r * A.ncomp], psi[r * A.nd], v);
  f[off] = (T)((double)f[off] + v);
}

}  // namespace inject

int launch_inject(void* u, void* s, const inject::Args& a, int f32, void* stream) {
  const int64_t total = a.ngroups * a.nd * a.ncomp;
  if (total <= 0) return 0;
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  if (f32)
    hipLaunchKernelGGL(inject::point_add<float>, grid, block, 0, (hipStream_t)stream, (float*)u, (float*)s, a);
  else
    hipLaunchKernelGGL(inject::point_add<double>, grid, block, 0, (hipStream_t)stream, (double*)u, (double*)s, a);
  return (int)hipGetLastError();
}

}  // namespace sg
