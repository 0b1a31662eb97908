// The monitor's sample on the device (include/seigen_hip.h sg_measure / sg_set_monitor): the L2 norms of the velocity and the
// stress and the elastic energy of a block, taken inside the time loop without downloading a field - the global observer
// beside the point-wise one of kernels_recv.hip.
//
// Per cell c three quadratic forms in the reference mass matrix Mhat:
//   Qu = sum_i u_i^T Mhat u_i,   Qs = sum_ij s_ij^T Mhat s_ij,   Qt = t^T Mhat t with t = sum_i s_ii node by node,
// a form v^T Mhat v evaluated as sum_a v_a (Mhat_aa v_a + 2 sum_{b<a} Mhat_ab v_b): b ascending inside a, a ascending, every
// step an fma, all in double (FP32 blocks convert every nodal value first).  In symmetric-stress storage only the i <= j
// lines are read and an off-diagonal form counts twice.  A sample is { U2, S2, T2, EK, ES } = the sums over the block's
// cells of |det J| { Qu, Qs, Qt, wk Qu, ws Qs + wt Qt }; cells of the layout's padding contribute nothing (their lanes are
// read - they lie inside the allocation - and discarded).
//
// Two passes, no floating-point atomics:
//   pass 1  streams u and s once.  One lane owns one cell of an item (hostlogic.hpp Layout), so a (node, component) access
//           of the gw lanes of an item is a whole line of the interleaved layouts.  One WAVE owns one chunk of
//           SG_MONITOR_CHUNK_ITEMS consecutive items by item index - whatever the grid - and writes one partial (five
//           doubles): the five values of a lane are reduced over the lanes of its item by a fixed xor tree, then the items
//           of the chunk are added in ascending order.  Mhat's lower triangle (row a: b = 0 .. a) is the same for every
//           lane: it is read through the scalar cache and enters the FMAs as scalar operands.  The fields are read with
//           non-temporal loads, the next component's ahead of the arithmetic of the current one.
//             pass1_reg  gw = 16, ND = 20 / 35 (the 3-D matrix-pipe layout at P3 / P4): one component's nodal values of the
//                        cell in registers, the next one's in flight in a second set.
//             pass1_lds  every other layout (gw = 1, 16, 64; nd up to 125): the values staged in LDS, one column per lane -
//                        a lane reads back only what it wrote, so no barrier - and as many items of the chunk at a time as
//                        64 KB hold (Args::ips).
//   pass 2  one workgroup: thread t adds the partials t, t + 256, ... in ascending order, a fixed LDS tree follows, thread 0
//           writes the sample.
// On a step that is not a sample step both passes exit at once; the step comes from the argument or, under graph replay,
// from a device word (the role of RecvArgs::ctr).  The bits of a sample depend only on the block and the field contents.
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace sg {
namespace measure {

typedef __attribute__((address_space(4))) const double cdouble;

// the sample this launch takes: false where the step is none
__device__ __forceinline__ bool sample_index(const Args& A, int64_t& j) {
  const int64_t step = A.ctr != nullptr ? *A.ctr + 1 : A.step;
  if (step <= 0 || step % A.every != 0) return false;
  j = step / A.every - 1;
  return j < A.capacity;
}

// the five weighted values of a lane's cell
__device__ __forceinline__ void weigh(const Args& A, bool active, int64_t cell, double Qu, double Qs, double Qt, double v[5]) {
  double wk = A.w0[0], ws = A.w0[1], wt = A.w0[2];
  if (A.w != nullptr && active) {
    wk = A.w[cell * 3 + 0];
    ws = A.w[cell * 3 + 1];
    wt = A.w[cell * 3 + 2];
  }
  v[0] = active ? A.detj * Qu : 0.0;
  v[1] = active ? A.detj * Qs : 0.0;
  v[2] = active ? A.detj * Qt : 0.0;
  v[3] = active ? A.detj * (wk * Qu) : 0.0;
  v[4] = active ? A.detj * fma(ws, Qs, wt * Qt) : 0.0;
}

// over the gw lanes of every item of the sweep (xor tree, widest first), then the sweep's `ips` items in ascending order
// onto the chunk's running sums - the same in every lane
__device__ __forceinline__ void reduce_items(int gw, int ips, double v[5], double tot[5]) {
  for (int off = gw >> 1; off > 0; off >>= 1)
#pragma unroll
    for (int q = 0; q < 5; ++q) v[q] += __shfl_xor(v[q], off);
  for (int i = 0; i < ips; ++i)
#pragma unroll
    for (int q = 0; q < 5; ++q) tot[q] += __shfl(v[q], i * gw);
}

// v^T Mhat v of the ND values in registers.  Mhat's rows arrive as a stream of MCH values at a time: the next MCH are
// requested, then the current ones enter the FMAs - two sets of scalar registers.  (Left to itself the compiler requests
// all nd (nd + 1) / 2 values ahead, keeps them across the components and spills a thousand scalar registers.)
constexpr int MCH = 16;
template <int ND>
__device__ __forceinline__ double quad_reg(const cdouble* M, const double (&v)[ND]) {
  constexpr int NM = ND * (ND + 1) / 2;
  asm volatile("" : "+s"(M));      // not loop-invariant: read again for every form
  double mb[2][MCH];
#pragma unroll
  for (int i = 0; i < MCH; ++i) mb[0][i] = M[i < NM ? i : NM - 1];
  double acc = 0.0;
  int m = 0;
#pragma unroll
  for (int a = 0; a < ND; ++a) {
    double t = 0.0;
#pragma unroll
    for (int b = 0; b <= a; ++b, ++m) {
      if (m % MCH == 0) {
        // the FMAs so far are complete here, and the requests below depend on it (sched_barrier orders the machine
        // scheduler only)
        asm volatile("" : "+v"(t), "+v"(acc), "+s"(M));
        if (m + MCH < NM) {
#pragma unroll
          for (int i = 0; i < MCH; ++i) mb[(m / MCH + 1) & 1][i] = M[m + MCH + i < NM ? m + MCH + i : NM - 1];
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      const double mv = mb[(m / MCH) & 1][m % MCH];
      if (b < a)
        t = fma(mv, v[b], t);
      else
        acc = fma(v[a], fma(mv, v[a], 2.0 * t), acc);
    }
  }
  return acc;
}

template <typename T, int ND>
__global__ __launch_bounds__(256) void pass1_reg(const T* __restrict__ u, const T* __restrict__ s, Args A) {
  int64_t j;
  if (!sample_index(A, j)) return;
  const int lane = threadIdx.x & 63;
  const int64_t chunk = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (chunk >= A.nchunks) return;
  const cdouble* M = (const cdouble*)(unsigned long long)A.Mtri;
  const int64_t item = chunk * SG_MONITOR_CHUNK_ITEMS + (lane >> 4);
  const int64_t itc = item < A.nitems ? item : A.nitems - 1;     // (a lane beyond the last item reads the last and is discarded)
  const int64_t g = itc / A.ncls, cube = g * 16 + (lane & 15);
  const bool active = item < A.nitems && cube < A.ncube;
  const int nu = A.dim, nsc = A.dim * A.dim;
  // a wave-uniform base per (node, component) and one 32-bit offset per lane and field: no address registers per load
  const T* bu = u + chunk * SG_MONITOR_CHUNK_ITEMS * ND * nu * 16;
  const T* bs = s + chunk * SG_MONITOR_CHUNK_ITEMS * ND * nsc * 16;
  const unsigned li = (unsigned)(itc - chunk * SG_MONITOR_CHUNK_ITEMS);
  const unsigned lo_u = (li * ND * nu * 16 + (lane & 15)) * (unsigned)sizeof(T);      // bytes
  const unsigned lo_s = (li * ND * nsc * 16 + (lane & 15)) * (unsigned)sizeof(T);

  double va[ND], vb[ND], tr[ND];
#pragma unroll
  for (int a = 0; a < ND; ++a) tr[a] = 0.0;
  double Qu = 0.0, Qs = 0.0;
  const int n = A.ncomp;
  auto load = [&](double (&v)[ND], int k) {
    const T* b = k < nu ? bu + A.comp[k] * 16 : bs + A.comp[k] * 16;
    const unsigned lo = k < nu ? lo_u : lo_s;
    const int stride = (k < nu ? nu : nsc) * 16;
#pragma unroll
    for (int a = 0; a < ND; ++a) {
      // (the node's base kept apart from the lane's byte offset: scalar base + 32-bit vector offset, no address registers)
      unsigned long long ba = (unsigned long long)(b + a * stride);
      asm volatile("" : "+s"(ba));
      typedef __attribute__((address_space(1))) const char gchar;
      typedef __attribute__((address_space(1))) const T gT;
      v[a] = (double)__builtin_nontemporal_load((gT*)((gchar*)ba + lo));
    }
  };
  auto consume = [&](const double (&v)[ND], int k) {
    const double q = quad_reg<ND>(M, v);
    if (k < nu) {
      Qu += q;
    } else {
      Qs += A.mult[k] * q;
      if (A.diag[k])
#pragma unroll
        for (int a = 0; a < ND; ++a) tr[a] += v[a];
    }
  };
  load(va, 0);
  for (int k = 0; k < n; k += 2) {
    if (k + 1 < n) load(vb, k + 1);
    consume(va, k);
    if (k + 1 < n) {
      if (k + 2 < n) load(va, k + 2);
      consume(vb, k + 1);
    }
  }
  const double Qt = quad_reg<ND>(M, tr);

  double v[5], tot[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  weigh(A, active, cube * A.ncls + (itc - g * A.ncls), Qu, Qs, Qt, v);
  reduce_items(16, SG_MONITOR_CHUNK_ITEMS, v, tot);
  if (lane == 0)
#pragma unroll
    for (int q = 0; q < 5; ++q) A.partial[chunk * 5 + q] = tot[q];
}

// v^T Mhat v of the nd values of this lane's column of `col` (stride ls)
__device__ __forceinline__ double quad_lds(const cdouble* M, const double* col, int nd, int ls) {
  double acc = 0.0;
  int m = 0;
  for (int a = 0; a < nd; ++a) {
    double t = 0.0;
    for (int b = 0; b < a; ++b) t = fma(M[m + b], col[b * ls], t);
    const double va = col[a * ls];
    acc = fma(va, fma(M[m + a], va, 2.0 * t), acc);
    m += a + 1;
  }
  return acc;
}

constexpr int PF = 8;   // nodal values of the next component requested ahead of the current one's arithmetic (pass1_lds)

template <typename T>
__global__ __launch_bounds__(64) void pass1_lds(const T* __restrict__ u, const T* __restrict__ s, Args A) {
  extern __shared__ double lds[];   // [2][nd][ls]: the component at hand, the trace t
  int64_t j;
  if (!sample_index(A, j)) return;
  const int lane = threadIdx.x;
  const int64_t chunk = blockIdx.x;
  const cdouble* M = (const cdouble*)(unsigned long long)A.Mtri;
  const int nd = A.nd, gw = A.gw, ips = A.ips, ls = ips * gw;
  const int nu = A.dim, nsc = A.dim * A.dim, n = A.ncomp;
  const bool lane_used = lane < ls;
  const int lc = lane_used ? lane : 0;         // (an unused lane works on lane 0's cell and is discarded)
  double* col = lds + lc;
  double* trc = lds + (size_t)nd * ls + lc;
  double tot[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int sweep = 0; sweep < SG_MONITOR_CHUNK_ITEMS / ips; ++sweep) {
    const int64_t item = chunk * SG_MONITOR_CHUNK_ITEMS + sweep * ips + lc / gw;
    const int64_t itc = item < A.nitems ? item : A.nitems - 1;
    const int64_t g = itc / A.ncls, cube = g * gw + lc % gw;
    const bool active = lane_used && item < A.nitems && cube < A.ncube;
    const T* pu = u + itc * nd * nu * gw + lc % gw;
    const T* ps = s + itc * nd * nsc * gw + lc % gw;
    auto src = [&](int k, int64_t& stride) {
      stride = (int64_t)(k < nu ? nu : nsc) * gw;
      return k < nu ? pu + A.comp[k] * gw : ps + A.comp[k] * gw;
    };
    if (lane_used)
      for (int a = 0; a < nd; ++a) trc[a * ls] = 0.0;
    double Qu = 0.0, Qs = 0.0;
    const int npf = nd < PF ? nd : PF;
    T pf[PF];
    {
      int64_t stride;
      const T* p = src(0, stride);
#pragma unroll
      for (int a = 0; a < PF; ++a)
        if (a < npf) pf[a] = __builtin_nontemporal_load(p + a * stride);
    }
    for (int k = 0; k < n; ++k) {
      int64_t stride;
      const T* p = src(k, stride);
      // the rest of this component, behind its first values that are already in flight
      if (lane_used) {
#pragma unroll
        for (int a = 0; a < PF; ++a)
          if (a < npf) col[a * ls] = (double)pf[a];
        for (int a = npf; a < nd; ++a) col[a * ls] = (double)__builtin_nontemporal_load(p + a * stride);
      }
      if (k + 1 < n) {
        int64_t stride1;
        const T* p1 = src(k + 1, stride1);
#pragma unroll
        for (int a = 0; a < PF; ++a)
          if (a < npf) pf[a] = __builtin_nontemporal_load(p1 + a * stride1);
      }
      const double q = quad_lds(M, col, nd, ls);
      if (k < nu) {
        Qu += q;
      } else {
        Qs += A.mult[k] * q;
        if (A.diag[k] && lane_used)
          for (int a = 0; a < nd; ++a) trc[a * ls] += col[a * ls];
      }
    }
    const double Qt = quad_lds(M, trc, nd, ls);
    double v[5];
    weigh(A, active, cube * A.ncls + (itc - g * A.ncls), Qu, Qs, Qt, v);
    reduce_items(gw, ips, v, tot);
  }
  if (lane == 0)
#pragma unroll
    for (int q = 0; q < 5; ++q) A.partial[chunk * 5 + q] = tot[q];
}

__global__ __launch_bounds__(256) void pass2(Args A) {
  __shared__ double sh[5][256];
  int64_t j;
  if (!sample_index(A, j)) return;
  const int t = threadIdx.x;
  double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t p = t; p < A.nchunks; p += 256)
#pragma unroll
    for (int q = 0; q < 5; ++q) acc[q] += A.partial[p * 5 + q];
#pragma unroll
  for (int q = 0; q < 5; ++q) sh[q][t] = acc[q];
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w)
#pragma unroll
      for (int q = 0; q < 5; ++q) sh[q][t] += sh[q][t + w];
    __syncthreads();
  }
  if (t == 0)
#pragma unroll
    for (int q = 0; q < 5; ++q) A.out[j * 5 + q] = sh[q][0];
}

}  // namespace measure

size_t measure_lds_bytes(int nd, int gw, int ips) { return (size_t)2 * nd * ips * gw * sizeof(double); }

int measure_items_per_sweep(int nd, int gw) {
  int ips = gw >= 64 ? 1 : SG_MONITOR_CHUNK_ITEMS;
  while (ips > 1 && measure_lds_bytes(nd, gw, ips) > 65536) ips >>= 1;
  return measure_lds_bytes(nd, gw, ips) <= 65536 ? ips : 0;
}

int prepare_measure(int nd, int gw, int ips, int f32) {
  if (ips <= 0) return -1;
  const void* k = f32 ? (const void*)measure::pass1_lds<float> : (const void*)measure::pass1_lds<double>;
  return hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)measure_lds_bytes(nd, gw, ips)) == hipSuccess ? 0 : -1;
}

int launch_measure(const void* u, const void* s, const measure::Args& a, int f32, void* stream) {
  using namespace measure;
  if (a.nchunks <= 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const bool reg = a.gw == 16 && a.dim == 3 && (a.nd == 20 || a.nd == 35);
  if (reg) {
    const dim3 grid((unsigned)((a.nchunks + 3) / 4)), block(256);
    if (a.nd == 20 && !f32) hipLaunchKernelGGL((pass1_reg<double, 20>), grid, block, 0, st, (const double*)u, (const double*)s, a);
    if (a.nd == 20 && f32) hipLaunchKernelGGL((pass1_reg<float, 20>), grid, block, 0, st, (const float*)u, (const float*)s, a);
    if (a.nd == 35 && !f32) hipLaunchKernelGGL((pass1_reg<double, 35>), grid, block, 0, st, (const double*)u, (const double*)s, a);
    if (a.nd == 35 && f32) hipLaunchKernelGGL((pass1_reg<float, 35>), grid, block, 0, st, (const float*)u, (const float*)s, a);
  } else {
    if (a.ips <= 0 || a.ips * a.gw > 64) return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)a.nchunks), block(64);
    const size_t lds = measure_lds_bytes(a.nd, a.gw, a.ips);
    if (f32)
      hipLaunchKernelGGL(pass1_lds<float>, grid, block, lds, st, (const float*)u, (const float*)s, a);
    else
      hipLaunchKernelGGL(pass1_lds<double>, grid, block, lds, st, (const double*)u, (const double*)s, a);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(pass2, dim3(1), dim3(256), 0, st, a);
  return (int)hipGetLastError();
}

}  // namespace sg
