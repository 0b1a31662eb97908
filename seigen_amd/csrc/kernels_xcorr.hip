// The per-cell correlation of two handles' fields on the device (include/seigen_hip.h sg_correlate): the observer between
// the point-wise one of kernels_recv.hip and the block-wide one of kernels_measure.hip.
//
// Per cell c three bilinear forms in the reference mass matrix Mhat, of handle a's fields against handle b's:
//   Buu = sum_i a.u_i^T Mhat b.u_i,   Bss = sum_ij a.s_ij^T Mhat b.s_ij,   Btt = t_a^T Mhat t_b with t_x = sum_i x.s_ii node by node,
// a form x^T Mhat y evaluated as sum_alpha x_alpha r_alpha with r = Mhat y, r_alpha summed over beta ascending, all in double
// (FP32 blocks convert every nodal value first).  Components in the order of hostlogic.hpp xcorr_components: the velocity's,
// then the stress's row-major; each handle reads (i, j) from the line its own storage holds.  Then
//   acc[c][k] = fma(wd[k], B_k, acc[c][k]),   wd[k] = w[k] |det J|,   k = uu, ss, tt
// by one lane per cell: no sum across cells, no atomics; the bits of a cell's result depend only on that cell's nodal values,
// the weights, the dtype and the kernel form.  One lane owns one cell of an item (hostlogic.hpp Layout), so a (node, component)
// access of the gw lanes of an item is a whole line of the interleaved layouts.  The fields are read with non-temporal loads,
// the next component's ahead of the arithmetic of the current one.
//
//   xcorr_mfma  gw = 16, ND = 20 / 35 (the 3-D matrix-pipe layout at P3 / P4).  One wave owns the 16 cells of an item; lane
//               (cell, q) = (lane & 15, lane >> 4).  Per component b's nodal lines are loaded as B operands of
//               v_mfma_f64_16x16x4_f64 - k-step ks: lane (cell, q) holds node 4 ks + q, one full line per lane group, no LDS -
//               and r = Mhat b is that product with Mhat's 16 x 4 tiles as A operands, zero-padded (ND = 35: 3 row tiles x 9
//               k-steps), staged once per block in LDS as [tile][lane] and read back with one conflict-free ds_read per
//               product: in registers the 27 tiles take 54 VGPRs and the second wave per SIMD with them.  A persistent
//               grid, every wave striding over the items.  k-steps ascending; the three row tiles are independent
//               accumulators.  The f64 accumulator of row tile rt leaves lane (cell, q) with rows 16 rt + 4 reg + q, reg = 0..3:
//               node 4 ks' + q of k-step ks' = 4 rt + reg - so a is loaded in the very same fragment form, and a . r is a
//               per-lane fma chain in ascending (rt, reg), from zero for every component.  The chains of the components are
//               added per lane (Bss: fma(mult, chain, Bss)); the traces are summed per lane from the diagonal components and
//               take one more product; at the end the four lane groups of a cell are folded by xor 32, then xor 16.  Lanes
//               of padding cells are read (they lie inside the allocation) and discarded; a node beyond ND reads node ND - 1
//               and enters as zero.
//   xcorr_lds   every other layout (gw = 1, 16, 64; nd up to 125): four column sets staged in LDS - a's component, b's
//               component, t_a, t_b - one column per lane; a lane reads back only what it wrote, so no barrier.  Mhat is the
//               full matrix, read through the scalar cache and entering the FMAs as scalar operands.  A workgroup of 64 lanes
//               holds as many items as 64 KB take (Args::ipw).  Lanes of padding cells leave at once.
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace sg {
namespace xcorr {

typedef __attribute__((address_space(4))) const double cdouble;
typedef double v4 __attribute__((ext_vector_type(4)));

template <typename T, int ND>
__global__ __launch_bounds__(256, 2) void xcorr_mfma(Args A) {
  constexpr int NKS = (ND + 3) / 4, NRT = (ND + 15) / 16;
  constexpr int NU = 3, NSC = 9;
  const int lane = threadIdx.x & 63, cell = lane & 15, q = lane >> 4;
  const int64_t wave = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
  // Mhat's tiles in LDS, read by every wave of the block as [tile][lane]: conflict-free, one ds_read per product
  __shared__ double mt_lds[NRT * NKS * 64];
  for (int t = threadIdx.x; t < NRT * NKS * 64; t += 256) mt_lds[t] = A.M[t];
  __syncthreads();
  const double* mt = mt_lds + lane;
  // a wave-uniform base per (k-step, component) and one 32-bit byte offset per lane and field: no address registers per load.
  // This lane's node of k-step ks is 4 ks + q; one beyond ND (the last k-step only) reads node ND - 1 and enters as zero
  constexpr int QLAST = ND - 1 - 4 * (NKS - 1);     // the last k-step's last lane group with a node
  const bool last_is_pad = q > QLAST;
  const int ql = last_is_pad ? QLAST : q;
  const unsigned lo_u = (unsigned)(q * NU * 16 + cell) * (unsigned)sizeof(T), lo_s = (unsigned)(q * NSC * 16 + cell) * (unsigned)sizeof(T);
  const unsigned ll_u = (unsigned)(ql * NU * 16 + cell) * (unsigned)sizeof(T), ll_s = (unsigned)(ql * NSC * 16 + cell) * (unsigned)sizeof(T);
  const T* ua = (const T*)A.ua;
  const T* sa = (const T*)A.sa;
  const T* ub = (const T*)A.ub;
  const T* sb = (const T*)A.sb;
  const int n = A.ncomp;
  typedef __attribute__((address_space(1))) const char gchar;
  typedef __attribute__((address_space(1))) const T gT;

  for (int64_t item = wave; item < A.nitems; item += nwaves) {
    const int64_t ou = item * ND * NU * 16, os = item * ND * NSC * 16;
    auto load = [&](double (&fa)[NKS], double (&fb)[NKS], int k) {
      const int nc = k < NU ? NU : NSC;
      const T* pa = (k < NU ? ua + ou : sa + os) + A.comp_a[k] * 16;
      const T* pb = (k < NU ? ub + ou : sb + os) + A.comp_b[k] * 16;
      const unsigned lo = k < NU ? lo_u : lo_s, ll = k < NU ? ll_u : ll_s;
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) {
        unsigned long long ba = (unsigned long long)(pa + 4 * ks * nc * 16), bb = (unsigned long long)(pb + 4 * ks * nc * 16);
        asm volatile("" : "+s"(ba), "+s"(bb));
        const unsigned o = (ks == NKS - 1 && 4 * NKS > ND) ? ll : lo;
        fa[ks] = (double)__builtin_nontemporal_load((gT*)((gchar*)ba + o));
        fb[ks] = (double)__builtin_nontemporal_load((gT*)((gchar*)bb + o));
      }
    };
    auto pad = [&](double (&fa)[NKS], double (&fb)[NKS]) {
      if (4 * NKS > ND) {
        fa[NKS - 1] = last_is_pad ? 0.0 : fa[NKS - 1];
        fb[NKS - 1] = last_is_pad ? 0.0 : fb[NKS - 1];
      }
    };
    // x^T Mhat y of this lane's rows: r = Mhat y on the matrix pipe, then the chain over (rt, reg)
    auto form = [&](const double (&fx)[NKS], const double (&fy)[NKS]) {
      v4 r[NRT];
#pragma unroll
      for (int rt = 0; rt < NRT; ++rt) r[rt] = v4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
        for (int rt = 0; rt < NRT; ++rt) r[rt] = __builtin_amdgcn_mfma_f64_16x16x4f64(mt[(rt * NKS + ks) * 64], fy[ks], r[rt], 0, 0, 0);
      double c = 0.0;
#pragma unroll
      for (int rt = 0; rt < NRT; ++rt)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg)
          if (4 * rt + reg < NKS) c = fma(fx[4 * rt + reg], r[rt][reg], c);
      return c;
    };
    double ta[NKS], tb[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) ta[ks] = tb[ks] = 0.0;
    double Buu = 0.0, Bss = 0.0;
    auto consume = [&](double (&fa)[NKS], double (&fb)[NKS], int k) {
      pad(fa, fb);
      const double c = form(fa, fb);
      if (k < NU) {
        Buu += c;
      } else {
        Bss = fma(A.mult[k], c, Bss);
        if (A.diag[k])
#pragma unroll
          for (int ks = 0; ks < NKS; ++ks) {
            ta[ks] += fa[ks];
            tb[ks] += fb[ks];
          }
      }
    };
    double fa0[NKS], fb0[NKS], fa1[NKS], fb1[NKS];
    load(fa0, fb0, 0);
    for (int k = 0; k < n; k += 2) {
      if (k + 1 < n) load(fa1, fb1, k + 1);
      consume(fa0, fb0, k);
      if (k + 1 < n) {
        if (k + 2 < n) load(fa0, fb0, k + 2);
        consume(fa1, fb1, k + 1);
      }
    }
    double Btt = form(ta, tb);
    Buu += __shfl_xor(Buu, 32);
    Bss += __shfl_xor(Bss, 32);
    Btt += __shfl_xor(Btt, 32);
    Buu += __shfl_xor(Buu, 16);
    Bss += __shfl_xor(Bss, 16);
    Btt += __shfl_xor(Btt, 16);
    const int64_t g = item / A.ncls, cube = g * 16 + cell;
    if (q == 0 && cube < A.ncube) {
      double* o = A.acc + (cube * A.ncls + (item - g * A.ncls)) * 3;
      o[0] = fma(A.wd[0], Buu, o[0]);
      o[1] = fma(A.wd[1], Bss, o[1]);
      o[2] = fma(A.wd[2], Btt, o[2]);
    }
  }
}

// x^T Mhat y of the nd values of this lane's columns (stride ls)
__device__ __forceinline__ double form_lds(const cdouble* M, const double* x, const double* y, int nd, int ls) {
  double acc = 0.0;
  for (int a = 0; a < nd; ++a) {
    double r = 0.0;
    for (int b = 0; b < nd; ++b) r = fma(M[a * nd + b], y[b * ls], r);
    acc = fma(x[a * ls], r, acc);
  }
  return acc;
}

constexpr int PF = 8;   // nodal values of the next component, of either handle, requested ahead of the current one's arithmetic

template <typename T>
__global__ __launch_bounds__(64) void xcorr_lds(Args A) {
  extern __shared__ double lds[];   // [4][nd][ls]: a's component, b's component, t_a, t_b
  const int lane = threadIdx.x;
  const int nd = A.nd, gw = A.gw, ls = A.ipw * gw;
  if (lane >= ls) return;
  const int64_t item = (int64_t)blockIdx.x * A.ipw + lane / gw;
  if (item >= A.nitems) return;
  const int64_t g = item / A.ncls, cube = g * gw + lane % gw;
  if (cube >= A.ncube) return;
  const cdouble* M = (const cdouble*)(unsigned long long)A.M;
  double* ca = lds + lane;
  double* cb = ca + (size_t)nd * ls;
  double* ta = cb + (size_t)nd * ls;
  double* tb = ta + (size_t)nd * ls;
  const int nu = A.dim, nsc = A.dim * A.dim, n = A.ncomp;
  const int64_t ou = item * nd * nu * gw + lane % gw, os = item * nd * nsc * gw + lane % gw;
  auto src = [&](int k, const T*& pa, const T*& pb, int64_t& stride) {
    stride = (int64_t)(k < nu ? nu : nsc) * gw;
    pa = (k < nu ? (const T*)A.ua + ou : (const T*)A.sa + os) + A.comp_a[k] * gw;
    pb = (k < nu ? (const T*)A.ub + ou : (const T*)A.sb + os) + A.comp_b[k] * gw;
  };
  for (int a = 0; a < nd; ++a) ta[a * ls] = tb[a * ls] = 0.0;
  double Buu = 0.0, Bss = 0.0;
  const int npf = nd < PF ? nd : PF;
  T pfa[PF], pfb[PF];
  {
    const T *pa, *pb;
    int64_t stride;
    src(0, pa, pb, stride);
#pragma unroll
    for (int a = 0; a < PF; ++a)
      if (a < npf) {
        pfa[a] = __builtin_nontemporal_load(pa + a * stride);
        pfb[a] = __builtin_nontemporal_load(pb + a * stride);
      }
  }
  for (int k = 0; k < n; ++k) {
    const T *pa, *pb;
    int64_t stride;
    src(k, pa, pb, stride);
    // the rest of this component, behind its first values that are already in flight
#pragma unroll
    for (int a = 0; a < PF; ++a)
      if (a < npf) {
        ca[a * ls] = (double)pfa[a];
        cb[a * ls] = (double)pfb[a];
      }
    for (int a = npf; a < nd; ++a) {
      ca[a * ls] = (double)__builtin_nontemporal_load(pa + a * stride);
      cb[a * ls] = (double)__builtin_nontemporal_load(pb + a * stride);
    }
    if (k + 1 < n) {
      const T *pa1, *pb1;
      int64_t stride1;
      src(k + 1, pa1, pb1, stride1);
#pragma unroll
      for (int a = 0; a < PF; ++a)
        if (a < npf) {
          pfa[a] = __builtin_nontemporal_load(pa1 + a * stride1);
          pfb[a] = __builtin_nontemporal_load(pb1 + a * stride1);
        }
    }
    const double c = form_lds(M, ca, cb, nd, ls);
    if (k < nu) {
      Buu += c;
    } else {
      Bss = fma(A.mult[k], c, Bss);
      if (A.diag[k])
        for (int a = 0; a < nd; ++a) {
          ta[a * ls] += ca[a * ls];
          tb[a * ls] += cb[a * ls];
        }
    }
  }
  const double Btt = form_lds(M, ta, tb, nd, ls);
  double* o = A.acc + (cube * A.ncls + (item - g * A.ncls)) * 3;
  o[0] = fma(A.wd[0], Buu, o[0]);
  o[1] = fma(A.wd[1], Bss, o[1]);
  o[2] = fma(A.wd[2], Btt, o[2]);
}

template <typename T, int ND>
static const void* mfma_kernel() { return (const void*)xcorr_mfma<T, ND>; }
static const void* mfma_kernel_of(int nd, int f32) {
  if (nd == 20) return f32 ? mfma_kernel<float, 20>() : mfma_kernel<double, 20>();
  if (nd == 35) return f32 ? mfma_kernel<float, 35>() : mfma_kernel<double, 35>();
  return nullptr;
}

}  // namespace xcorr

size_t xcorr_lds_bytes(int nd, int gw, int ipw) { return (size_t)4 * nd * ipw * gw * sizeof(double); }

int xcorr_items_per_group(int nd, int gw) {
  if (gw < 1 || gw > 64) return 0;
  int ipw = 64 / gw;
  while (ipw > 1 && xcorr_lds_bytes(nd, gw, ipw) > 65536) ipw >>= 1;
  return xcorr_lds_bytes(nd, gw, ipw) <= 65536 ? ipw : 0;
}

int prepare_xcorr(int nd, int gw, int ipw, int mfma, int f32, int ncu) {
  if (mfma) {
    const void* k = xcorr::mfma_kernel_of(nd, f32);
    int per_cu = 0;
    if (!k || hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k, 256, 0) != hipSuccess || per_cu < 1) return -1;
    return per_cu * (ncu > 0 ? ncu : 1);
  }
  if (ipw <= 0) return -1;
  const void* k = f32 ? (const void*)xcorr::xcorr_lds<float> : (const void*)xcorr::xcorr_lds<double>;
  return hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)xcorr_lds_bytes(nd, gw, ipw)) == hipSuccess ? 1 : -1;
}

int launch_xcorr(const xcorr::Args& a, int mfma, int f32, int grid, void* stream) {
  using namespace xcorr;
  if (a.nitems <= 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (mfma) {
    if (!xcorr_has_mfma(a.dim, a.nd, a.gw, 0) || grid < 1) return (int)hipErrorInvalidValue;
    const int64_t want = (a.nitems + 3) / 4;
    const dim3 g((unsigned)(want < grid ? want : grid)), block(256);
    if (a.nd == 20 && !f32) hipLaunchKernelGGL((xcorr_mfma<double, 20>), g, block, 0, st, a);
    if (a.nd == 20 && f32) hipLaunchKernelGGL((xcorr_mfma<float, 20>), g, block, 0, st, a);
    if (a.nd == 35 && !f32) hipLaunchKernelGGL((xcorr_mfma<double, 35>), g, block, 0, st, a);
    if (a.nd == 35 && f32) hipLaunchKernelGGL((xcorr_mfma<float, 35>), g, block, 0, st, a);
  } else {
    if (a.ipw <= 0 || a.ipw * a.gw > 64) return (int)hipErrorInvalidValue;
    const dim3 g((unsigned)((a.nitems + a.ipw - 1) / a.ipw)), block(64);
    const size_t lds = xcorr_lds_bytes(a.nd, a.gw, a.ipw);
    if (f32)
      hipLaunchKernelGGL(xcorr_lds<float>, g, block, lds, st, a);
    else
      hipLaunchKernelGGL(xcorr_lds<double>, g, block, lds, st, a);
  }
  return (int)hipGetLastError();
}

}  // namespace sg
