// Device-to-device field transfers (include/seigen_hip.h sg_get_field_dev / sg_set_field_dev / sg_get_spectrum_dev): cells
// cell0 .. cell0 + ncells - 1 between a buffer in the layout of the fields and the caller's device buffer in the host layout
// [cell][node][comp].
//
// For one item (cube group, class) the device side is one contiguous block [row = node * ncomp + comp][lane < gw], the
// caller's side gw runs of rows = nd * ncomp contiguous words, one per cube, ncls * rows words apart: a [rows][gw] <->
// [gw][rows] transpose per item.  A workgroup of four waves takes a UNIT - a slice of rows_per_slice rows of an item - through
// an LDS image [row][pitch = gw + 1] in the block's word type:
//   device side   thread t moves (row t >> log2 gw, lane t & (gw - 1)): consecutive threads are consecutive words - whole
//                 128-byte lines of doubles for gw = 16, 512 bytes for gw = 64;
//   caller's side a wave takes one cube's run at a time, 64 consecutive rows per pass: consecutive threads are consecutive
//                 words there too (the flat layout kernel of the host transfers, kernels.hip layout_kernel, is contiguous on
//                 the staging side only: on the field side its threads are gw words apart).
// In the image a row-fastest walk has the odd stride gw + 1 words and a lane-fastest walk stride 1: neither has a bank conflict.
// Where a slice ends is the plan's decision (hostlogic.hpp xfer_plan), as are the items, the grid and the LDS bytes; the grid
// strides over the units.  All index arithmetic is 64-bit.
//
// A lane whose cell lies outside the range - the cubes before cell0's and behind the last cell's, the classes of the first
// and last cube outside it, the padding lanes of the last group - is neither read nor written on either side.
// Symmetric storage: a download takes row (i, j), i > j, from device row (j, i); the lane index stays the contiguous one.
// An upload compares every (i, j), i < j, word of the caller's with its (j, i) and reports a difference through *flag (the
// caller's values, before any rounding: layout_kernel's test), and writes all lines.
// Conversions are one C++ cast: (float)v rounds once, (double)f is exact.
//
// gw = 1 (generic family): the layouts coincide; equal types are a hipMemcpyAsync of the host code, the others the flat pass.
// The stores are plain ones: non-temporal stores have not been compared for these kernels.
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace sg {
namespace xfer {

// row (node, i * dim + j) with i > j -> row (node, j * dim + i)
__device__ __forceinline__ int mirror_row(int row, int ncomp, int dim) {
  const int c = row % ncomp, i = c / dim, j = c % dim;
  return i > j ? row - c + j * dim + i : row;
}

// F: the block's word type, C: the caller's.  DIR = 0: buf -> field, 1: field -> buf.
template <typename F, typename C, int DIR>
__global__ __launch_bounds__(256) void tiled(F* __restrict__ field, C* __restrict__ buf, int* flag, int64_t item0, int64_t units,
                                             int slices, int rows_per_slice, int rows, int ncomp, int dim, int sym, int gw_shift,
                                             int ncls, int64_t cell0, int64_t ncells, int pitch) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  F* img = reinterpret_cast<F*>(lds_raw);
  const int gw = 1 << gw_shift;
  const int tid = threadIdx.x, wave = tid >> 6, wl = tid & 63;
  for (int64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
    const int64_t item = item0 + unit / slices;
    const int r0 = (int)(unit % slices) * rows_per_slice;
    const int nr = min(rows_per_slice, rows - r0);
    const int64_t group = item / ncls;
    const int cls = (int)(item % ncls);
    // the cell of lane w is ((group << gw_shift) + w) * ncls + cls; in the range for rel = cell - cell0 in 0 .. ncells - 1
    const int64_t rel0 = (group << gw_shift) * ncls + cls - cell0;
    F* const dev0 = field + item * rows * gw;   // row 0 of the item
    F* const dev = dev0 + (int64_t)r0 * gw;     // ... and the slice's first
    if (DIR == 1) {
      for (int t = tid; t < nr << gw_shift; t += 256) {
        const int r = t >> gw_shift, w = t & (gw - 1);
        const int64_t rel = rel0 + (int64_t)w * ncls;
        if (rel < 0 || rel >= ncells) continue;
        const int rr = sym ? mirror_row(r0 + r, ncomp, dim) : r0 + r;
        img[r * pitch + w] = dev0[(int64_t)rr * gw + w];
      }
      __syncthreads();
      for (int w = wave; w < gw; w += 4) {
        const int64_t rel = rel0 + (int64_t)w * ncls;
        if (rel < 0 || rel >= ncells) continue;
        C* const run = buf + rel * rows + r0;
        for (int r = wl; r < nr; r += 64) run[r] = (C)img[r * pitch + w];
      }
    } else {
      for (int w = wave; w < gw; w += 4) {
        const int64_t rel = rel0 + (int64_t)w * ncls;
        if (rel < 0 || rel >= ncells) continue;
        const C* const run = buf + rel * rows + r0;
        for (int r = wl; r < nr; r += 64) {
          const C v = run[r];
          img[r * pitch + w] = (F)v;
          if (flag != nullptr) {   // a stress into symmetric storage: report any asymmetry
            const int c = (r0 + r) % ncomp, i = c / dim, j = c % dim;
            if (i < j && run[r - c + j * dim + i] != v) *flag = 1;
          }
        }
      }
      __syncthreads();
      for (int t = tid; t < nr << gw_shift; t += 256) {
        const int r = t >> gw_shift, w = t & (gw - 1);
        const int64_t rel = rel0 + (int64_t)w * ncls;
        if (rel < 0 || rel >= ncells) continue;
        dev[t] = img[r * pitch + w];
      }
    }
    __syncthreads();   // the image is free for the next unit
  }
}

// gw = 1: word k of the range on both sides, converted; unit = a chunk of 256 words
template <typename F, typename C, int DIR>
__global__ __launch_bounds__(256) void flat(F* __restrict__ field, C* __restrict__ buf, int64_t n, int64_t units) {
  for (int64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
    const int64_t k = unit * 256 + threadIdx.x;
    if (k >= n) continue;
    if (DIR == 1) buf[k] = (C)field[k];
    else field[k] = (F)buf[k];
  }
}

}  // namespace xfer

int launch_xfer(int gw, int ncls, int nd, int ncomp, int dim, int dir, void* field, void* buf, int64_t cell0, int64_t ncells,
                int sym, int* flag, int f32, int c32, int64_t item0, int64_t units, int slices, int rows_per_slice, int pitch,
                int grid, size_t lds_bytes, void* stream) {
  if (ncells <= 0 || units <= 0 || grid <= 0) return 0;
  const int rows = nd * ncomp;
  const dim3 g((unsigned)grid), block(256);
  if (gw == 1) {
    const int64_t n = ncells * rows;
#define SG_XFER_FLAT(FT, CT, D)                                                                                         \
  hipLaunchKernelGGL((xfer::flat<FT, CT, D>), g, block, 0, (hipStream_t)stream, (FT*)field + cell0 * rows, (CT*)buf, n, units)
    // (the generic family has double blocks only, and equal types are the host code's hipMemcpyAsync)
    if (f32 || !c32) return -1;
    if (dir == 0) SG_XFER_FLAT(double, float, 0);
    else SG_XFER_FLAT(double, float, 1);
#undef SG_XFER_FLAT
    return (int)hipGetLastError();
  }
  const int gw_shift = gw == 16 ? 4 : 6;
  if (gw != 1 << gw_shift) return -1;
  // the mirror and the symmetry test belong to a tensor: ncomp = dim^2
  if (ncomp != dim * dim) {
    sym = 0;
    flag = nullptr;
  }
#define SG_XFER_TILED(FT, CT, D)                                                                                               \
  hipLaunchKernelGGL((xfer::tiled<FT, CT, D>), g, block, lds_bytes, (hipStream_t)stream, (FT*)field, (CT*)buf, flag, item0, units, \
                     slices, rows_per_slice, rows, ncomp, dim, sym, gw_shift, ncls, cell0, ncells, pitch)
  if (dir == 0) {
    if (f32 && c32) SG_XFER_TILED(float, float, 0);
    else if (f32) SG_XFER_TILED(float, double, 0);
    else if (c32) SG_XFER_TILED(double, float, 0);
    else SG_XFER_TILED(double, double, 0);
  } else {
    if (f32 && c32) SG_XFER_TILED(float, float, 1);
    else if (f32) SG_XFER_TILED(float, double, 1);
    else if (c32) SG_XFER_TILED(double, float, 1);
    else SG_XFER_TILED(double, double, 1);
  }
#undef SG_XFER_TILED
  return (int)hipGetLastError();
}

}  // namespace sg
