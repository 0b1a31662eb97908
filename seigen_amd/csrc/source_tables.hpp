// What sg_set_source, sg_set_source_separable and sg_set_source_box_ricker derive from the caller's arrays - plain C++,
// no device, no HIP header: built by `make host-asan` too and walked by tools/host_asan_driver.cpp.
//
// A plan is everything the setter uploads, computed from the request and the caller's arrays alone: api.cpp asks for it,
// uploads it into locals and moves those into the handle, so that index arithmetic over caller-supplied arrays runs where
// the CPU sanitizers can see it.
#pragma once
#include <cstdint>
#include <vector>

#include "hostlogic.hpp"

namespace sg {

struct SourceRequest {
  int dim = 0;
  Layout L;                  // the layout of the block's fields
  int64_t ncells = 0, ncube_pad = 0;
  int32_t n[3] = {1, 1, 1};
  std::vector<Box> first;    // the boxes of SG_REGION_FIRST
  bool want_fused = false;   // the family's G stage kernels add the source themselves (and no SEIGEN_HIP_SOURCE_LAUNCH)
  bool sym = false;          // the handle is in the symmetric-stress mode: the plan says whether the values allow it
};

struct SourcePlan {
  int64_t nnz = 0;              // nodes after merging (0: no source)
  int64_t nfirst = 0;           // ... of which the first nfirst lie in cells of SG_REGION_FIRST
  std::vector<int64_t> offs;    // [nnz] device offset of component 0 of each node in the field layout
  std::vector<double> vals;     // [nslices][nnz][dim * dim], nslices = 1 with weights, else nsteps
  std::vector<double> weights;  // [nsteps], or empty
  int64_t nsteps = 0;
  bool is_static = false;       // one time slice that holds at every step (nsteps = -1 on entry, 1 here)
  std::vector<int32_t> slot;    // fused table: [item] -> slot or -1; empty where not wanted or not buildable
  std::vector<int32_t> idx;     // [slot][nd][gw] -> index into offs / vals rows, or -1
  bool symmetric = true;        // (rq.sym) every value block equals its transpose
};

// nsteps slices of values[nslices][nnz][dim * dim] (-1: one that holds at every step), or - weights given - one slice
// scaled by weights[k] at step k < nsteps.  nnz = 0 or nsteps = 0: the empty plan.  Throws std::invalid_argument on a
// null array, nsteps < -1 or a node outside the block.
SourcePlan plan_source(const SourceRequest& rq, int64_t nnz, const int64_t* nodes, int64_t nsteps, const double* values,
                       const double* weights);

// sg_set_source_box_ricker: the nodes of the block inside the closed box [lo, hi], in the host numbering, ascending;
// throws std::invalid_argument unless lo <= hi on every axis
std::vector<int64_t> box_nodes(const NodeGeom& G, const double* lo, const double* hi);
// ... and the Ricker wavelet (-1 + 2 a q) exp(-a q), q = (t - t0)^2, at t = t_first + k dt_step, k < nsteps
std::vector<double> ricker_weights(double a, double t0, double t_first, double dt_step, int64_t nsteps);

}  // namespace sg
