// The handle behind the C-ABI (include/seigen_hip.h) and what its translation units share:
//   api.cpp      create / destroy, parameters, sponge, source, receivers, injectors, monitor, correlation, spectra: device checks, uploads, the move into the handle
//   transfer.cpp host <-> device field transfers (layout conversion, pinned pipeline)
//   devxfer.cpp  device <-> device field and spectrum transfers into the caller's buffers, queued on the stream
//   frame.cpp    a field rastered on a cube-aligned pixel lattice into the caller's device buffer, queued on the stream
//   grad.cpp     the broken gradient of a velocity field at the nodes into the caller's device buffer, queued on the stream
//   peak.cpp     the peak maps: arming, the end-of-step launches, the read-outs through the host and on the stream
//   gauge.cpp    the gauges: arming, the end-of-step launch, the read-out, the one-shot probe of the gradient at points
//   stages.cpp   regions, stage launches, the LF4 step, graphs, halo packs, timing
// and, without a device or a HIP header (the CPU sanitizer build, `make host-asan`):
//   hostapi.cpp (hostlogic.hpp)  family choice, field layout, stage table, region boxes / items, point location, receiver and injector plans;
//                                what stepping remembers between calls: field write counts, the sponge pre-pass's state,
//                                the source's slice at a step, the clock of the end-of-step hooks (StepClock)
//   sponge_tables.cpp            what sg_set_absorption derives from the nodal sigma
//   source_tables.cpp            what the source setters derive from the caller's nodes and values
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/seigen_hip.h"
#include "hostlogic.hpp"
#include "kernels.hpp"
#include "mesh_tables.hpp"
#include "mfma_tables.hpp"
#include "refelem.hpp"

using namespace sg;

struct sg_comm_state;   // comm.cpp: RCCL communicator, peers and halo buffers of the native exchange

// The one owner of a hipMalloc'ed array: freed by its destructor, moved but never copied.  A setter builds its new
// tables in locals and moves them into the handle only once everything has succeeded, so that a call which fails
// leaves the handle as it was.
template <typename T>
struct DevBuf {
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      reset();
      std::swap(p_, o.p_);
    }
    return *this;
  }
  ~DevBuf() { reset(); }
  T* get() const { return p_; }
  void reset() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
  }
  hipError_t alloc(size_t n) {   // (an empty array still gets an address: 8 bytes)
    reset();
    return hipMalloc((void**)&p_, std::max<size_t>(n * sizeof(T), 8));
  }
  hipError_t upload(const T* src, size_t n) {
    hipError_t e = alloc(n);
    return (e != hipSuccess || n == 0) ? e : hipMemcpy(p_, src, n * sizeof(T), hipMemcpyHostToDevice);
  }

 private:
  T* p_ = nullptr;
};

// What sg_set_absorption derived from the nodal sigma (sponge_tables.cpp plan_sponge), on the device
struct SpongeTables {
  DevBuf<int32_t> slot;    // [cell] -> slot or -1
  DevBuf<double> B;        // [matrix][nd][nd]
  DevBuf<double> sigma;    // 2-D tile and 3-D MFMA kernels only (kernels.hpp StageArgs::sponge_sigma)
  int32_t nslots = 0;      // cells with a sponge matrix of their own
  DevBuf<int32_t> cells;   // [slot] -> cell: the pre-pass of the F stages (kernels.hpp launch_sponge_pre)
  DevBuf<int32_t> mat;     // [slot] -> matrix in B (cells with the same nodal sigma share one)
  DevBuf<char> pre;        // [slot][nd][dim] in the field type
  int pre_lines = 0;       // pre in line layout, slot = item * gw + w (3-D MFMA family), else a record per slot
  // cells whose sigma is affine in the reference coordinates take dim + 1 numbers instead of a matrix (kernels.hpp
  // launch_sponge_pre_affine); the cells that keep a matrix are then a LIST of slots
  int32_t nmat_slots = 0;  // slots with a matrix (all of them where no cell is affine: mat_slots stays empty)
  DevBuf<int32_t> mat_slots;
  int32_t aff_nitems = 0, aff_W = 0;
  DevBuf<int32_t> aff_items;  // [item] -> (cube group) * ncls + class
  DevBuf<int32_t> aff_slots;  // [item][gw] -> slot or -1
  DevBuf<double> aff_coef;    // [slot][dim + 1]
  DevBuf<double> aff_X;       // [dim][nd][W]
  DevBuf<int32_t> aff_col;    // [nd][W], empty where the rows are dense
  DevBuf<double> aff_frag;    // 3-D MFMA family in double: the X_k as row tiles (mfma_frags_dense)
  int aff_grid = 0;           // persistent grid of the affine pre-pass (sponge_affine_mfma where aff_frag is set), on the handle's device; capped by SEIGEN_HIP_GRID_BLOCKS
  PrePass pre_state;          // what `pre` holds and when it is due again (hostlogic.hpp); new tables start with none
};

// The source of sg_set_source / sg_set_source_separable, on the device
struct SourceTables {
  int64_t nnz = 0;
  int64_t nfirst = 0;       // source nodes are stored with those in cells of SG_REGION_FIRST first
  DevBuf<int64_t> nodes;    // device offset of component 0 of each node in the field layout
  DevBuf<double> values;    // [nsteps][nnz][dim*dim]
  int64_t nsteps = 0;
  bool is_static = false;   // one time slice that holds at every step
  std::vector<double> weights;   // separable source: values is one slice, scaled by weights[src_step]
  DevBuf<double> weights_d;
  // 2-D tile path: the source is added inside the G stage kernels (StageArgs::src_slot / src_idx)
  bool fused = false;
  DevBuf<int32_t> slot, idx;
};

// What each of the six end-of-step hooks - receivers, gauges, monitor, spectra, peak maps, injectors (stages.cpp hooks) - keeps besides its
// tables.  ctr serves graph replay: it is the step index of the hook's launches in a capture - they read it (the kernels'
// Args::ctr), a one-thread launch bumps it behind them, and sg_step sets it to clock.steps before it replays: the role of
// sg_handle::src_ctr_d for the source.  A setter puts a zero there when it arms (arm_hook below).
struct StepSeries {
  StepClock clock;            // every, count, steps completed since arming (hostlogic.hpp)
  DevBuf<int64_t> ctr;
};

// The receivers of sg_set_receivers (the points of tests/explosive_source/uy.py:31-43), on the device: the owned ones'
// cells and basis values, and the trace the recorder (kernels_recv.hip) fills at the end of every `every`-th step
struct ReceiverTables : StepSeries {   // clock.count: the capacity of the trace
  int64_t nrec = 0;           // receivers armed (0: none; every block of a mesh is handed all of them)
  int64_t nown = 0;           // ... of which this block owns these, in the order given
  std::vector<int64_t> row;   // [nown] -> receiver index (the row of sg_get_receivers' output)
  DevBuf<int64_t> item;       // [nown] item and
  DevBuf<int32_t> lane;       // [nown] lane of the owning cell in the layout of the fields (hostlogic.hpp Layout)
  DevBuf<double> phi;         // [nown][nd] basis of the cell at the point
  int what = 0;               // bit 0: velocity (dim values), bit 1: stress (dim x dim, row-major)
  int ncomp = 0;
  DevBuf<double> trace;       // [capacity][nown][ncomp]
};

// The gauges of sg_set_gauges (gauge.cpp, kernels_gauge.hip), on the device: the owned points' cells, classes and derivative rows
// (hostlogic.hpp GaugePlan), the block's J, and the trace the kernel fills at the end of every `every`-th step
struct GaugeTables : StepSeries {      // clock.count: the capacity of the trace
  int64_t npts = 0;           // gauges armed (0: none; every block of a mesh is handed all of them)
  int64_t nown = 0;           // ... of which this block owns these, in the order given
  std::vector<int64_t> row;   // [nown] -> point index (the row of sg_get_gauges' output)
  DevBuf<int64_t> item;       // [nown] item and
  DevBuf<int32_t> lane;       // [nown] lane of the owning cell in the layout of the fields (hostlogic.hpp Layout)
  DevBuf<int32_t> cls;        // [nown] its class
  DevBuf<double> D;           // [nown][dim][nd] d(phi_a)/d(xi_r) at the point
  DevBuf<double> J;           // [ncls][3][3] = MeshDev::Jinv
  int kind = 0;               // sg_get_gradient_dev's: 0 gradient, 1 divergence, 2 curl, 3 symmetric strain rate
  int ncomp = 0;
  DevBuf<double> trace;       // [capacity][nown][ncomp]
  // the hook's launch (gauge.cpp queue_gauges), set by the arming call: stages.cpp reaches the feature through the armed tables
  // alone, as it reaches the peak maps
  int (*queue)(sg_handle* h, hipStream_t stream, const int64_t* ctr, int64_t step) = nullptr;
};

// The injectors of sg_set_injectors (and, for the one launch, of sg_inject), on the device: the owned points grouped by cell
// (hostlogic.hpp InjectorPlan), their psi, and the series that the kernel (kernels_inject.hip) adds at the end of the steps
struct InjectTables : StepSeries {   // clock.count: the entries of the series, clock.every = 1
  int64_t npts = 0;           // points armed (0: none; every block of a mesh is handed all of them)
  int64_t nown = 0;           // ... of which this block owns these
  int64_t ngroups = 0;        // cells with points
  DevBuf<int64_t> item;       // [ngroups] item and
  DevBuf<int32_t> lane;       // [ngroups] lane of the cell in the layout of the fields (hostlogic.hpp Layout)
  DevBuf<int64_t> start;      // [ngroups + 1] the group's rows
  DevBuf<double> psi;         // [nown][nd]
  DevBuf<double> amp;         // [nsteps][nown][ncomp]
  int what = 0;               // bit 0: velocity (dim values), bit 1: stress (dim x dim, row-major)
  int ncomp = 0;
};

// The spectra of sg_set_spectra (kernels_spectra.hip), on the device: per selected field the weight table and the accumulators,
// which have the field's own layout (double for FP32 blocks too)
struct SpectraTables : StepSeries {   // clock.count: nsamples
  int nfreq = 0;              // frequencies armed (0: none)
  int what = 0;               // bit 0: velocity, bit 1: stress
  DevBuf<double> w[2];        // [nsamples][nfreq][2] of the velocity / of the stress
  DevBuf<double> acc[2];      // [nfreq][2][field_alloc] of the velocity / of the stress
  bool has(int k) const { return nfreq > 0 && (what & (1 << k)) != 0; }   // k = 0: velocity, 1: stress
};

// The peak maps of sg_set_peaks (kernels_peak.hip), on the device: per selected field the running maximum of the squared
// magnitude and the sample that reached it, in the field's own layout with one component (12 bytes per node and field)
struct PeakTables : StepSeries {      // clock.count: nsamples
  int what = 0;               // bit 0: velocity, bit 1: stress (0: none armed)
  DevBuf<double> val[2];      // [field_alloc / ncomp] of the velocity / of the stress
  DevBuf<int32_t> idx[2];     // ... the 0-based sample of the maximum, -1: never above zero
  // the hook's launches (peak.cpp queue_peaks), set by the arming call: stages.cpp reaches the feature through the armed
  // tables alone, so a program that never arms the maps links without peak.cpp and kernels_peak.hip
  int (*queue)(sg_handle* h, hipStream_t stream, const int64_t* ctr, int64_t step) = nullptr;
  bool has(int k) const { return (what & (1 << k)) != 0; }   // k = 0: velocity, 1: stress
};

// The monitor of sg_set_monitor and the scratch of sg_measure (kernels_measure.hip), on the device
struct MonitorTables : StepSeries {   // clock.count: the capacity of the trace
  bool armed = false;
  DevBuf<double> w;           // [ncells][3] per-cell weights, or empty: w0
  double w0[3] = {0.0, 0.0, 0.0};
  DevBuf<double> trace;       // [capacity][5]
};
// what every sample needs, built by the first sg_measure / sg_set_monitor of the handle and kept
struct MeasureScratch {
  DevBuf<double> Mtri;        // hostlogic.hpp mass_lower_rows
  DevBuf<double> partial;     // [nchunks][5]
  DevBuf<double> out;         // [5]: the sample of sg_measure
  int64_t nitems = 0, nchunks = 0;
  int ips = 0;                // measure::Args::ips
  bool ready = false;
};

// An event of the runtime with one owner, as DevBuf is for arrays
struct DevEvent {
  DevEvent() = default;
  DevEvent(DevEvent&& o) noexcept : e_(o.e_) { o.e_ = nullptr; }
  DevEvent& operator=(DevEvent&& o) noexcept {
    if (this != &o) {
      reset();
      std::swap(e_, o.e_);
    }
    return *this;
  }
  ~DevEvent() { reset(); }
  hipEvent_t get() const { return e_; }
  void reset() {
    if (e_) (void)hipEventDestroy(e_);
    e_ = nullptr;
  }
  hipError_t create() {
    reset();
    return hipEventCreateWithFlags(&e_, hipEventDisableTiming);
  }

 private:
  hipEvent_t e_ = nullptr;
};

// The correlation of sg_correlate (kernels_xcorr.hip): built by the handle's first successful call and kept until
// sg_reset_correlation releases it
struct CorrelationTables {
  DevBuf<double> acc;         // [ncells][3] = (uu, ss, tt) in host cell order
  DevBuf<double> M;           // the operator in the form the kernel takes: hostlogic.hpp xcorr_mass_tiles, or Mhat [nd][nd]
  bool mfma = false;          // the matrix-pipe form (SEIGEN_HIP_XCORR=lds: the LDS-staged one on its layouts too)
  int ipw = 0;                // xcorr::Args::ipw
  int grid = 0;               // persistent grid of the matrix-pipe form
  int grid64 = 0;             // ... of its double instantiation on an FP32 block (sg_correlate_spectra: prepared by its first call)
  int64_t nitems = 0;
  DevEvent ev_in, ev_out;     // the other handle's stream -> the launch -> the other handle's stream
  bool ready = false;
};

// The frames of sg_get_frame_dev (frame.cpp, kernels_frame.hip): the tables of the last frame specification, on the device
struct FrameTables {
  bool ready = false;
  sg_frame key = {};          // the specification (frame.cpp frame_key)
  FramePlan plan;             // ... and its plan (hostlogic.hpp)
  DevBuf<FrameSpec> spec;     // what the specification fixes for every launch (kernels.hpp)
  DevBuf<int32_t> cls;        // [Q] class of in-cube pixel q
  DevBuf<int32_t> order;      // [Q] the pixels sorted by class
  DevBuf<int32_t> cstart;     // [ncls + 1]
  DevBuf<double> phi;         // [Q][nd]
  DevBuf<int32_t> groups;     // the listed groups of gw cubes (hostlogic.hpp FramePlan)
};

// The gradient of sg_get_gradient_dev (grad.cpp, kernels_grad.hip): its tables on the device, built by the handle's first call
struct GradTables {
  bool ready = false;
  DevBuf<double> C;           // simplices: [dim][nd][nd] dense; tensor-product cells: the 1-D matrix [n1][n1]
  DevBuf<double> J;           // [ncls][3][3] = MeshDev::Jinv
  int n1 = 0;                 // P + 1 on tensor-product cells, else 0 (kernels.hpp GradArgs::n1)
};

// The four fields of a block.  Whoever writes one asks for it with write(), which counts the write: what remembers a field
// state (the sponge pre-pass, hostlogic.hpp PrePass) can then tell that the field has moved on - from a stage, a source
// launch, an upload or the mirror launch alike.  Readers take the const pointer.
struct Fields {
  const double* read(int f) const { return buf_[f].get(); }
  double* write(int f) {
    ver_.written(f);
    return buf_[f].get();
  }
  void replayed() { ver_.replayed(); }
  const FieldVersions& versions() const { return ver_; }
  hipError_t alloc(int f, size_t n) { return buf_[f].alloc(n); }

 private:
  DevBuf<double> buf_[4];   // double, or float where f32
  FieldVersions ver_;
};

struct sg_handle {
  sg_config cfg;
  sg_comm_state* comm = nullptr;
  RefElem re;
  MeshDev md;
  DevBuf<MeshDev> md_dev;
  DevBuf<double> Dt, Lt;
  Fields field;
  size_t field_len[4] = {0, 0, 0, 0};    // doubles, host layout (ncells * nd * comps)
  size_t field_alloc[4] = {0, 0, 0, 0};  // values allocated on the device (layout padding included)
  Family family = Family::Generic;   // the kernels that run the block (hostlogic.hpp); md.gw = family_gw(family)
  int f32 = 0;              // sg_config.dtype = 1: fields, halo buffers, operator tiles and arithmetic are float (MFMA path)
  bool sym = false;         // MFMA path: all stress fields symmetric -> kernels touch only the i <= j lines
  DevBuf<int> sym_flag;     // device word set by an upload that is not symmetric
  // active (cell group, class) items of each region of a split stage (MFMA / lane paths), by sg_region
  DevBuf<int32_t> region_items[5];
  int32_t region_nitems[5] = {-1, -1, -1, -1, -1};  // -1: not built yet
  bool region_whole[5] = {false, false, false, false, false};  // no listed cell group is cut by the region's boxes
  DevBuf<double> fragF, fragG, fragL;  // MFMA operator fragment tables (float where f32)
  // G stages with the factorised volume term (kernels_mfma.hip mfma_stage_G<.., FACT = 1>; double, degrees 3 and 4;
  // SEIGEN_HIP_GQ): the Q tiles and the P_r tiles, or empty
  DevBuf<double> fragQ, fragP;
  bool gstash = true;      // ... at degree 4 launched in the form with the own traces out of the LDS stash (eight-wave blocks); SEIGEN_HIP_GSTASH=0: the form before it
  DevBuf<double> staging;  // host-layout staging buffer for layout conversion
  // large transfers: two pinned host slots + two device slots, so that the DMA of one chunk, the
  // layout kernel of the next and the host-side copy of the previous one overlap
  double* pin[2] = {nullptr, nullptr};
  DevBuf<double> dstage[2];
  hipEvent_t xfer_ev[2] = {nullptr, nullptr};
  DevBuf<unsigned long long> dbg;  // SEIGEN_HIP_STAMPS=1 (diagnostic builds): [kind][8] cycle sums
  size_t staging_len = 0;
  int64_t ncells = 0;
  int ncls = 0;
  // parameters
  bool params_set = false;
  double rho = 1.0, dt = 0.0, lam0 = 0.0, mu0 = 0.0;
  int per_cell = 0;
  DevBuf<double> lam_d, mu_d;
  DevBuf<double> rho2_d;     // per-cell density factors [cell][2] (kernels.hpp), or empty
  int rho_physical = 0;      // scalar density: 0 = rho*u0 + ..., 1 = u0 + (...)/rho
  SpongeTables sponge;
  SourceTables src;
  int64_t src_step = 0;
  // graph replay with a source: the step index lives in a device word that the captured launches read and a one-thread
  // launch bumps at the end of every step (kernels.hpp SrcStep); sg_step sets it to src_step before it replays.
  // Allocated by the first source and kept.
  DevBuf<int64_t> src_ctr_d;
  ReceiverTables rec;
  GaugeTables gge;
  MonitorTables mon;
  MeasureScratch msr;
  InjectTables inj;
  SpectraTables spc;
  PeakTables pk;
  FrameTables frm;
  GradTables grd;
  // whose launches the captured graphs contain: bit 0 the source's, bit 1 + k those of end-of-step hook k (stages.cpp hooks)
  uint32_t in_graphs = 0;
  CorrelationTables cor;
  // halo
  const double* ghost[4][6] = {};
  // execution
  hipStream_t stream = nullptr;
  bool own_stream = false;
  // Split stages (blocks with neighbours): SG_REGION_SECOND of a stage depends on the stage before it, not on the
  // FIRST launch of its own stage, so it may run on a second (lower-priority) stream and fill the slots that FIRST's
  // persistent blocks free as they drain (default; SEIGEN_HIP_OVERLAP=0: one stream).  ev_stage: everything before this stage's FIRST;
  // ev_second: the SECOND launch, which every later piece of work on `stream` waits for.
  bool overlap = false;
  hipStream_t stream2 = nullptr;
  hipEvent_t ev_stage = nullptr, ev_second = nullptr;
  bool second_pending = false;
  DevBuf<int32_t> nbr_tab;   // MFMA path: per-item neighbour table (StageArgs::nbr_tab)
  DevBuf<MfmaConst> mk_dev;  // MFMA path: scalar-load copy of the mesh constants (kernels.hpp MfmaConst)
  DevBuf<int32_t> ftab_dev;  // MFMA path, F stages: tabulated trace offsets (kernels.hpp mfma_trace_offsets)
  int grid_blocks = 0;  // persistent grid of the MFMA stage kernels: while an exchange is in flight ...
  int order_chunk = 0;  // MFMA path: items per XCD chunk of whole-block launches (StageArgs::order_chunk)
  int grid_full = 0;    // ... and otherwise (every block slot of the device)
  int ncu = 0;          // CUs of the handle's device
  T2Const t2c;          // 2-D tile kernels: kernarg copy of the mesh tables
  std::vector<std::pair<const void*, int>> tile_resident;   // ... and the blocks the device holds of each instantiation met so far (stages.cpp tile_resident)
  int tile_grid = 0, tile_grid_sponge = 0;    // 2-D tile kernels: cap of the grid in blocks of four waves, without / with a sponge (SEIGEN_HIP_TILE_GRID)
  // small blocks are launch-bound (config 1: six 5-us launches per step): sg_step replays captured
  // hipGraphs of one and of eight steps there; any setter that changes kernel arguments bumps the epoch
  bool graph_ok = false;
  uint64_t epoch = 0, graph_epoch = ~0ull;
  hipGraphExec_t graph1 = nullptr, graph8 = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  double last_ms = 0.0;
  bool timing = false;
  std::vector<hipEvent_t> ev_pool;   // per-launch event pairs, resolved lazily (no sync in the hot loop)
  // stage of pair k = events 2k, 2k+1 (6 = halo pack); + 16 for the FIRST, + 32 for the SECOND launch of a stage
  // that runs its two regions side by side on two streams (their pairs overlap in time: the stage counts the longer)
  std::vector<int> ev_stage_ids;
  double first_ms_pending[6] = {-1, -1, -1, -1, -1, -1};
  int first_recorded_stage = -1;         // stage whose FIRST launch recorded ev_stage last (SECOND must follow it)
  sg_counters_t counters = {};
  bool no_whole = false;             // SEIGEN_HIP_NO_WHOLE (diagnostic): region launches always test the boxes
  std::string err;
};

static_assert(SG_MAX_BOXES == SG_MAX_REGION_BOXES, "kernels.hpp and seigen_hip.h disagree on the box limit");

// (an allocation the device refuses is SG_ERR_NOMEM wherever it happens - DevBuf::alloc / upload, hipHostMalloc)
#define HIPCHECK(h, expr)                                                                        \
  do {                                                                                           \
    hipError_t _e = (expr);                                                                      \
    if (_e != hipSuccess) {                                                                      \
      (h)->err = std::string(#expr) + ": " + hipGetErrorString(_e);                              \
      return _e == hipErrorOutOfMemory ? SG_ERR_NOMEM : SG_ERR_DEVICE;                           \
    }                                                                                            \
  } while (0)

inline int fail(sg_handle* h, int code, const std::string& msg) {
  if (h) h->err = msg;
  return code;
}

inline bool field_is_stress(int f) { return f == SG_FIELD_S || f == SG_FIELD_SH; }

// work queued on `stream` from here on comes after the SECOND launch that may still run on stream2
inline int join_second(sg_handle* h) {
  if (h->second_pending) {
    HIPCHECK(h, hipStreamWaitEvent(h->stream, h->ev_second, 0));
    h->second_pending = false;
  }
  return SG_OK;
}

// the host waits for everything the handle has queued (both streams)
inline hipError_t sync_all(sg_handle* h) {
  if (h->second_pending) {
    hipError_t e = hipStreamWaitEvent(h->stream, h->ev_second, 0);
    if (e != hipSuccess) return e;
    h->second_pending = false;
  }
  return hipStreamSynchronize(h->stream);
}

// transfer.cpp: make the (i > j) lines of both stress buffers valid again and continue with the full-tensor kernels
int leave_sym_mode(sg_handle* h);
int queue_sym_mirrors(sg_handle* h);   // ... its launches alone: sg_inject changes the mode behind its own launch

// The tail of every setter of an end-of-step hook (StepSeries), once nothing of its own can fail any more: armed tables get
// their device-side step counter, a zero; the host waits for whatever still reads the old tables; a table that is not
// symmetric makes the block leave symmetric storage - the last step that can fail, and it fails before the mode changes;
// the new ones move into the handle; the captured graphs are out of date.
template <typename Tables>
int arm_hook(sg_handle* h, Tables& slot, Tables& fresh, bool armed, bool leave_sym = false) {
  const int64_t zero = 0;
  if (armed) HIPCHECK(h, fresh.ctr.upload(&zero, 1));
  HIPCHECK(h, sync_all(h));
  if (leave_sym)
    if (int rc = leave_sym_mode(h)) return rc;
  slot = std::move(fresh);
  h->epoch += 1;
  return SG_OK;
}

// hostlogic.hpp: the layout of the block's fields
inline Layout layout(const sg_handle* h) { return Layout{h->md.gw, h->ncls, h->re.nd}; }
// hostapi.cpp (hostlogic.hpp): the regions of a split stage
inline void region_boxes(const sg_handle* h, int region, std::vector<Box>& out) {
  region_boxes(h->cfg.dim, h->cfg.n, h->md.has_nbr, region, out,
               shell_width_x(h->md.gw, h->cfg.n[0], h->md.has_nbr[0] != 0, h->md.has_nbr[1] != 0));
}
int resolve_timing(sg_handle* h);
int finish_step_call(sg_handle* h);   // stages.cpp: the end of sg_step and comm_step (ev1, synchronise, last_ms)
// stages.cpp: one launch of the injector kernel (sym: the storage mode the launch writes in, -1: the handle's)
int queue_inject(sg_handle* h, hipStream_t stream, const InjectTables& it, const int64_t* ctr, int64_t step, int sym = -1);
int measure_prepare(sg_handle* h);    // api.cpp: the scratch of the monitor's samples (MeasureScratch), built once
// transfer.cpp: one buffer in the device layout of field `field` (doubles) -> host[cell][node][comp], behind everything queued
int download_layout(sg_handle* h, int field, const double* dev, double* host);
// comm.cpp
int comm_step(sg_handle* h, int64_t nsteps);
void comm_release(sg_handle* h);
