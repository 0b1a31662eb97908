/*
 * seigen_hip.h - C-ABI of libseigen_hip.so: the MI355X (gfx950) replacement for
 * the per-timestep hot path of devitocodes/seigen.
 *
 * Every entry point below replaces something Firedrake/PyOP2 generate or run
 * for `seigen/elastic.py` (paths relative to the reference checkout).  The
 * host side (seigen_amd/elastic.py) binds these with ctypes; INTEGRATION.md
 * shows the stub a maintainer of the reference would add.
 *
 * Conventions
 *   - plain C types only; no torch / HIP types in signatures (streams and
 *     device buffers cross as void*).
 *   - every call returns SG_OK (0) or a negative error code; the message is
 *     available from sg_last_error().  A call that fails leaves the handle as
 *     it was.
 *   - one host thread drives a handle.  The handle owns its device memory;
 *     host buffers are caller-owned and copied synchronously.
 *   - there is NO CPU fallback: sg_create fails if no HIP device is usable.
 *
 * Host field layout = the reference's `Function.dat.data` layout [upstream]:
 *   velocity  [cell][node][dim]        (VectorFunctionSpace, elastic.py:82)
 *   stress    [cell][node][dim][dim]   (TensorFunctionSpace, elastic.py:81)
 * cells ordered cube-major (x fastest) / simplex-class-minor, nodes on the
 * equispaced lattice ordered with the first reference coordinate fastest
 * (see DESIGN.md "Mesh and numbering").
 */
#ifndef SEIGEN_HIP_H
#define SEIGEN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version: bumped whenever the MEANING of an existing entry point, argument or field changes (new entry points
 * alone do not bump it).  A host that drives stages itself must check it: it is the only sign of such a change.
 *   1  rounds 1-4: SG_FIELD_UH holds utemp after stage UTEMP; stage S1 reads sh1 (SG_FIELD_SH) and utemp
 *   2  round 5: stage UTEMP leaves w = dt u1 + dt^3/24 utemp in SG_FIELD_UH, stage S1 = s0 + Minv g(w) reads
 *      SG_FIELD_UH and SG_FIELD_S only (enum sg_stage below); (u1, s1) unchanged to round-off */
#define SG_ABI_VERSION 2
int sg_abi_version(void);   /* the SG_ABI_VERSION the loaded library was built with (device-free) */

#define SG_OK 0
#define SG_ERR_ARG (-1)      /* bad argument */
#define SG_ERR_DEVICE (-2)   /* HIP runtime error / no device */
#define SG_ERR_STATE (-3)    /* call sequence error (e.g. params not set) */
#define SG_ERR_NOMEM (-4)

/* device-resident fields.  The ten Functions of elastic.py:93-103 map onto
 * four buffers because the fused stages never materialise uh2 / sh2 and
 * u0.assign(u1) / s0.assign(s1) (elastic.py:296,304) are in-place updates. */
enum sg_field {
  SG_FIELD_U = 0,  /* VelocityOld / VelocityNew   (u0, u1)      */
  SG_FIELD_UH = 1, /* VelocityHalf1 / VelocityTemp (uh1; after stage UTEMP: w = dt u1 + dt^3/24 utemp, see enum sg_stage) */
  SG_FIELD_S = 2,  /* StressOld / StressNew       (s0, s1)      */
  SG_FIELD_SH = 3  /* StressTemp / StressHalf1    (stemp, sh1)  */
};

/* the six fused launches of one LF4 step (elastic.py:291-304) */
enum sg_stage {
  SG_STAGE_UH1 = 0,   /* uh1   = Minv f(s0; u0)                          :292 */
  SG_STAGE_STEMP = 1, /* stemp = Minv g(uh1)                              :293 */
  SG_STAGE_U1 = 2,    /* u1 = rho*u0 + dt*uh1 + dt^3/24 * Minv f(stemp; u0); u0<-u1   :294-296 */
  SG_STAGE_SH1 = 3,   /* sh1   = Minv g(u1)                               :300 */
  SG_STAGE_UTEMP = 4, /* utemp = Minv f(sh1; u1)                          :301   - left in UH as w = dt*u1 + dt^3/24*utemp */
  SG_STAGE_S1 = 5     /* s1 = s0 + dt*sh1 + dt^3/24 * Minv g(utemp); s0<-s1           :302-304 - computed as s0 + Minv g(w) */
};
/* g is linear in the velocity, and utemp has no other consumer than sh2 = Minv g(utemp): dt*sh1 + dt^3/24*sh2 =
 * Minv g(dt*u1 + dt^3/24*utemp) (+ (dt + dt^3/24) S with a source).  Stage UTEMP therefore leaves that ONE velocity w in
 * the UH buffer (its fused epilogue reads u1 beside its result) and stage S1 reads w and s0 only - neither sh1 nor a
 * second right-hand side: 6 of the 21 words per node the stress update moved.  (u1, s1) are the reference's to round-off;
 * what a caller finds in SG_FIELD_UH after a step is w, not utemp.  SG_FIELD_SH holds sh1 as before. */

/* which cubes of the block a stage launch covers (halo overlap) */
enum sg_region {
  SG_REGION_ALL = 0,
  SG_REGION_INTERIOR = 1, /* cubes whose stencil needs no remote trace */
  SG_REGION_BOUNDARY = 2, /* the one-cube shell next to sides that have a neighbour block */
  /* the same stage cut differently, for the pipelined exchange (seigen_amd/parallel.py): */
  SG_REGION_FIRST = 3,    /* the shell and the lower half of the interior: everything whose results
                             the neighbours wait for, inside one large launch */
  SG_REGION_SECOND = 4    /* the rest of the interior: runs while the traces of FIRST travel */
};

typedef struct sg_handle sg_handle;

typedef struct sg_config {
  int32_t dim;       /* 1, 2 or 3          (ElasticLF4.create(..., dimension), elastic.py:28) */
  int32_t degree;    /* 1..4               (ElasticLF4.create(..., degree)) */
  int32_t n[3];      /* squares / cubes per axis in THIS block */
  double h[3];       /* cell size per axis */
  double origin[3];  /* physical coordinate of the block's low corner (of cube -cube0, see below) */
  int32_t diagonal;  /* 2-D: 0 = "left" (Firedrake default), 1 = "right": how each square is cut into two triangles;
                        2 = not at all: quadrilateral cells (dim 2) or hexahedral cells (dim 3) with
                        the tensor-product element DQ_k, what FunctionSpace(mesh, "DG", k) (elastic.py:81-82) is on
                        a quadrilateral / hexahedral mesh.  3-D simplicial blocks ignore 0 / 1 (one Kuhn cut). */
  int32_t nbr_mask;  /* bit (2*axis + side) set: that side touches another block (halo), else free surface */
  int32_t device;    /* HIP device ordinal */
  int32_t dtype;     /* 0: FP64 storage and arithmetic - the reference's precision (elastic.py:442 'double'),
                        the parity and headline mode; 1: FP32 storage and arithmetic, the separately reported
                        second mode of SURVEY 8d (32 B per DoF-update; 3-D blocks on the MFMA path, 2-D blocks on the MFMA
                        tile kernels; SG_ERR_ARG elsewhere: 1-D blocks, forced generic / lane kernels).  The C-ABI
                        keeps double on the host side in both modes; halo buffers hold the device type. */
  void* stream;      /* hipStream_t to launch on, or NULL for the handle's own stream (non-blocking, made by sg_create,
                        destroyed by sg_destroy).  A caller's stream: any stream of `device` that is not the null / legacy
                        stream - default flags (blocking) or hipStreamNonBlocking, any priority, torch's
                        (torch.cuda.Stream().cuda_stream) included; several handles may share one, and sg_correlate takes
                        handles on one stream or on different ones.  It stays the caller's: the library never destroys it,
                        sg_destroy waits for what the handle queued on it and leaves it alive and idle, and the caller
                        destroys it after the last handle on it.  Everything the handle launches goes on it - stage
                        kernels, captured graphs (captured on it, thread-local mode: the calling thread must not have a
                        capture of its own under way on it) and their replays, pre-passes, sources, recorder, monitor,
                        injectors, packs, the layout kernels and asynchronous copies of transfers - except the
                        SG_REGION_SECOND launches of a block with neighbours, which run on a second stream of the
                        library's own (sg_get_second_stream), ordered against this one by events in both directions.
                        Calls that return with the launches only QUEUED, ordered on the stream against whatever the
                        caller puts there before and after, and never waiting on the host: sg_run_stage, sg_end_step,
                        sg_halo_pack, sg_halo_pack_sides, sg_apply_F, sg_apply_G, sg_correlate, sg_reset_correlation
                        (release = 0), sg_get_field_dev, sg_get_spectrum_dev, sg_get_peaks_dev, sg_get_frame_dev and sg_get_gradient_dev (their
                        tables in place) and sg_set_field_dev (but for a stress
                        handed to a block in symmetric storage).  Calls that make the host wait for the stream:
                        sg_create (the whole device), sg_step and the native exchange's stepping (to the end of what
                        they queued), every setter (sg_set_* but sg_set_field_dev, sg_leave_sym), sg_inject, sg_measure,
                        every transfer and read-out through host memory (sg_set_field, sg_get_field, their _range
                        forms, sg_get_spectrum, sg_get_peaks, sg_get_gradient, sg_get_receivers, sg_get_monitor, sg_get_correlation, sg_get_counters
                        with timing on), sg_set_field_dev of a stress handed to a block in symmetric storage, sg_sync
                        and sg_destroy.  The set-up paths also use the legacy stream (hipMemset, hipMemcpy)
                        after that wait and return when those have completed (a fill is followed by a blocking copy); a
                        non-blocking stream is not ordered against the legacy stream, so a fill that no host wait follows
                        (sg_correlate's accumulator, sg_comm_selftest's buffers) goes on the handle's stream. */
  int32_t cube0[3];  /* index of the block's first square / cube counted from `origin` (0: origin is the block's own low
                        corner).  Node coordinates are origin + (cube0 + cube + lattice) * h with the integers added
                        first: a block of a partitioned mesh, or a slab / sub-box of a block evaluated on its own
                        (sg_block_node_coords), given the MESH's origin and its integer offset, gets bit for bit the
                        coordinates the whole mesh gets - a source box whose faces lie on node lines
                        (explosive_source_lf4.py:36-38) then selects the same nodes under every partition. */
  int32_t pad_;
} sg_config;

typedef struct sg_info {
  int32_t dim, degree;
  int32_t nd;        /* scalar nodes per cell */
  int32_t nf;        /* nodes per facet */
  int32_t nfaces;    /* facets per cell */
  int32_t nclasses;  /* simplices per square / cube */
  int64_t ncells;
  int64_t u_dofs;    /* dim   * nd * ncells */
  int64_t s_dofs;    /* dim^2 * nd * ncells */
  int32_t halo_faces[6]; /* cell-facets lying on each block side (2*axis+side) */
} sg_info_t;

typedef struct sg_counters {
  double kernel_ms[6];   /* accumulated device time per stage (hipEvent), only when timing is enabled */
  int64_t launches[6];
  int64_t steps;
  /* halo layer (the role of ParLoopHaloEnd, tests/tiling/utils.py:144) */
  double halo_pack_ms;       /* device time of the trace-pack launches, only when timing is enabled */
  int64_t halo_pack_launches;
  int64_t halo_bytes_packed; /* bytes written to send buffers = bytes this block hands to the transport */
} sg_counters_t;

/* ---- lifecycle ------------------------------------------------------------------- */
/* replaces: function-space/field construction (elastic.py:66-103) and
 * ExplicitElasticLF4.setup (elastic.py:369-385: element-wise inverse mass). */
int sg_create(const sg_config* cfg, sg_handle** out);
void sg_destroy(sg_handle* h);
const char* sg_last_error(const sg_handle* h); /* h may be NULL: error of the last failed sg_create */
int sg_get_info(const sg_handle* h, sg_info_t* out);
int sg_sync(sg_handle* h);
/* the hipStream_t the handle launches on (its own or the one given in sg_config): the host layer
 * makes it the current stream around its torch.distributed calls, which order themselves against
 * the current stream (the role PyOP2's implicit halo/compute ordering has, elastic.py:404-436) */
int sg_get_stream(const sg_handle* h, void** stream);
/* Blocks with neighbours launch SG_REGION_SECOND of a split stage on a second, lower-priority stream beside
 * SG_REGION_FIRST of the same stage (it depends on the stage before, not on FIRST; SEIGEN_HIP_OVERLAP=0 switches
 * this off); everything queued later on the main stream waits for it.  NULL if the handle has no such stream.
 * Call order: sg_run_stage(stage, SG_REGION_SECOND) must directly follow sg_run_stage(stage, SG_REGION_FIRST) of
 * the SAME stage (FIRST records the event SECOND's stream waits for); anything else returns SG_ERR_STATE.
 * Timing counters (sg_get_counters kernel_ms) count such a stage once, with the longer of its two launches.
 * For instrumentation: the host layer records an event on it to tell how long the next stage really waited
 * for traces (what ParLoopHaloEnd times in the reference, tests/tiling/utils.py:144). */
int sg_get_second_stream(const sg_handle* h, void** stream);

/* physical coordinates of the DG nodes, [cell][node][dim]; `degree` may differ
 * from the solver's (e.g. 4 for the DG4 sponge space of
 * tests/explosive_source/explosive_source_lf4.py:43).  Replaces what
 * Function.interpolate(Expression) needs from the mesh (elastic.py:141,154). */
int sg_node_coords(const sg_handle* h, int degree, double* out, size_t nbytes);
/* the same from a configuration alone (device-free; cfg->device / stream ignored) */
int sg_block_node_coords(const sg_config* cfg, int degree, double* out, size_t nbytes);

/* ---- parameters (plain attributes density, dt, mu, l: eigenmode_2d.py:17-20) ------- */
/* per_cell = 0: lambda/mu point to one value each; 1: one value per cell
 * (build-defined heterogeneous extension). */
int sg_set_params(sg_handle* h, double density, double dt, const double* lambda, const double* mu, int per_cell);
/* Density beyond the scalar of sg_set_params (which it overrides until the next sg_set_params):
 *   per_cell = 0: rho[0];  1: one value per cell (SURVEY 8 f2 "(and rho)", build-defined like per-cell
 *   lambda/mu: each cell's velocity update uses its own density).
 *   physical = 0: the explicit reference's update u1 = rho*u0 + dt*uh1 + dt^3/24*uh2 - explicit
 *   mode keeps only rhs(form_u1) and applies the unweighted mass inverse (elastic.py:341-345,
 *   :354-356, :376), which is the physical update only for rho = 1;
 *   physical = 1: u1 = u0 + (dt*uh1 + dt^3/24*uh2)/rho, what the implicit form solves (elastic.py:175-178). */
int sg_set_density(sg_handle* h, const double* rho, int per_cell, int physical);

/* ---- field transfer (u0.assign(...), s0.assign(...): eigenmode_2d.py:32,36) -------- */
int sg_set_field(sg_handle* h, int field, const double* host, size_t nbytes);
int sg_get_field(sg_handle* h, int field, double* host, size_t nbytes);

/* the same for `ncells` consecutive cells starting at `cell0` (chunked transfer of large fields) */
int sg_set_field_range(sg_handle* h, int field, int64_t cell0, int64_t ncells, const double* host, size_t nbytes);
int sg_get_field_range(sg_handle* h, int field, int64_t cell0, int64_t ncells, double* host, size_t nbytes);

/* ---- device transfers: the same between the field and a DEVICE buffer of the caller's, on the handle's stream -------
 * The caller's buffer is memory of the handle's device in the host layout [cell][node][comp] of sg_get_field_range, for
 * `ncells` cells from `cell0`, of the type `dtype` (0 = double, 1 = float: the CALLER's buffer, independent of
 * sg_config::dtype); nbytes is exactly its size.  A double block into a float buffer, and doubles into a float block,
 * round once, (float)v - bitwise what sg_set_field gives for the same doubles; float into double is exact.  The library
 * does not test that the pointer is device memory: that is the caller's contract.  The buffer stays alive until the
 * stream has passed the launch.  SG_ERR_ARG: a null pointer, a dtype outside 0 .. 1, a field, range or nbytes that
 * sg_get_field_range refuses.  A call that fails leaves fields, storage mode, write counts and epoch as they were.
 * sg_get_field_dev returns with its launch only QUEUED on the handle's stream, ordered against whatever the caller puts
 *   there before and after, and never waits on the host; in symmetric-stress storage the (i > j) entries are delivered
 *   from their mirrors, as sg_get_field does.
 * sg_set_field_dev is queued only as well, EXCEPT for a stress field handed to a block in symmetric storage: that
 *   upload tests the caller's data for symmetry, the call waits for the stream and reads the answer, and an asymmetric
 *   stress makes the block leave symmetric storage (sg_leave_sym) and the upload run again in full storage - the rule
 *   of sg_set_field.  Cells outside the range and the padding lanes of the layout are not written.
 * sg_get_spectrum_dev delivers one accumulator of sg_set_spectra (always double on the device; errors and mirror rule
 *   of sg_get_spectrum), queued only. */
int sg_get_field_dev(sg_handle* h, int field, int64_t cell0, int64_t ncells, void* dev_out, int dtype, size_t nbytes);
int sg_set_field_dev(sg_handle* h, int field, int64_t cell0, int64_t ncells, const void* dev_in, int dtype, size_t nbytes);
int sg_get_spectrum_dev(sg_handle* h, int field, int freq, int part, void* dev_out, int dtype, size_t nbytes);
/* The launch plan of one such transfer (device-free): a block whose layout puts gw cubes of ncls cells side by side
 * (1: host layout, 16, 64), nd nodes of ncomp components, dev_bytes per word on the device and caller_bytes in the
 * caller's buffer (4 or 8 each).  out = first item (cube group * ncls + class; gw = 1: cell), number of items, rows
 * (node * ncomp + comp) per slice, slices per item, blocks of the grid (at most SG_XFER_GRID_CAP: the grid strides over
 * the (item, slice) units beyond it), bytes of LDS per block. */
#define SG_XFER_GRID_CAP 1048576
int sg_xfer_plan(int gw, int ncls, int nd, int ncomp, int dev_bytes, int caller_bytes, int64_t cell0, int64_t ncells, int64_t out[6]);

/* ---- frames: a field rastered on a pixel lattice aligned with the block's cubes, on the device -----------------------
 * Along a FREE axis a every cube holds m[a] pixels: pixel i * m[a] + j (0 <= j < m[a]) belongs to the block's cube i, lies
 * at the cube fraction t = (j + 1/2) / m[a], physically at origin[a] + (cube0[a] + i + t) * h[a]; the extent is
 * P[a] = n[a] * m[a].  A FIXED axis (fixed[a] = 1) is the single plane x_a = at[a] - a slice - of extent 1: the cube layer
 * and t in [0, 1] come from (at[a] - origin[a]) / h[a] by the rule of sg_locate_points (on a grid plane the lower cube
 * where the mesh has one); a block that does not hold that layer owns nothing of the frame: the call succeeds and
 * launches nothing.  Limits: 1 <= m[a] <= 8, at most 64 in-cube pixels Q = prod m[a] over the free axes, at least one
 * free axis; entries of axes beyond dim are ignored.  Every cube of a block has the same cell class k(q) and reference
 * coordinates xi(q) for its in-cube pixel q = j0 + m0 * (j1 + m1 * j2): what sg_locate_points returns on the UNIT block
 * (same dim, diagonal and cell kind, n = 1, h = 1, origin = 0, cube0 = 0) at the point t - the lowest class whose
 * coordinates pass the 1e-12 tests - and the weights phi[q][a] are sg_tabulate_cell at xi(q), as for the receivers. */
typedef struct sg_frame {
  int32_t m[3];      /* pixels per cube along axis a (>= 1); ignored where fixed[a] */
  int32_t fixed[3];  /* 1: the frame is the single plane x_a = at[a] (a slice); extent 1 along a */
  double  at[3];
} sg_frame;
/* sg_get_frame_dev writes out[comp][P2][P1][P0] (axes beyond dim have extent 1) of field `field` (any of
 * sg_get_field_dev's) into DEVICE memory of the caller's, of type dtype (0 = double, 1 = float); the components in the
 * host layout's order - dim of a velocity, dim^2 row-major of a stress, in symmetric storage the (i > j) entries from
 * their mirrors.  stride = { comp, axis 2, axis 1, axis 0 } in elements (non-negative), NULL: contiguous; nbytes must
 * cover the largest index touched, else SG_ERR_ARG and nothing is queued.  Strides let the blocks of a mesh write into
 * views of one image.  The value is the receivers':
 *   out[c][pixel] = sum_a phi[q][a] * (double)field[cell(cube, k(q))][a][c]
 * over a ascending with fma from zero in double, rounded once where dtype is float - the same bits on every kernel
 * family, storage mode and stream.  The launch is only QUEUED on the handle's stream under the ordering rules of
 * sg_get_field_dev.  The tables of a frame specification (classes, weights, listed cube groups) live on the device with
 * the handle, which keeps those of the last specification: a call with another specification builds them first (an
 * allocation and blocking copies, as a setter does), a repeated one does not.  A call that fails leaves the handle as it
 * was.  SG_ERR_ARG: a null pointer, a field or dtype outside its range, a frame beyond the limits, a negative stride,
 * nbytes too small. */
int sg_get_frame_dev(sg_handle* h, int field, const sg_frame* fr, void* dev_out, int dtype, const int64_t stride[4], size_t nbytes);
/* The plan of a frame on a block (device-free; the kernel family, hence the group width gw of the layout, as sg_create
 * chooses it): out = { P0, P1, P2, Q, owns (0 / 1), layer of axis 0, 1, 2 (block-local cube index of a fixed axis the
 * block holds, else -1), listed groups of gw cubes, units (waves' (64 cubes, class) units; gw = 1: (cube, in-cube pixel)
 * threads), blocks of 256 threads along x (at most SG_FRAME_GRID_CAP: the grid strides over the units beyond it; the
 * output component is the grid's y), gw }.  groups (or NULL) receives the listed groups, ascending, at most max_groups. */
#define SG_FRAME_GRID_CAP 65536
int sg_frame_plan(const sg_config* cfg, const sg_frame* fr, int64_t out[12]);
int64_t sg_frame_groups(const sg_config* cfg, const sg_frame* fr, int32_t* groups, int64_t max_groups);
/* cls[Q], xi[Q][dim] and phi[Q][nd] of the in-cube pixels (device-free; degree <= 8 as sg_locate_points) */
int sg_frame_weights(const sg_config* cfg, int degree, const sg_frame* fr, int32_t* cls, double* xi, double* phi);

/* ---- gradient: strain rate, divergence and curl of a velocity field at the nodes, on the device -----------------------
 * The broken (cell-local) gradient of field `field` (SG_FIELD_U or SG_FIELD_UH; a stress field: SG_ERR_ARG): the gradient of
 * every cell's own polynomial at the cell's nodes, no facet terms - exact for every member of the element's space.  For the
 * cell of class k, node a, velocity component i:
 *   t_r[a][i] = sum_b C_r[a][b] * (double)u[b][i]      C_r[a][b] = d(phi_b)/d(xi_r) at the reference point of node a
 *   G_ij[a]   = sum_r J[k][r][j] * t_r[a][i]           J[k][r][j] = d(xi_r)/d(x_j) (sg_mesh_tables' jinv)
 * kind 0: the gradient, ncomp = dim^2, component c = i * dim + j holds d(u_i)/d(x_j);
 * kind 1: the divergence, ncomp = 1;
 * kind 2: the curl: 3-D ncomp = 3, (G21 - G12, G02 - G20, G10 - G01); 2-D ncomp = 1, G10 - G01; 1-D: SG_ERR_ARG;
 * kind 3: the symmetric strain rate, ncomp = dim^2, 0.5 * (G_ij + G_ji), the diagonal entries G_ii themselves.
 * Arithmetic: nodal values are converted to double first; t_r is formed with fma from zero over b ascending - simplices over
 * the dense row, tensor-product cells over the P + 1 nodes of the line through a along axis r (the 1-D derivative matrix,
 * what sum factorisation gives); G_ij with fma from zero over r ascending; the combinations of kinds 1 to 3 are single
 * additions, subtractions and one multiplication by 0.5, each rounded on its own in the order written, the divergence as
 * (G00 + G11) + G22.  The bits therefore depend on the cell's nodal values, the cell type, the degree, the class and h[]
 * alone - not on the kernel family, the layout of the fields, the stream, the range or the caller's dtype.
 * sg_get_gradient_dev writes dev_out[cell][node][ncomp] for `ncells` cells from `cell0` into DEVICE memory of the caller's of
 * type dtype (0 = double, 1 = float, rounded once); nbytes is exactly its size; cell order, range rule and padding rule are
 * sg_get_field_dev's, and so are the ordering rules: the launch is only QUEUED on the handle's stream, never waits on the
 * host, and may be called between graph replays.  It writes no field and changes neither the storage mode nor a counter.
 * The tables (C_r, J) live on the device with the handle from the first call to sg_destroy: that call builds them first (two
 * allocations and blocking copies, as a setter does), no later one does.  A call that fails leaves the handle as it was.
 * SG_ERR_ARG: a null pointer, a field, kind or dtype outside its range, a range or nbytes that sg_get_field_range would
 * refuse for a field of ncomp components.
 * sg_get_gradient is the same into HOST memory, doubles: a temporary device buffer, one blocking copy; it waits for the
 * stream like every host read-out. */
int sg_get_gradient_dev(sg_handle* h, int field, int kind, int64_t cell0, int64_t ncells, void* dev_out, int dtype, size_t nbytes);
int sg_get_gradient(sg_handle* h, int field, int kind, int64_t cell0, int64_t ncells, double* host_out, size_t nbytes);
/* The tables of a block (device-free): C[r][a][b], dim * nd * nd doubles, dense for both cell types - bitwise
 * sg_tabulate_grad_cell at the nodes' reference points (lattice / degree) - and J[cls][3][3], the block's jinv.  Either may
 * be NULL; returns the number of doubles of C (NULL, NULL: a size query), or SG_ERR_ARG. */
int64_t sg_gradient_tables(const sg_config* cfg, double* C, double* J);
/* The class frame of the 3-D matrix-pipe F stages (device-free): tetrahedra of a 3-D block, class k = the reference simplex
 * with the axes permuted by p[k].  Per class k = 0 .. 5: p[k][3]; s[k][3] = 1 / h[p[k][m]]; cn[k][4][2], the scaled normal of
 * facet f at its non-zero columns {0} {0,1} {1,2} {2} of the permuted order (second entry 0 on facets 0 and 3);
 * lines[k][2][36], per storage (0: full tensor, 1: symmetric) the line offsets in values of the field type: own[9] (slot
 * 3 a + b: the line of T(p[a], p[b])), trace[4][6] (the neighbour lines facet f reads, in the order of kernels.hpp
 * MfmaClassConst::cf_tr) and vel[3] (the line of velocity component p[i]).
 * E and Ed, [3][nd][nd] each: the dense volume operators E_r (own-trace half of the flux folded in) and their differences
 * E'_m = E_m - E_(m-1) as the F stages' tiles hold them (before the sign).  Any output may be NULL; returns nd, or SG_ERR_ARG
 * (also when the block's tables do not have the shape the kernels are written to). */
int64_t sg_mfma_class_frame(const sg_config* cfg, int32_t* p, double* s, double* cn, int32_t* lines, double* E, double* Ed);
/* The launch plan of one call (device-free), the counterpart of sg_xfer_plan: out = first item, number of items, output nodes
 * per slice, slices per item, blocks of the grid (at most SG_XFER_GRID_CAP: the grid strides over the (item, slice) units
 * beyond it), bytes of LDS per block (at most 64 KiB: the item's velocity block and a slice's values as doubles, pitch
 * gw + 1).  gw = 1: items are cells, a thread per (cell, node), no LDS. */
int sg_gradient_plan(int gw, int ncls, int nd, int dim, int ncomp, int dev_bytes, int caller_bytes, int64_t cell0, int64_t ncells,
                     int64_t out[6]);

/* ---- absorption (elastic.py:136-141, :207-208) ------------------------------------ */
/* sigma_nodes: [cell][nd(sigma_degree)] nodal values of the DG_q sponge field, or NULL to disable. */
int sg_set_absorption(sg_handle* h, const double* sigma_nodes, int sigma_degree);

/* ---- source (elastic.py:149-154, :217-218, :285-288) ------------------------------- */
/* Sparse nodal source: `nnz` scalar DG nodes (flat index = cell*nd + node) carry a
 * source; values[k][i][dim*dim] is the nodal S_ij of entry i during step k
 * (k = 0 .. nsteps-1 counted from this call; no source afterwards).  This is the
 * re-interpolated `source_function` of elastic.py:285-288 restricted to its
 * support.  nsteps = -1: a time-independent source, values[0][i][dim*dim] holds at
 * every step.  nnz = 0 disables.  A node listed more than once receives the SUM of its
 * entries (added up in the order listed, once, on the host: deterministic). */
int sg_set_source(sg_handle* h, int64_t nnz, const int64_t* nodes, int64_t nsteps, const double* values);
/* The same for a SEPARABLE source S_ij(node, step k) = weights[k] * pattern[node][dim*dim] - what every source of
 * the reference's tests is (the indicator of a box times a Ricker wavelet re-interpolated at every step,
 * tests/explosive_source/explosive_source_lf4.py:36-40 with elastic.py:285-288): one slice of nodal values and
 * one factor per step (k = 0 .. nsteps-1 counted from this call; no source afterwards) instead of a table of
 * nsteps * nnz * dim^2 values.  The product weights[k] * pattern is rounded before it is added, so the result is
 * bitwise what sg_set_source gives for the table of those products (node lists without repeated nodes; the entries
 * of a repeated node are summed first, here of the pattern, there of the products). */
int sg_set_source_separable(sg_handle* h, int64_t nnz, const int64_t* nodes, const double* pattern, int64_t nsteps,
                            const double* weights);
/* The reference's explosive source itself, from its parameters (tests/explosive_source/explosive_source_lf4.py:36-40):
 *   S_ij(x, t) = delta_ij w(t) at the DG nodes x inside the CLOSED box lo <= x <= hi (the nodal interpolation of the
 *   box indicator, elastic.py:149-154), w(t) = (-1 + 2 a (t - t0)^2) exp(-a (t - t0)^2),
 * for the steps k = 0 .. nsteps-1 counted from this call, evaluated at t = t_first + k * dt_step (elastic.py:285-288
 * sets t to the time of the step before re-interpolating: t_first = dt, dt_step = dt for a run from t = 0).
 * lo, hi: dim doubles each.  Node coordinates are those of sg_node_coords.  A convenience over
 * sg_set_source_separable (same storage, same rounding rule); a box that contains no node of this block disables
 * the source of the block. */
int sg_set_source_box_ricker(sg_handle* h, const double* lo, const double* hi, double a, double t0, double t_first,
                             double dt_step, int64_t nsteps);

/* ---- the hot path ---------------------------------------------------------------- */
/* whole steps (all six stages, source included); replaces the body of
 * ElasticLF4.run's while-loop (elastic.py:283-313).  A block with neighbours needs a communicator
 * (sg_comm_init): the exchanges then run inside this call; without one, drive stages and halo from the host
 * (sg_run_stage + sg_halo_pack_sides + your transport). */
int sg_step(sg_handle* h, int64_t nsteps);
/* one fused stage over a region (multi-block overlap and stage-level tests). */
int sg_run_stage(sg_handle* h, int stage, int region);
/* end a manually staged step: advance the source-amplitude index; receivers, monitor and injectors take their turn */
int sg_end_step(sg_handle* h);

/* ---- receivers (tests/explosive_source/uy.py:31-43: VelocityNew written to a VTU file at every step, three points
 * probed in every 5th file with vtktools.vtu.ProbeData) ------------------------------------------------------------
 * A receiver is a physical point; its samples are taken on the device inside the time loop.  A step is a completed LF4
 * step counted from the arming call - through sg_step (graph replay or eager, with or without a communicator) or through
 * sg_end_step after host-driven stages.  Sample j (0-based) is taken after step (j+1)*every.  Per receiver a sample holds
 * the velocity u1 (what bit 0: dim values) and then the stress s1 (bit 1: dim x dim, row-major; in symmetric-stress
 * storage the i > j entries are their mirrors), each value sum_a phi_a(xi) field[cell][a][c] over the nodes a in
 * ascending order, in double with fma (FP32 blocks convert every nodal value first): bitwise the same under graph replay
 * and eager launches, for one sg_step(n) and n calls of sg_step(1), for host-driven stages, and on a split block.
 * The cell and xi of a point: sg_locate_points.  A block owns a receiver when the chosen cube (in the mesh's indices)
 * lies in it: under any partition every point inside the mesh has exactly one owner, a point outside none.
 * Arm: nrec points [nrec][dim] (all of the mesh's receivers: each block keeps the ones it owns), owned[nrec] out (0/1,
 * may be NULL), what = bit 0 velocity | bit 1 stress, every >= 1, capacity = samples the device buffer holds.  nrec = 0
 * disarms; re-arming discards the old samples; a failed call leaves the previous receivers recording, samples intact.
 * sg_step(n) whose samples would exceed the capacity returns SG_ERR_STATE before it queues anything (fields, counters
 * and trace untouched); sg_end_step of a step due a sample the trace has no room for returns SG_ERR_STATE and does not
 * count the step.  No receivers armed: no extra launch, the same captured graphs. */
int sg_set_receivers(sg_handle* h, int64_t nrec, const double* pts, int what, int64_t every, int64_t capacity,
                     int32_t* owned);
/* samples taken so far -> out[nsamples][nrec][ncomp] (ncomp = dim * bit0 + dim^2 * bit1), rows of receivers this block
 * does not own are 0.0; nbytes must be that of `capacity` samples; *nsamples = samples taken.  Replaces the host-side
 * probe of every 5th VTU file (uy.py:36-43, vtktools.vtu.ProbeData). */
int sg_get_receivers(sg_handle* h, double* out, size_t nbytes, int64_t* nsamples);

/* ---- gauges: strain rate, rotation rate and dilatation rate recorded at physical points inside the time loop - what a
 * strainmeter, a fibre (DAS) or a rotational seismometer delivers, beside the receivers' velocity seismograms -----------------
 * A gauge is a physical point with a `kind`, sg_get_gradient_dev's: 0 gradient, 1 divergence, 2 curl, 3 symmetric strain rate,
 * with that call's ncomp and component order; kind 2 in 1-D: SG_ERR_ARG.  Its value is the broken gradient of the velocity at
 * the point: the gradient of the polynomial of the cell that holds it.
 * The cell and xi of a point: sg_locate_points.  A block owns a gauge when the chosen cube (in the mesh's indices) lies in it:
 * under any partition every point inside the mesh has exactly one owner, a point outside none.  The broken gradient is
 * discontinuous across cells: on a grid line a gauge reads the LOWER cell's polynomial (the one-sided value from below), as a
 * receiver reads the lower side.
 * Arithmetic, for a gauge in a cell of class k, velocity component i:
 *   D_r[a]  = d(phi_a)/d(xi_r) at xi            bitwise sg_tabulate_grad_cell(cell_type, dim, degree, 1, xi, .), dense over all
 *                                               nd nodes for both cell types
 *   t_r[i]  = sum_a D_r[a] * (double)u[a][i]    with fma from zero over a ascending
 *   G_ij    = sum_r J[k][r][j] * t_r[i]         with fma from zero over r ascending; J is sg_gradient_tables' J
 * and the combinations of kinds 1 to 3 are the gradient's: single additions, subtractions and one multiplication by 0.5, each
 * rounded on its own in the order written there, the divergence as (G00 + G11) + G22.  FP32 blocks convert every nodal value
 * first.  The bits therefore depend on the cell's nodal values, the point, the cell type, the degree, the class and h[] alone -
 * not on the kernel family, the layout of the fields, the stream, graph replay or the partition.
 * Series: a step is a completed LF4 step counted from the arming call - through sg_step (graph replay or eager, with or without
 * a communicator) or through sg_end_step after host-driven stages.  Sample j (0-based) is taken of u1 after step (j+1)*every.
 * Arm: npts points [npts][dim] (all of the mesh's gauges: each block keeps the ones it owns), owned[npts] out (0/1, may be
 * NULL), every >= 1, capacity = samples the device buffer holds.  npts = 0 disarms; re-arming discards the old samples; a
 * failed call leaves the previous gauges recording, samples intact.  sg_step(n) whose samples would exceed the capacity
 * returns SG_ERR_STATE before it queues anything (fields, counters and trace untouched); sg_end_step of a step due a sample
 * the trace has no room for returns SG_ERR_STATE and does not count the step.  No gauges armed: no extra launch, the same
 * captured graphs. */
int sg_set_gauges(sg_handle* h, int64_t npts, const double* pts, int kind, int64_t every, int64_t capacity, int32_t* owned);
/* samples taken so far -> out[nsamples][npts][ncomp], rows of gauges this block does not own are 0.0; nbytes must be that of
 * `capacity` samples; *nsamples = samples taken. */
int sg_get_gauges(sg_handle* h, double* out, size_t nbytes, int64_t* nsamples);
/* One shot: the same arithmetic on `field` (SG_FIELD_U or SG_FIELD_UH; a stress field: SG_ERR_ARG) as it stands behind
 * everything the handle has queued, into host_out[npts][ncomp] (nbytes exactly that); rows not owned are 0.0; owned[npts] out
 * (may be NULL).  Temporary device buffers and one blocking copy, as sg_get_gradient; it arms nothing, counts nothing, writes no
 * field, and may be called between graph replays. */
int sg_probe_gradient(sg_handle* h, int field, int kind, int64_t npts, const double* pts, double* host_out, size_t nbytes,
                      int32_t* owned);
/* device-free, like sg_injector_weights: cell[k] (or -1) and dphi[k][dim][nd] = D_r[a] of point k (0 where -1); degree <= 4.
 * Returns nd, or SG_ERR_ARG. */
int64_t sg_gauge_weights(const sg_config* cfg, int64_t npts, const double* pts, int64_t* cell, double* dphi);

/* ---- injectors: force and stress series added at physical points inside the time loop - the driving side beside the
 * receivers, what puts a point force into the velocity equation or a data residual into an adjoint field ----------------
 * An injector is the transpose of a receiver.  Where the recorder forms sum_a phi_a(xi) field[cell][a][c], an injector adds
 *   field[cell][a][c] += amp[c] * psi_a,   psi = Mhat^-1 phi(xi) / |det J|,
 * the L2 projection of amp * delta(x - x_r) onto the element: sum_a psi_a (|det J| Mhat v)_a = v(x_r) for every v of the
 * element's space.  Mhat is the cell type's own (simplex or tensor-product), |det J| the product of the cell sizes.
 * what: bit 0 adds to the velocity SG_FIELD_U (dim values), bit 1 to the stress SG_FIELD_S (dim x dim, row-major); per point
 * amp holds the velocity's values and then the stress's, ncomp = dim * bit0 + dim^2 * bit1 as for the receivers.
 * The cell and xi of a point: sg_locate_points.  A block owns an injector when the chosen cube (in the mesh's indices) lies
 * in it: under any partition every point inside the mesh has exactly one owner, a point outside none.  On a grid line the
 * lower cell gets the whole delta - the transpose of the receiver reading the lower side.  Every block is handed all of the
 * mesh's points [npts][dim] and keeps the ones it owns; owned[npts] out (0/1, may be NULL).
 * Arithmetic: the host groups the owned points by cell; one thread per (cell with points, node a, component q) forms
 * v = sum_r fma(amp[r][q], psi_r[a], v) from zero over that cell's points in the order listed, then field = field + v in
 * double (FP32 blocks convert, add and round once).  No atomics: the bits depend only on the field contents, the amplitudes
 * and the points - the same under graph replay and eager launches, for one sg_step(n) and n calls of sg_step(1), for
 * host-driven stages with sg_end_step, with timing on or off, and on a split block.
 * Symmetric-stress storage: a stress table that is symmetric to the bit (the owned points', every entry) writes the i <= j
 * lines only; one that is not makes THIS block leave symmetric storage at the call, as a non-symmetric source does
 * (sg_get_sym / sg_leave_sym: the blocks of a mesh must agree).
 * The library adds exactly amp * psi: 1/rho, dt, or the 1/wk of an adjoint source in the energy inner product are the
 * caller's, folded into amp.
 * Series: entry k (k = 0 .. nsteps-1) is added at the END of step k+1 counted from the arming call - through sg_step (graph
 * replay or eager, with or without a communicator) or through sg_end_step after host-driven stages - after the recorder and
 * the monitor have sampled that step: a sample of step k+1 never contains entry k, which belongs to the step that follows.
 * sg_inject supplies the entry "before step 1": a force f(t) is sg_inject(q_0), then the series q_1, q_2, ...  After nsteps
 * entries nothing is added (no refusal, as with a source that has run out).  npts = 0 or nsteps = 0 disarms; re-arming
 * replaces the series and restarts the count; a failed call leaves the previous injectors armed, their count intact.
 * With a communicator a step that added a stress entry sends the traces of s1 again before the next step reads them; a host
 * that drives stages and halo itself does the same after its sg_end_step.  Nothing armed: no extra launch, the same
 * captured graphs. */
/* device-free, like sg_locate_points: cell[k] (or -1) and psi[k][nd] = Mhat^-1 phi(xi_k) / |det J| (0 where -1); degree <= 4 */
int sg_injector_weights(const sg_config* cfg, int64_t npts, const double* pts, int64_t* cell, double* psi);
/* one shot, behind everything the handle has queued: field += amp[npts][ncomp] at the points */
int sg_inject(sg_handle* h, int64_t npts, const double* pts, int what, const double* amp);
/* a series: amp[nsteps][npts][ncomp] */
int sg_set_injectors(sg_handle* h, int64_t npts, const double* pts, int what, int64_t nsteps, const double* amp,
                     int32_t* owned);

/* ---- monitor: L2 norms and elastic energy of the block, taken on the device (the global observer beside the point-wise
 * one; what a harness gets from norm(u) of the downloaded fields, or the oracle's energy test from 1/2 (rho |u|^2 +
 * s : C^-1 : s) of its state) --------------------------------------------------------------------------------------------
 * With Mhat the reference mass matrix of the element and |det J| the cell's Jacobian determinant, every cell c has
 *   Qu_c = sum_i u_i^T Mhat u_i,   Qs_c = sum_ij s_ij^T Mhat s_ij,   Qt_c = t^T Mhat t with t = sum_i s_ii node by node
 * of u = SG_FIELD_U and s = SG_FIELD_S.  A SAMPLE is five doubles { U2, S2, T2, EK, ES }:
 *   U2 = sum_c |det J| Qu_c  (= ||u||^2 in L2; S2, T2 likewise from Qs_c, Qt_c),
 *   EK = sum_c |det J| wk_c Qu_c,   ES = sum_c |det J| (ws_c Qs_c + wt_c Qt_c).
 * The weights w = (wk, ws, wt) are the caller's: one triple for the block (per_cell = 0: w[3]) or one per cell (per_cell
 * = 1: w[ncells][3], host cell order cube * ncls + cls); the library does not derive them from its material state.  The
 * physical choice in dimension d is wk = rho / 2, ws = 1 / (4 mu), wt = -lambda / (4 mu (d lambda + 2 mu)): EK + ES is
 * then the kinetic plus the compliance energy 1/2 s : C^-1 : s, strain = (s - lambda / (d lambda + 2 mu) tr(s) I) / (2 mu).
 * w = NULL: EK = ES = 0.
 * Arithmetic: a form v^T Mhat v is sum_a v_a (Mhat_aa v_a + 2 sum_{b<a} Mhat_ab v_b), b ascending inside a ascending, with
 * fma, in double (FP32 blocks convert every nodal value first).  In symmetric-stress storage only the i <= j lines are
 * read and an off-diagonal form counts twice.  Cells of the layout's padding contribute nothing; ghost traces are no
 * part of a block (a split block measures its own cells).  The lanes of an item are summed by a fixed tree, then
 * SG_MONITOR_CHUNK_ITEMS consecutive items (by item index) in ascending order into one partial, then the partials by one
 * workgroup in a fixed order; no floating-point atomics.  The bits of a sample therefore depend only on the block (shape,
 * kernel family, dtype, storage mode) and the field contents: the same under graph replay and eager launches, for one
 * sg_step(n) and n calls of sg_step(1), for host-driven stages with sg_end_step, with timing on or off.  They are NOT
 * promised equal across partitions: the sum over the blocks of a split equals the single block's to round-off.
 * Arm: a sample after every `every`-th completed step counted from the arming call - through sg_step (graph replay or
 * eager, with or without a communicator) or through sg_end_step after host-driven stages; sample j (0-based) is taken
 * after step (j+1)*every from u1 (time t) and s1 (time t + dt/2); `capacity` >= 1 samples the device buffer holds.  every
 * = 0 disarms; re-arming discards the old samples; a failed call leaves the previous monitor recording, samples intact.
 * sg_step(n) whose samples would exceed the capacity returns SG_ERR_STATE before it queues anything (fields, counters
 * and trace untouched); sg_end_step of a step due a sample the trace has no room for returns SG_ERR_STATE and does not
 * count the step.  No monitor armed: no extra launch, the same captured graphs. */
#define SG_MONITOR_CHUNK_ITEMS 4
/* one sample of the fields as they stand now, after everything the handle has queued */
int sg_measure(sg_handle* h, const double* w, int per_cell, double out[5]);
int sg_set_monitor(sg_handle* h, int64_t every, int64_t capacity, const double* w, int per_cell);
/* samples taken so far -> out[nsamples][5]; nbytes must be that of `capacity` samples (0 with no monitor armed);
 * *nsamples = samples taken */
int sg_get_monitor(sg_handle* h, double* out, size_t nbytes, int64_t* nsamples);

/* ---- correlation: the zero-lag cross-correlation of two handles' fields, cell by cell, accumulated on the device (the
 * observer between the point-wise one and the block-wide one: what imaging and material-gradient loops form from a forward
 * and an adjoint or back-propagated wavefield) ---------------------------------------------------------------------------
 * For two handles a, b of the same shape, with Mhat and |det J| as above, every cell c of the block has
 *   Buu_c = sum_i  a.u_i^T  Mhat b.u_i,
 *   Bss_c = sum_ij a.s_ij^T Mhat b.s_ij,
 *   Btt_c = t_a^T Mhat t_b,   t_x = sum_i x.s_ii node by node,
 *   acc_a[c][k] += w[k] |det J| B_k,c        k = uu, ss, tt
 * of u = SG_FIELD_U and s = SG_FIELD_S of each handle.  acc_a is a device buffer [ncells][3] of doubles owned by a, in host
 * cell order cube * ncls + cls; the first successful sg_correlate allocates and zeroes it.  It is double for FP32 blocks
 * too: every nodal value is converted first.
 * Arithmetic: a form x^T Mhat y is sum_alpha x_alpha r_alpha with r = Mhat y, r_alpha summed over beta ascending and the
 * products over alpha ascending, with fma, from zero for every component.  Components: the velocity's, then the stress's
 * row-major; Buu adds the components' forms in that order, Bss takes fma(mult, form, Bss), then acc = fma(w[k] |det J|,
 * B_k, acc) with the factor rounded once.  Each handle reads (i, j) from the line its own storage mode holds, the mirror
 * (min, max) in symmetric storage; when both handles are symmetric only i <= j is read and an off-diagonal form counts
 * twice (mult = 2), otherwise all d^2 pairs are formed.  The matrix-pipe form (3-D P3 / P4 blocks in the 16-cube layout)
 * computes r with v_mfma_f64_16x16x4_f64 - four beta at a time, the sums inside the instruction in the hardware's own fixed
 * order - and every lane of the four that share a cell sums alpha = 4 m + q over m ascending, q = its lane group; the groups
 * are then added as (q0 + q2) + (q1 + q3).  There is no sum across cells and no atomic: the bits of a cell's result depend
 * only on that cell's nodal values in both handles, the weights, the dtype and the kernel form - not on nbr_mask, the stage
 * kernels of either handle or the order of launches.  Cells of the layout's padding contribute nothing; ghost traces are
 * no part of a block.
 * Handles: b may be a itself.  Otherwise both must be on the same device and agree in dim, degree, cell type and diagonal,
 * dtype, n[], h[] and the layout of their fields (the kernel family's group width); anything else returns SG_ERR_ARG and
 * sg_last_error(a) names the first difference.  nbr_mask, material, sponge, source and storage mode may differ.
 * Ordering: the launch runs on a's stream after everything both handles have queued, and b's stream waits for it: a later
 * sg_step(b) cannot overwrite what is being read.  There is no arming and no graph integration: the caller drives the
 * call between its stepping calls.  By bilinearity B(a, (b^{n+1} - b^n) / dt) is two calls with weights -+ 1/dt.
 * A failed call leaves the accumulator, the fields and both handles untouched. */
int sg_correlate(sg_handle* a, sg_handle* b, const double w[3]);     /* w = NULL: (1, 1, 1) */
/* acc_a -> out[ncells][3]; SG_ERR_STATE before the first successful sg_correlate, SG_ERR_ARG for another nbytes */
int sg_get_correlation(sg_handle* a, double* out, size_t nbytes);
/* zero the accumulator (behind what a has queued); release != 0: free it and the tables with it */
int sg_reset_correlation(sg_handle* a, int release);

/* ---- spectra: running Fourier transforms of the wavefield, accumulated on the device inside the time loop (on-the-fly DFT,
 * Sirgue, Etgen and Albertin 2008: what frequency-domain imaging and inversion built on time-domain modelling keep instead of
 * the forward states; it needs no reverse sweep and works with sources and sponges) ---------------------------------------
 * Armed with nfreq frequencies, `every` and `nsamples`, the handle takes sample j (0-based) after completed step
 * (j + 1) * every counted from the arming call - through sg_step (graph replay or eager, with or without a communicator) and
 * through sg_end_step after host-driven stages alike - behind the receivers' recorder and the monitor and BEFORE the
 * injectors: the sample of step k + 1 never contains injector entry k.  For every word x of a selected field and every
 * frequency f
 *   re[f] = fma(w_re, x, re[f]),   im[f] = fma(w_im, x, im[f]),   (w_re, w_im) = w[j][f]
 * with the caller's table: wu[nsamples][nfreq][2] for the velocity u = SG_FIELD_U (what bit 0, it lives at t) and
 * ws[nsamples][nfreq][2] for the stress s = SG_FIELD_S (bit 1, at t + dt / 2) - the receivers' bits.  The library adds
 * exactly w * field, as the injectors add exactly amp * psi: exp(-i omega t), the quadrature weight every * dt, a taper and
 * the half-step stagger all belong to the caller.  After nsamples samples nothing is added and nothing is refused.
 * Storage: per selected field and frequency two device buffers (re, im) of doubles in the field's own device layout, word
 * ((item * nd + a) * ncomp + c) * gw + lane - double for FP32 blocks too, x is converted first (exactly).  A frequency costs
 * 2 (dim + dim^2) doubles per node.  A word has one writer and there are no atomics: the bits depend only on the field
 * contents and the weights - the same under graph replay and eager launches, for sg_step(n) and n calls of sg_step(1), for
 * host-driven stages, with timing on or off, and on a split block (each block accumulates its own cells).
 * Symmetric-stress storage: only the i <= j lines are accumulated; when the block leaves it (sg_leave_sym, an upload or an
 * injector table that is not symmetric) the stress accumulators' i > j lines are filled from their mirrors and all lines are
 * accumulated from then on.
 * nfreq = 0 disarms and frees; arming again zeroes the accumulators and restarts the count.  A failed call - SG_ERR_ARG: what
 * outside 1..3, nfreq < 0 or > SG_SPECTRA_MAX_FREQ, every < 1, nsamples < 1, no table for a selected field; SG_ERR_NOMEM -
 * leaves the spectra armed before it with accumulators and count intact; all buffers are allocated or none.  The host waits
 * for the handle's stream, as in every setter. */
#define SG_SPECTRA_MAX_FREQ 8
int sg_set_spectra(sg_handle* h, int nfreq, int what, int64_t every, int64_t nsamples, const double* wu, const double* ws);
/* one accumulator -> host[cell][node][comp], the layout of sg_get_field (in symmetric storage the i > j entries from their
 * mirrors); field 0: velocity, 1: stress; part 0: re, 1: im.  SG_ERR_STATE: nothing armed or the field not selected;
 * SG_ERR_ARG: another nbytes, freq outside 0 .. nfreq - 1, another part.  The host waits for the handle's stream. */
int sg_get_spectrum(sg_handle* h, int field, int freq, int part, double* host, size_t nbytes);
/* samples taken so far (0 when nothing is armed) */
int sg_spectra_samples(sg_handle* h, int64_t* taken);
/* The correlation of two handles' spectra, into the accumulator sg_correlate owns (sg_get_correlation / sg_reset_correlation):
 *   acc_a[c][k] += w[k] |det J| Re( z conj(a^_fa) . b^_fb )_k,c      k = uu, ss, tt
 * the forms B_k of sg_correlate taken of frequency fa of a against frequency fb of b.  By bilinearity these are launches of
 * sg_correlate's kernels in double on the accumulators (FP32 blocks too), in this order: (re, re) and (im, im) with weight
 * z_r w, then - unless z = NULL or z[1] == 0, which both mean z = (1, 0) - (re, im) with -z_i w and (im, re) with +z_i w.
 * Handles, ordering and failures as in sg_correlate; both handles must have armed the fields a non-zero weight asks for
 * (w[0]: velocity; w[1], w[2]: stress), else SG_ERR_STATE.  b may be a. */
int sg_correlate_spectra(sg_handle* a, int fa, sg_handle* b, int fb, const double w[3], const double z[2]);
/* The spectra's clock and line list as the library keeps them (device-free).  With `steps` steps completed since arming:
 * out = { step steps + 1 is a sample step (0 / 1), its sample index or -1, some later step is one (0 / 1: "active", the
 * graph cache key), samples taken once `more` further steps are done }. */
int sg_spectra_clock(int64_t every, int64_t nsamples, int64_t steps, int64_t more, int64_t out[4]);
/* the stress lines c = i * dim + j accumulated in full (sym = 0) or symmetric storage, ascending; returns their number */
int sg_spectra_lines(int dim, int sym, int32_t* lines, int max_lines);

/* ---- peak maps: per node the maximum of |u|^2 and of s:s over the samples of a run and the sample that reached it, on the
 * device inside the time loop (the peak-ground-velocity, peak-stress and time-of-peak maps of an elastic-wave run) -----------
 * Armed with `what`, `every` and `nsamples`, the handle takes sample j (0-based) after completed step (j + 1) * every counted
 * from the arming call - through sg_step (graph replay or eager, with or without a communicator) and through sg_end_step
 * after host-driven stages alike.  The hook order at the end of a step is receivers, monitor, spectra, peak maps, injectors:
 * the maps come behind the spectra and BEFORE the injectors, so the sample of step k + 1 never contains injector entry k.
 * For every node of the block and every selected field - the velocity u = SG_FIELD_U (what bit 0, it lives at t), the stress
 * s = SG_FIELD_S (bit 1, at t + dt / 2): the receivers' bits -
 *   every nodal value is converted to double first;
 *   m starts as x_0 * x_0, then m = m + (x_c * x_c) for c ascending, each product and each sum rounded to double on its own
 *   (no fma);
 *   velocity: c = 0 .. dim - 1;  stress in full storage: c = i * dim + j, ascending over all dim^2;  stress in symmetric
 *   storage: the lines of sg_spectra_lines(dim, 1), ascending, an off-diagonal line entering as 2.0 * (x * x) - the doubling
 *   is exact - and the i > j lines are not read;
 *   then  if (m > val) { val = m; idx = j; }  - the comparison is strict, so the earliest sample wins a tie, a NaN never
 *   enters, and a node that never moved keeps idx = -1.
 * numpy restates this to the bit.  After nsamples samples nothing is recorded and nothing is refused.
 * Storage: per selected field val (doubles) and idx (int32) in the field's own device layout with one component, word
 * (item * nd + a) * gw + lane - double / int32 for FP32 blocks too: 12 bytes per node and selected field.  A word has one
 * writer and there are no atomics: the bits depend only on the field contents - the same under graph replay and eager
 * launches, for sg_step(n) and n calls of sg_step(1), for host-driven stages, with timing on or off, and on a split block
 * (each block keeps its own cells).  When the block leaves symmetric storage mid-run val needs no fix-up: from that step on
 * the full-storage formula runs.
 * what: bit 0 velocity (|u|^2), bit 1 stress (s:s) - the receivers' bits; what = 0 disarms and frees.
 * sample j (0-based) after completed step (j + 1) * every counted from the arming call; after nsamples samples nothing
 * is recorded and nothing is refused.  SG_ERR_ARG: what outside 0..3, every < 1, nsamples < 1 or > 2^31 - 1.
 * SG_ERR_NOMEM: all buffers are allocated or none.  Arming again zeroes the maps (val = 0.0, idx = -1) and restarts the
 * count.  A failed call leaves the maps armed before it, their values and the count intact.  The host waits for the handle's
 * stream, as in every setter. */
int sg_set_peaks(sg_handle* h, int what, int64_t every, int64_t nsamples);
/* field 0: velocity, 1: stress -> value[ncells][nd] (the maxima of the SQUARES) and sample[ncells][nd] (-1: never above 0),
 * cells in the order of sg_get_field, the cubes of the layout's padding dropped; either pointer may be NULL; nvalues must be
 * ncells * nd, else SG_ERR_ARG.  SG_ERR_STATE: nothing armed or the field not selected.  The host waits for the handle's
 * stream. */
int sg_get_peaks(sg_handle* h, int field, double* value, int32_t* sample, size_t nvalues);
/* the same into the caller's device buffers on the handle's stream, queued only; dtype of the values as in sg_get_field_dev
 * (0: double, 1: float, rounded once); the samples are int32 */
int sg_get_peaks_dev(sg_handle* h, int field, void* dev_value, int dtype, int32_t* dev_sample, size_t nvalues);
/* samples taken so far (0 when nothing is armed) */
int sg_peaks_samples(sg_handle* h, int64_t* taken);

/* un-fused operators for stage-level parity tests:
 *   out = Minv f(w; s_in, u_abs)   (elastic.py:204-209 + :358-367)
 *   out = Minv g(v; u_in)          (elastic.py:211-219 + :358-367)
 * `use_source` adds the current step's source to g. */
int sg_apply_F(sg_handle* h, int s_in, int u_abs, int u_out);
int sg_apply_G(sg_handle* h, int u_in, int s_out, int use_source);

/* ---- halo layer (replaces PyOP2's implicit halo exchange, elastic.py:404-436) ------- */
/* Facet traces of `field` on block side `side` (2*axis + hi), packed as
 * [facet][facet-node][dim]: the velocity components, or for a stress field the column
 * T_i,axis (i < dim) - on an axis-aligned block side the only part of the neighbour's tensor that
 * enters `avg(s0)*n` (elastic.py:206; SURVEY 8e "send T.n").  Written to the DEVICE buffer
 * `dev_out` (caller-allocated, e.g. a torch tensor). */
int sg_halo_bytes(const sg_handle* h, int field, int side, size_t* nbytes);
int sg_halo_pack(sg_handle* h, int field, int side, void* dev_out);
/* register the DEVICE buffer holding the neighbour block's packed traces of
 * `field` for `side`; read by the next stages that consume `field`. */
/* the same for several sides in ONE launch: dev_out[side] = send buffer of that side or NULL, 6 entries */
int sg_halo_pack_sides(sg_handle* h, int field, void* const* dev_out);
int sg_halo_attach(sg_handle* h, int field, int side, const void* dev_in);
/* ---- native exchange over RCCL (csrc/comm.cpp) --------------------------------------------
 * The reference's halo exchange is implicit in every assemble (elastic.py:364; set-up :404-436).  With a
 * communicator attached, sg_step on a block with neighbours runs the whole pipelined schedule itself - per stage
 * FIRST, pack, grouped ncclSend/ncclRecv with the face neighbours on the handle's stream, SECOND beside them -
 * for all six stages of all `nsteps` steps without returning to the caller; the handle owns the send / receive
 * buffers.  One process per GPU: every rank of the block grid calls sg_comm_init (collective) with the SAME unique
 * id - made by one rank with sg_comm_get_unique_id and distributed by whatever the host has (MPI_Bcast in the
 * reference's world, torch.distributed here) - its rank, the number of ranks, and per block side the rank of the
 * face neighbour (-1: none; must agree with sg_config::nbr_mask). */
#define SG_COMM_ID_BYTES 128
typedef struct sg_comm_stats {
  int64_t exchanges;        /* grouped send/receive calls issued */
  int64_t bytes_sent;       /* bytes handed to RCCL */
  double exposed_wait_ms;   /* timing enabled: time the receives lasted beyond the SECOND launch beside them */
} sg_comm_stats_t;
int sg_comm_get_unique_id(void* id, size_t nbytes);
int sg_comm_init(sg_handle* h, const void* id, size_t nbytes, int rank, int nranks, const int32_t* peers);
/* RCCL is bound at run time, on first use: the copy already in the process (torch brings its own) or the system's
 * librccl.so - or the one file the environment variable SEIGEN_RCCL_LIB names (a site's own build; the transport
 * double of tests/fake_rccl) - and must report the major version of the rccl.h this library was compiled against;
 * SG_ERR_STATE where there is none or the wrong one (single blocks and the device-free entry points do not need it).
 * sg_comm_version: its version as RCCL encodes it (e.g. 22707).  sg_comm_library: the path of the shared object the
 * bound entry points come from, NUL-terminated into buf[n] - which MPI / which RCCL moved the traces is part of a
 * run's record (the reference prints its MPI through PyOP2's configuration, tests/tiling/utils.py:143-144 timers). */
int sg_comm_version(int* version);
int sg_comm_library(char* buf, size_t n);
/* Everything sg_comm_init can refuse WITHOUT another rank (RCCL present, rank / nranks, peers[] against
 * sg_config::nbr_mask; two sides may share a peer only as the two ends of one axis).  Hosts call it on every rank and
 * agree on the result BEFORE the collective sg_comm_init: a rank that failed alone would leave the others waiting. */
int sg_comm_check(sg_handle* h, int rank, int nranks, const int32_t* peers);
/* Collective self-test of the exchange, after sg_comm_init: every rank sends a pattern naming (rank, side, position)
 * from each send buffer and counts the values that did not arrive from the FACING side of the right neighbour
 * (0 = every side receives its neighbour's trace; the role of a halo-exchange consistency check before a run).
 * Receives are posted in the order of the facing sides, so two faces between the same pair of ranks - a block that is
 * its own neighbour across an axis - are paired correctly, not mirrored. */
int sg_comm_selftest(sg_handle* h, int64_t* mismatches);   /* SG_ERR_STATE once traces have been exchanged: it overwrites the ghost buffers */
int sg_comm_finalize(sg_handle* h);
int sg_comm_get_stats(sg_handle* h, sg_comm_stats_t* out, int reset);
/* one exchange of `field`'s traces on its own (tests), and the device addresses of a side's buffers */
int sg_comm_exchange(sg_handle* h, int field);
int sg_comm_buffers(sg_handle* h, int kind, int side, void** send, void** recv, size_t* nbytes);

/* Symmetric-stress storage is left automatically when THIS block is handed a
 * non-symmetric stress or source; blocks of one mesh must agree, so the host layer reads the
 * state of every block (sg_get_sym) and makes all of them leave together (sg_leave_sym). */
int sg_get_sym(const sg_handle* h, int* sym);
int sg_leave_sym(sg_handle* h);

/* ---- instrumentation --------------------------------------------------------------- */
int sg_enable_timing(sg_handle* h, int on);
int sg_get_counters(sg_handle* h, sg_counters_t* out);
/* ms of the last sg_step call measured with hipEvents on the launch stream */
int sg_last_step_ms(sg_handle* h, double* ms);
/* Name of the kernel a launch of `stage` over `region` runs on this handle, as rocprofv3 --kernel-trace prints it
 * (e.g. "void sg::mfma_stage_G<double, 4, 0, 1, 1>(sg::StageArgs)"), NUL-terminated into buf[n] (truncated if longer).
 * Launches, allocates and uploads nothing: the name is that of the kernel handle picked by the same choice a launch makes
 * from the handle's state, so profiles and bench.py's `roofline.kernel` name what actually runs - the role of PyOP2's per-parloop kernel names in the reference's
 * timing summaries (tests/tiling/utils.py:143-144 [upstream get_timers]).  Blocks with neighbours: after sg_halo_attach /
 * sg_comm_init (the choice depends on the attached halo buffers). */
int sg_stage_kernel_name(sg_handle* h, int stage, int region, char* buf, size_t n);

/* ---- device-free setup queries (host logic; usable without a GPU) ------------------------ */
/* Reference-element operators of equispaced Lagrange P_degree on the dim-simplex
 * (what `assemble(..., inverse=True)`, elastic.py:376-382, and the generated
 * element kernels tabulate [upstream]).  which = 0: D[r][a][b] = (Mhat^-1 Shat_r)
 * (dim*nd*nd), 1: L[f][a][b'] facet lifts (nfaces*nd*nf), 2: Mhat (nd*nd),
 * 3: sponge tensor A[a][c][b] for a DG_q sigma (nd*nq*nd), 4: facet node lists
 * fnode[f][b'] as doubles (nfaces*nf).  out = NULL: size query.
 * Returns the number of doubles or a negative error. */
int64_t sg_reference_operator(int dim, int degree, int which, int q, double* out, size_t nbytes);
/* phi[p][a]: Lagrange basis of P_degree (degree <= 8) at reference points xi[p][dim] - the
 * tabulation behind Function evaluation / the error functional of eigenmode_2d.py:49-63. */
int sg_tabulate(int dim, int degree, int64_t npts, const double* xi, double* phi);
/* The same two for a cell type: 0 = simplex (the functions above), 1 = tensor-product cell (the unit square / cube,
 * (degree+1)^dim equispaced nodes with the first coordinate fastest; facet 2m: x_m = 0, facet 2m+1: x_m = 1) -
 * the element of sg_config::diagonal = 2. */
int64_t sg_reference_operator_cell(int cell_type, int dim, int degree, int which, int q, double* out, size_t nbytes);
int sg_tabulate_cell(int cell_type, int dim, int degree, int64_t npts, const double* xi, double* phi);
/* dphi[p][a][r] = d(phi_a)/d(xi_r) at xi[p][dim] (degree <= 8): the derivative of the interpolant's basis, the tables of
 * sg_get_gradient_dev - not which = 0 of sg_reference_operator, the weak operator with the derivative on the test function. */
int sg_tabulate_grad_cell(int cell_type, int dim, int degree, int64_t npts, const double* xi, double* dphi);
/* Point location (device-free; cfg->device / stream ignored, like sg_block_node_coords): cell[k] = the block-local cell
 * owning pts[k][dim], or -1 (another block's, or outside the mesh); xi[k][dim] its reference coordinates (0 where -1).
 * The rule (seigen_amd/functionspace.py locate, the stand-in for the point location behind vtktools.vtu.ProbeData that
 * tests/explosive_source/uy.py:36-43 relies on): per axis t = (p - origin) / h; the cube floor(t) and, on a grid line
 * (|t - round t| < 1e-9), also the one below it if its index in the MESH (cube0 + local) is >= 0; candidates in ascending
 * order (z slowest), classes in ascending order; the first cell whose reference coordinates pass xi >= -1e-12 and
 * sum xi <= 1 + 1e-12 (tensor-product cells: max xi) wins - on a grid line the lower cube, the lower side of a
 * discontinuous field. */
int sg_locate_points(const sg_config* cfg, int64_t npts, const double* pts, int64_t* cell, double* xi);
/* The disjoint boxes of cubes {origin[3], extent[3]} a region of a split stage covers in the block
 * `cfg` describes (n, dim, nbr_mask); returns their number (at most SG_MAX_REGION_BOXES; a stage
 * launch carries that many), writes the first `max_boxes` of them to boxes[][6]. */
#define SG_MAX_REGION_BOXES 7
int sg_region_boxes(const sg_config* cfg, int region, int32_t* boxes, int max_boxes);
/* Translation-invariant neighbour tables of the structured simplicial mesh:
 * nb [cls][face][5] = {axis crossed (-1: same cube), direction, neighbour class,
 * neighbour facet, ordinal on the cube side}; nb_node [cls][face][nf] neighbour
 * element node matching each facet node; cn [cls][face][3] = |F|/|detJ| * outward
 * normal; jinv [cls][3][3]. */
int sg_mesh_tables(int dim, int degree, int diagonal, const double* h, int32_t* nb, int32_t* nb_node, double* cn,
                   double* jinv);

#ifdef __cplusplus
}
#endif
#endif /* SEIGEN_HIP_H */
