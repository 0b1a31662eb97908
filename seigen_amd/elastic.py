"""`ElasticLF4` - the solver-class API of ``seigen/elastic.py`` on MI355X.

Drop-in for the explicit path of the reference: same factory
(``ElasticLF4.create``, ``seigen/elastic.py:27-64``), same plain attributes
(``density dt mu l``), same ``absorption`` / ``source`` properties whose setters
interpolate an ``Expression`` into a pre-assigned ``Function`` (``:126-154``),
same ten named fields (``:93-103``) and the same ``run(T)`` loop (``:267-315``).
What Firedrake/PyOP2 generated and ran on CPU per timestep - eight assembles,
eight inverse-mass mat-vecs, two copies, halo exchanges - is six fused HIP
launches in libseigen_hip.so, driven through ctypes (include/seigen_hip.h).

Differences, all documented in DESIGN.md:
  * ``uh2`` and ``sh2`` are never materialised (fused into the combine stages);
    ``u0``/``u1`` (``s0``/``s1``) share one device buffer because
    ``u0.assign(u1)`` (``:296``) is an in-place update.
  * ``utemp`` has one consumer, ``sh2 = g(utemp)`` in the stress update ``s1 = s0 + dt sh1 + dt^3/24 sh2`` (``:302-303``),
    and ``g`` is linear: the library leaves ``w = dt u1 + dt^3/24 utemp`` in the buffer behind ``uh1`` / ``utemp`` and
    computes ``s1 = s0 + g(w)`` - one application of ``g`` that reads neither ``sh1`` nor a second right-hand side
    (include/seigen_hip.h, ``enum sg_stage``).  After a step ``elastic.utemp`` therefore holds ``w``; ``(u1, s1)`` are
    unchanged to round-off.
  * ``solver='implicit'`` (``:318-332``): the reference hands every form to a PETSc KSP; all eight
    systems are DG mass matrices (block diagonal), so the solve IS the element-wise inverse the
    explicit path applies, up to the KSP tolerance.  Here it runs the same six launches with the
    implicit forms' density convention (``form_u1``, ``:175-178``: u1 = u0 + (...)/rho).
  * VTK output (``:221-232``): ``velocity_<k>.vtu`` / ``stress_<k>.vtu`` streams with ``.pvd`` indices
    (``seigen_amd/vtu.py``; ``SEIGEN_OUTPUT=npy`` writes raw arrays instead).
  * The halo exchange implicit in every assemble (``:364``, ``:404-436``) runs inside the library over RCCL
    (``NativeExchanger``), or stage by stage from ``seigen_amd/parallel.py`` for process groups without device transport.
"""
import os
import sys
from contextlib import contextmanager

import numpy as np

from . import _lib
from .backend import HipBlock
from .functionspace import Function, FunctionSpace, TensorFunctionSpace, VectorFunctionSpace
from .helpers import log, allreduce_sum, allreduce_sum_array
from .parallel import world, HaloExchanger, NativeExchanger
from .profiling import timed_region

_SOLVER_MODES = ("implicit", "explicit", "parloop", "fusion", "tiling", "hip")


def monitor_weights(dim, density, mu, l, ncells):
    """The weights (wk, ws, wt) that make the monitor's EK + ES the kinetic plus the compliance energy 1/2 s : C^-1 : s
    (include/seigen_hip.h): wk = rho / 2, ws = 1 / (4 mu), wt = -lambda / (4 mu (d lambda + 2 mu)).  Floats: one triple
    [3]; any of the three one value per cell: [ncells, 3]."""
    rho, mu, lam = (np.atleast_1d(np.asarray(a, dtype=np.float64)).ravel() for a in (density, mu, l))
    per_cell = max(rho.size, mu.size, lam.size) > 1
    if per_cell:
        rho, mu, lam = (np.broadcast_to(a, (int(ncells),)) for a in (rho, mu, lam))
    w = np.stack([rho / 2.0, 1.0 / (4.0 * mu), -lam / (4.0 * mu * (dim * lam + 2.0 * mu))], axis=-1)
    return np.ascontiguousarray(w if per_cell else w[0])


def sensitivity(dim, density, lam, mu, corr):
    """The derivatives of rho * uu + alpha * ss + beta * tt with respect to rho, lambda and mu at fixed correlations
    corr = {"uu", "ss", "tt"} (ElasticLF4.correlation), where alpha = 1 / (2 mu) and beta = -lambda / (2 mu (d lambda +
    2 mu)) make alpha s:s' + beta tr s tr s' the compliance form s : C^-1 : s' (twice the monitor's ws, wt):
      K_rho = uu,   K_lambda = -tt / (d lambda + 2 mu)^2,
      K_mu = -ss / (2 mu^2) + lambda (d lambda + 4 mu) / (2 mu^2 (d lambda + 2 mu)^2) tt.
    Floats or one value per cell; returns {"rho", "lambda", "mu"}, each of the correlations' shape.
    The gradient of a misfit J = 1/2 sum_k |R u_k - obs_k|^2 is dJ/dm = -1/2 K_m when the correlations are those of the
    ADJOINT state MID-STEP against the forward step's INCREMENT (DESIGN.md "Correlation"): the
    adjoint solver (-dt, residuals (2 / rho_cell) r_k injected in reversed order) after its velocity half - stages UH1,
    STEMP, U1 - correlated with weights (+1, +1, +1) against the forward step's own result and, after `rewind(1)`, with
    (-1, -1, -1) against the state the step started from.  dJ/drho is then exact (3e-11 .. 4e-10 of the largest entry against
    central differences, the differences' floor; 2e-10 .. 6e-10 through device runs), dJ/dlambda and dJ/dmu second order in
    dt (8.0e-4 and 9.8e-4 at dt = 1/320 on the 4 x 4 P2 case); half a step off costs 4 .. 69 % (tests/test_gradient_oracle.py,
    tests/test_gradient_gpu.py).  The zero-lag product of the two states is an imaging condition, no gradient."""
    lam, mu = np.asarray(lam, dtype=np.float64), np.asarray(mu, dtype=np.float64)
    uu, ss, tt = (np.asarray(corr[k], dtype=np.float64) for k in ("uu", "ss", "tt"))
    k = dim * lam + 2.0 * mu
    return {"rho": uu + 0.0 * np.asarray(density, dtype=np.float64),
            "lambda": -tt / k ** 2,
            "mu": -ss / (2.0 * mu ** 2) + lam * (dim * lam + 4.0 * mu) / (2.0 * mu ** 2 * k ** 2) * tt}


def spectra_weights(freqs, dt, every, nsamples, t0=0.0, stagger=0.0, window=None):
    """The complex weights [nsamples, nfreq, 2] = (re, im) of a running Fourier transform (sg_set_spectra) by the rectangle
    rule: w[j][f] = every * dt * window[j] * exp(-2 pi i freqs[f] t_j) at the sample times t_j = t0 + (j + 1) * every * dt +
    stagger - stagger = dt / 2 for the stress, which lives half a step behind the velocity.  window: [nsamples] (a taper),
    None = 1.  The library adds exactly w * field; everything else is decided here."""
    freqs = np.atleast_1d(np.asarray(freqs, dtype=np.float64)).ravel()
    nsamples, every = int(nsamples), int(every)
    if every < 1 or nsamples < 0:
        raise ValueError("spectra_weights needs every >= 1 and nsamples >= 0")
    win = np.ones(nsamples) if window is None else np.asarray(window, dtype=np.float64).ravel()
    if win.shape != (nsamples,):
        raise ValueError("the window holds one value per sample (%d), not %r" % (nsamples, win.shape))
    t = float(t0) + (np.arange(nsamples) + 1.0) * every * float(dt) + float(stagger)
    w = (every * float(dt)) * win[:, None] * np.exp(-2j * np.pi * freqs[None, :] * t[:, None])
    return np.ascontiguousarray(np.stack([w.real, w.imag], axis=-1))


def _device_for_rank():
    if "SEIGEN_HIP_DEVICE" in os.environ:
        return int(os.environ["SEIGEN_HIP_DEVICE"])
    if world()[1] > 1:
        return int(os.environ.get("LOCAL_RANK", "0"))
    return 0


def fibre_points(dim, p0, p1, nchannels, gauge_length, nq=4):
    """(points [nchannels * nq, dim], unit tangent [dim], weights [nq]) of a straight fibre from p0 to p1: `nchannels` channel
    centres at equal spacing (the first at p0, the last at p1; one channel: the midpoint), per channel the `nq` Gauss-Legendre
    points of the gauge length about its centre; the weights sum to one (an average)."""
    p0 = np.asarray(p0, dtype=np.float64).reshape(dim)
    p1 = np.asarray(p1, dtype=np.float64).reshape(dim)
    length = float(np.linalg.norm(p1 - p0))
    if not length > 0.0 or int(nchannels) < 1 or int(nq) < 1 or not float(gauge_length) >= 0.0:
        raise ValueError("a fibre needs p0 != p1, nchannels >= 1, nq >= 1 and gauge_length >= 0")
    t = (p1 - p0) / length
    x, w = np.polynomial.legendre.leggauss(int(nq))
    centres = np.array([0.5]) if int(nchannels) == 1 else np.linspace(0.0, 1.0, int(nchannels))
    s = centres[:, None] * length + 0.5 * float(gauge_length) * x[None, :]
    return (p0[None, None, :] + s[:, :, None] * t[None, None, :]).reshape(-1, dim), t, 0.5 * w


def fibre_combine(t, w, nchannels, nq, eps):
    """the channels' axial strain rate [n, nchannels] from the strain-rate traces eps [n, nchannels * nq, dim, dim] at
    fibre_points: t . eps . t at every point, averaged with the weights over each channel's points"""
    axial = np.einsum("i,npij,j->np", t, eps, t).reshape(eps.shape[0], int(nchannels), int(nq))
    return axial @ w


class ElasticLF4(object):
    r"""Elastic wave equation, DG in space, fourth-order leap-frog in time.
    Create with ``ElasticLF4.create(mesh, family, degree, dimension, solver)``."""

    @staticmethod
    def create(mesh, family, degree, dimension, solver="explicit", output=True, dtype="f64"):
        """Same signature and solver strings as ``seigen/elastic.py:27-64``; every
        explicit mode ('explicit', 'parloop', 'fusion', 'tiling', and the alias
        'hip') runs the fused HIP path.  ``dtype`` (not in the reference, which is double
        throughout, ``:442``): 'f64', or 'f32' for the FP32 second mode (3-D blocks)."""
        if solver == "implicit":
            return ImplicitElasticLF4(mesh, family, degree, dimension, output=output, dtype=dtype)
        elif solver in ("explicit", "hip"):
            return ExplicitElasticLF4(mesh, family, degree, dimension, output=output, dtype=dtype)
        elif solver == "parloop":
            return TilingElasticLF4(mesh, family, degree, dimension, output=output, dtype=dtype, tiling_mode=None)
        elif solver == "fusion":
            return TilingElasticLF4(mesh, family, degree, dimension, output=output, dtype=dtype, tiling_mode="hard")
        elif solver == "tiling":
            return TilingElasticLF4(mesh, family, degree, dimension, output=output, dtype=dtype, tiling_mode="tile")
        else:
            raise ValueError("Unknown solver mode. Must be one of: implicit, explicit, parloop")

    def __init__(self, mesh, family, degree, dimension, output=True, dtype="f64"):
        self.dtype = dtype
        with timed_region('function setup'):
            if dimension != mesh.dim:
                raise ValueError("dimension=%r does not match the mesh (%d-D)" % (dimension, mesh.dim))
            if not (1 <= int(degree) <= 4):
                raise ValueError("degree must be 1..4")
            self.mesh = mesh
            self.dimension = dimension
            self.degree = int(degree)
            self.output = output

            self.S = TensorFunctionSpace(mesh, family, degree, name='S')
            self.U = VectorFunctionSpace(mesh, family, degree, name='U')

            # Assumes that the S and U function spaces are the same.
            dofs = allreduce_sum(self.S.dof_count)
            log("Number of degrees of freedom: %d" % dofs)

            self._block = self._create_block()

            def bound(space, name, field):
                f = Function(space, name=name)
                if field is not None:
                    f._bind(self._block, field)
                return f

            self.s0 = bound(self.S, "StressOld", _lib.FIELD_S)
            self.sh1 = bound(self.S, "StressHalf1", _lib.FIELD_SH)
            self.stemp = bound(self.S, "StressTemp", _lib.FIELD_SH)
            self.sh2 = bound(self.S, "StressHalf2", None)       # fused away, never materialised
            self.s1 = bound(self.S, "StressNew", _lib.FIELD_S)

            self.u0 = bound(self.U, "VelocityOld", _lib.FIELD_U)
            self.uh1 = bound(self.U, "VelocityHalf1", _lib.FIELD_UH)
            self.utemp = bound(self.U, "VelocityTemp", _lib.FIELD_UH)
            self.uh2 = bound(self.U, "VelocityHalf2", None)      # fused away
            self.u1 = bound(self.U, "VelocityNew", _lib.FIELD_U)

            self.absorption_function = None
            self.source_function = None
            self.source_expression = None
            # Separable source S(x, t) = w(t) * source_function(x): when set (a callable t -> float),
            # `source_function` holds the spatial pattern and is NOT re-interpolated from
            # `source_expression`.  Build-defined (the reference only knows re-interpolated Expressions,
            # elastic.py:285-288): lets a harness use a pattern that is not a nodal interpolant, e.g.
            # the L2 projection of the source box (harness/explosive_source.py, source_mode).
            self.source_time_function = None
            self.density = None
            # False: the explicit reference's update u1 = rho*u0 + dt*uh1 + dt^3/24*uh2 (only rhs(form_u1)
            # is kept, elastic.py:341-345, :354-356); True: u1 = u0 + (...)/rho, what the implicit form
            # solves (elastic.py:175-178).  Identical for rho = 1, which every reference test uses.
            self.density_physical = False
            self.dt = None
            self.mu = None
            self.l = None

            self.invmass_velocity = None
            self.invmass_stress = None
            self._exchanger = None
            self._step_index = 0
            self._receivers = None          # (points, every, what) of set_receivers
            self._receiver_times = []
            self._gauges = None             # (points, every, kind, capacity) of set_gauges
            self._gauge_times = []
            self._fibre = None              # (tangent, weights, nchannels, nq) of set_fibre
            self._monitor = None            # `every` of set_monitor
            self._monitor_times = []
            self._spectra = None            # (freqs, every, nsamples, what, window) of set_spectra
            self._spectra_freqs = None      # the frequencies armed by the last run
            self._peaks = None              # (what, every, nsamples) of set_peaks
            self._peaks_armed = None        # (what, every) armed by the last run
            self._frames = None             # (function, m, slice, every, dtype) of set_frames
            self._frame_stack = None        # the frames of the last run
            self._injected = []             # what inject / set_injectors have added, for rewind (see _position)
            self._armed = None              # the armed series' entries still to be logged
            self._rewound = 0               # steps re-wound so far

        if self.output:
            with timed_region('i/o'):
                # File("velocity.pvd") / File("stress.pvd") of the reference (elastic.py:117-124);
                # SEIGEN_OUTPUT=npy writes raw arrays instead
                from .vtu import VtuStream
                rank, nranks = world()
                self.u_stream = VtuStream("velocity", rank, nranks)
                self.s_stream = VtuStream("stress", rank, nranks)

    # ---- device block ---------------------------------------------------------------------
    def _create_block(self):
        part = self.mesh.partition
        # the mesh's origin + the block's integer offset: coordinates bitwise those of the unpartitioned mesh
        block = HipBlock(self.mesh.dim, self.degree, part.n, self.mesh.h, list(self.mesh.origin),
                         "quadrilateral" if self.mesh.quadrilateral else self.mesh.diagonal,
                         part.nbr_mask, device=_device_for_rank(), dtype=self.dtype, cube0=list(part.start))
        self._torch_stream = None
        if part.world > 1:
            # One process per GPU: the library's launch stream, wrapped for torch, is made current
            # around every torch.distributed call (seigen_amd/parallel.py), so packs, exchanges and
            # the boundary launches are ordered on it.
            import torch
            if torch.cuda.is_available():
                torch.cuda.set_device(_device_for_rank())
                self._torch_stream = torch.cuda.ExternalStream(block.stream_ptr(), device=_device_for_rank())
        return block

    @property
    def block(self):
        return self._block

    # ---- absorption / source (elastic.py:126-154) -----------------------------------------------
    @property
    def absorption(self):
        r"""The absorption coefficient :math:`\sigma` of the term :math:`\sigma\mathbf{u}`."""
        return self.absorption_function

    @absorption.setter
    def absorption(self, expression):
        self.absorption_function.interpolate(expression)

    @property
    def source(self):
        r"""The source term on the RHS of the stress equation."""
        return self.source_function

    @source.setter
    def source(self, expression):
        self.source_function.interpolate(expression)

    # ---- stage descriptors in place of the UFL forms (elastic.py:156-202) ------------------------
    form_uh1 = property(lambda self: ("uh1", _lib.STAGE_UH1))
    form_stemp = property(lambda self: ("stemp", _lib.STAGE_STEMP))
    form_uh2 = property(lambda self: ("uh2+u1", _lib.STAGE_U1))
    form_u1 = property(lambda self: ("uh2+u1", _lib.STAGE_U1))
    form_sh1 = property(lambda self: ("sh1", _lib.STAGE_SH1))
    form_utemp = property(lambda self: ("utemp", _lib.STAGE_UTEMP))
    form_sh2 = property(lambda self: ("sh2+s1", _lib.STAGE_S1))
    form_s1 = property(lambda self: ("sh2+s1", _lib.STAGE_S1))

    def write(self, u=None, s=None):
        r"""Write the velocity and/or stress fields (``seigen/elastic.py:221-232``): numbered
        ``.vtu`` files with point data named like the function (``VelocityNew``, ``StressNew``) and
        a ``.pvd`` index, as the reference's VTK streams; raw ``.npy`` with ``SEIGEN_OUTPUT=npy``."""
        if self.output:
            with timed_region('i/o'):
                if os.environ.get("SEIGEN_OUTPUT", "vtu") == "npy":
                    rank = world()[0]
                    if u:
                        np.save("velocity_%d_r%d.npy" % (self._step_index, rank), u.dat.data)
                    if s:
                        np.save("stress_%d_r%d.npy" % (self._step_index, rank), s.dat.data)
                    return
                if u:
                    self.u_stream.write(u, self._step_index * (self.dt or 0.0))
                if s:
                    self.s_stream.write(s, self._step_index * (self.dt or 0.0))

    def create_solver(self, form, result=None):
        """Solver context of one stage = its fused-launch id (``elastic.py:354-356``)."""
        return form[1]

    def solve(self, ctx, matrix=None, result=None):
        """Run one fused stage on the device (``elastic.py:358-367``).  The combine
        stages are fused into ``uh2``/``sh2``, so their contexts launch nothing new."""
        self._block.run_stage(ctx)

    def setup(self):
        """Upload parameters, sponge and source; stage contexts (``elastic.py:244-255``,
        ``:369-385`` - the inverse mass is folded into the reference operators)."""
        log("Creating solver contexts")
        with timed_region('solver setup'):
            for name in ("density", "dt", "mu", "l"):
                if getattr(self, name) is None:
                    raise ValueError("ElasticLF4.%s must be set before run()" % name)
            # density, l, mu: floats as in the reference's tests, or one value per cell of this
            # rank's block (build-defined heterogeneous extension)
            self._upload_params(self.dt)
            if self.absorption_function is not None:
                self._block.set_absorption(self.absorption_function.dat.data_cells,
                                           self.absorption_function.function_space().degree)
            else:
                self._block.set_absorption(None, 0)
            self.ctx_uh1 = self.create_solver(self.form_uh1, self.uh1)
            self.ctx_stemp = self.create_solver(self.form_stemp, self.stemp)
            self.ctx_uh2 = self.create_solver(self.form_uh2, self.uh2)
            self.ctx_u1 = self.create_solver(self.form_u1, self.u1)
            self.ctx_sh1 = self.create_solver(self.form_sh1, self.sh1)
            self.ctx_utemp = self.create_solver(self.form_utemp, self.utemp)
            self.ctx_sh2 = self.create_solver(self.form_sh2, self.sh2)
            self.ctx_s1 = self.create_solver(self.form_s1, self.s1)
            if self.mesh.partition.world > 1 and self._exchanger is None:
                import torch
                dev = torch.device("cuda", _device_for_rank())
                import torch.distributed as dist
                # SEIGEN_HALO_NATIVE: "1" (default) = inside the library when the process group is RCCL's; "0" = never;
                # "force" = also under a process group without device transport (gloo, MPI): the library makes its
                # own RCCL communicator, the group only carries the unique id and the ranks' agreement
                want = os.environ.get("SEIGEN_HALO_NATIVE", "1")
                native = (want == "force" or (dist.get_backend() == "nccl" and want != "0")) \
                    and os.environ.get("SEIGEN_HALO_SCHEDULE", "pipelined") != "plain"
                if native:      # the exchange inside the library: one C-ABI call per run of steps (csrc/comm.cpp)
                    # every rank must end up on the same path: agree on whether the communicator came up everywhere
                    try:
                        ex, failed = NativeExchanger(self._block, self.mesh.partition), 0
                    except Exception as e:      # noqa: BLE001 - whatever it was, the host-driven exchanger still works
                        ex, failed = None, 1
                        log("native halo exchange unavailable on this rank (%r): falling back to the host-driven one" % (e,))
                    if allreduce_sum(failed) > 0:
                        if ex is not None:
                            self._block.comm_finalize()
                        native = False
                    else:
                        self._exchanger = ex
                if not native:  # driven from here stage by stage (gloo / host-staged transports, the plain schedule)
                    self._exchanger = HaloExchanger(self._block, self.mesh.partition, dev, stream=self._torch_stream)

    def _upload_params(self, dt):
        rho = np.atleast_1d(np.asarray(self.density, dtype=np.float64)).ravel()
        self._block.set_params(float(rho[0]), dt, self.l, self.mu)
        if rho.size > 1 or self.density_physical:
            self._block.set_density(rho if rho.size > 1 else float(rho[0]), self.density_physical)

    @property
    def loop_context(self):
        @contextmanager
        def empty_loop_context():
            yield
        return empty_loop_context

    # ---- source handling -----------------------------------------------------------------------
    # a support this large means the source is not the localised kind the sparse table is meant for
    SOURCE_TABLE_MAX_BYTES = 2 << 30

    def _source_table(self, times):
        """Sparse source values: (nodes, values[nsteps or 1, nnz, d, d], static).

        The reference re-interpolates ``source_expression`` into ``source_function``
        at every step (``elastic.py:285-288``).  The same nodal values are computed
        here for all steps up front, but only on the support of the source, and uploaded
        once.  The support is found with ``t`` treated as unknown
        (``Expression.support_mask``): every node where the expression can be non-zero at
        ANY time - a time-windowed source is not missed, a source whose position depends on
        ``t`` gets the whole region it can reach.  A source without ``t`` is one time slice."""
        expr = self.source_expression
        nsteps = len(times)
        d = self.dimension
        if self.source_time_function is not None:
            vals = self.source_function.dat.data_cells
            nz = np.nonzero(np.abs(vals).reshape(vals.shape[0] * vals.shape[1], -1).max(axis=1) > 0)[0]
            v = vals.reshape(-1, d, d)[nz]
            w = np.array([float(self.source_time_function(t)) for t in times])
            return nz, w[:, None, None, None] * v[None], False
        if expr is None or not hasattr(expr, "_params") or "t" not in expr._params:
            vals = self.source_function.dat.data_cells
            nz = np.nonzero(np.abs(vals).reshape(vals.shape[0] * vals.shape[1], -1).max(axis=1) > 0)[0]
            v = vals.reshape(-1, d, d)[nz]
            return nz, v[None], True
        t_keep = expr.t
        nz, Xs = [], []
        for cell0, X, cells in self._support_scan_chunks(expr):
            idx = np.nonzero(expr.support_mask(X).reshape(-1))[0]
            if cells is None:
                nz.append(idx + cell0 * X.shape[1])
            else:                                         # a sub-box of the block: rows of X are the cells `cells`
                nz.append(cells[idx // X.shape[1]] * X.shape[1] + idx % X.shape[1])
            Xs.append(X.reshape(-1, X.shape[-1])[idx])
        nz, Xs = np.concatenate(nz), np.concatenate(Xs)
        if nsteps * len(nz) * d * d * 8 > self.SOURCE_TABLE_MAX_BYTES:
            raise MemoryError("the source can be non-zero at %d nodes over %d steps: its table would take %.1f GB; "
                              "too much for a per-step table, and the source does not factorise into w(t) * pattern(x)"
                              % (len(nz), nsteps, nsteps * len(nz) * d * d * 8 / 1e9))
        values = expr.evaluate_times(Xs, times).reshape(nsteps, len(nz), d, d)
        expr.t = t_keep
        return nz, values, False

    def _support_scan_chunks(self, expr):
        """Node coordinates to search for the support of a source: the whole block slab by slab (bounded host
        memory), or - when the expression carries a hint `support_box = (lo, hi)`, the caller's promise that it
        vanishes outside that box - only the cubes of this rank's block that touch the box (a 128^3-cube P4
        block has 440 M nodes; a localised source touches a few thousand).  Yields (cell0, X, cells): X
        [n, nd, dim]; cells = None for n consecutive cells from cell0, else the block-local cell of every row."""
        box = getattr(expr, "support_box", None)
        if box is None:
            for cell0, X in self.S.node_coords_chunks():
                yield cell0, X, None
            return
        import ctypes as C
        from .functionspace import block_config
        mesh, part, d = self.mesh, self.mesh.partition, self.dimension
        ncls = mesh.cells_per_block
        lo, hi = np.asarray(box[0], dtype=np.float64), np.asarray(box[1], dtype=np.float64)
        rng = []
        for a in range(d):
            o = mesh.origin[a] + part.start[a] * mesh.h[a]
            i0 = max(int(np.floor((lo[a] - o) / mesh.h[a] - 1e-9)), 0)
            i1 = min(int(np.floor((hi[a] - o) / mesh.h[a] + 1e-9)), part.n[a] - 1)
            if i1 < i0:
                return
            rng.append((i0, i1 - i0 + 1))
        cfg = block_config(mesh, self.degree)
        for a in range(d):
            cfg.n[a] = rng[a][1]
            cfg.cube0[a] = part.start[a] + rng[a][0]      # integer offset: the coordinates of the full scan, bit for bit
        nsub = int(np.prod([r[1] for r in rng])) * ncls
        X = np.empty((nsub, self.S.nd, d))
        _lib.check(_lib.load().sg_block_node_coords(C.byref(cfg), self.degree, X.ctypes.data, X.nbytes))
        # sub-box cube (x fastest) -> block cube -> cell = cube * ncls + class
        idx = np.indices([r[1] for r in reversed(rng)]).reshape(d, -1)[::-1]        # [axis][sub cube], x fastest
        cube = np.zeros(idx.shape[1], dtype=np.int64)
        mul = 1
        for a in range(d):
            cube += (idx[a] + rng[a][0]) * mul
            mul *= part.n[a]
        cells = (cube[:, None] * ncls + np.arange(ncls)[None, :]).reshape(-1)
        yield 0, X, cells

    def _source_separable(self, times):
        """(nodes, pattern [nnz, d, d], weights [nsteps]) if the source is S(x, t) = w(t) * pattern(x) on its
        support - what `cond(x) ? f(t) : 0` sources (explosive_source_lf4.py:36-40) and `source_time_function` are -
        else None.  An Expression is TESTED, not assumed: the factorisation found at one pivot entry must
        reproduce the full evaluation at six other steps to round-off."""
        d = self.dimension
        if self.source_time_function is not None:
            vals = self.source_function.dat.data_cells
            nz = np.nonzero(np.abs(vals).reshape(vals.shape[0] * vals.shape[1], -1).max(axis=1) > 0)[0]
            return nz, vals.reshape(-1, d, d)[nz], np.array([float(self.source_time_function(t)) for t in times])
        expr = self.source_expression
        if expr is None or not hasattr(expr, "_params") or "t" not in expr._params or len(times) < 1:
            return None
        t_keep = expr.t
        try:
            nz, Xs = [], []
            for cell0, X, cells in self._support_scan_chunks(expr):
                idx = np.nonzero(expr.support_mask(X).reshape(-1))[0]
                nz.append(idx + cell0 * X.shape[1] if cells is None else cells[idx // X.shape[1]] * X.shape[1] + idx % X.shape[1])
                Xs.append(X.reshape(-1, X.shape[-1])[idx])
            nz, Xs = np.concatenate(nz), np.concatenate(Xs)
            if len(nz) == 0:
                return nz, np.zeros((0, d, d)), np.zeros(len(times))
            n = len(times)
            best = None
            for k in sorted({0, n // 4, n // 2, 3 * n // 4, n - 1}):          # a step where the source is strong
                expr.t = times[k]
                V = expr.evaluate(Xs).reshape(len(nz), d, d)
                if best is None or np.abs(V).max() > np.abs(best[1]).max():
                    best = (k, V)
            k0, pattern = best
            if not np.abs(pattern).max() > 0:
                return None
            piv = np.unravel_index(np.abs(pattern).argmax(), pattern.shape)
            xp = Xs[piv[0]:piv[0] + 1]
            w = expr.evaluate_times(xp, times).reshape(n, d, d)[:, piv[1], piv[2]] / pattern[piv]
            rng = np.random.default_rng(0)
            for k in sorted(set(int(v) for v in rng.integers(0, n, size=6)) | {0, n - 1}):
                expr.t = times[k]
                V = expr.evaluate(Xs).reshape(len(nz), d, d)
                if np.abs(V - w[k] * pattern).max() > 1e-13 * max(np.abs(V).max(), np.abs(w[k] * pattern).max(), 1e-300):
                    return None
            return nz, pattern, w
        finally:
            expr.t = t_keep

    def upload_source(self, times):
        """Hand the source of the next len(times) steps to the device: as a table of nodal values per step
        (the reference's re-interpolation, elastic.py:285-288, restricted to the support) or, when that table would
        exceed SOURCE_TABLE_MAX_BYTES or `source_time_function` is set, as one slice and a weight per step
        (sg_set_source_separable) if the source factorises."""
        if not self.source:
            self._block.set_source([], None)
            return
        if self.source_time_function is not None:
            self._block.set_source_separable(*self._source_separable(times))
            return
        try:
            nodes, values, static = self._source_table(times)
        except MemoryError:
            sep = self._source_separable(times)
            if sep is None:
                raise
            self._block.set_source_separable(*sep)
            return
        self._block.set_source(nodes, values, static=static)

    # ---- receivers (tests/explosive_source/uy.py:31-43) -------------------------------------------
    def set_receivers(self, points, every=1, fields=("velocity",)):
        """Record `fields` ("velocity" = VelocityNew, "stress" = StressNew) at the physical `points` [R, dim] after every
        `every`-th step of the next runs, on the device inside the time loop (sg_set_receivers) - what the reference's
        receiver script gets by writing a VTU file per step and probing every 5th.  Collective with more than one rank:
        every point must have exactly one owning block (ValueError naming the first that has not)."""
        what = 0
        for f in fields:
            if f not in ("velocity", "stress"):
                raise ValueError("receiver fields are 'velocity' and 'stress', not %r" % (f,))
            what |= 1 if f == "velocity" else 2
        if what == 0 or int(every) < 1:
            raise ValueError("set_receivers needs at least one field and every >= 1")
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, self.dimension)
        from .backend import locate_points
        from .functionspace import block_config
        cell, _ = locate_points(block_config(self.mesh, self.degree), pts)
        owners = allreduce_sum_array((cell >= 0).astype(np.float64))
        for k in range(len(pts)):
            if owners[k] != 1:
                raise ValueError("receiver %d at %r has %d owning blocks, not one (outside the mesh?)"
                                 % (k, tuple(pts[k]), int(owners[k])))
        self._receivers = (pts, int(every), what)

    def receiver_traces(self):
        """(times [n], {"velocity": [n, R, dim], "stress": [n, R, dim, dim]}) of the receivers of the last run: sample j
        after step (j + 1) * every, at t = times[j]."""
        if self._receivers is None:
            raise RuntimeError("no receivers: call set_receivers before run")
        pts, every, what = self._receivers
        d = self.dimension
        tr = allreduce_sum_array(self._block.get_receivers())     # rows of the other blocks' receivers are 0 here
        n = tr.shape[0]
        out = {}
        if what & 1:
            out["velocity"] = tr[..., :d].copy()
        if what & 2:
            off = d if what & 1 else 0
            out["stress"] = tr[..., off:off + d * d].reshape(n, len(pts), d, d)
        return np.array(self._receiver_times[:n]), out

    def _arm_receivers(self, times):
        if self._receivers is None:
            return
        pts, every, what = self._receivers
        self._block.set_receivers(pts, what, every, len(times) // every)
        self._receiver_times = list(times[every - 1::every])

    # ---- gauges: strain rate, rotation rate, dilatation rate at points (sg_set_gauges) -----------------
    _GAUGE_KINDS = {"gradient": 0, "dilatation": 1, "rotation": 2, "strain_rate": 3}

    def set_gauges(self, points, kind="strain_rate", every=1, capacity=None):
        """Record the velocity's `kind` - "strain_rate" (symmetric part of the gradient), "gradient", "dilatation" (divergence)
        or "rotation" (curl) - at the physical `points` [R, dim] after every `every`-th step of the next runs, on the device
        inside the time loop (sg_set_gauges): what a strainmeter, a fibre or a rotational seismometer delivers.  The value is
        that of the polynomial of the cell holding the point, on a grid line the lower cell's.  `capacity`: the samples
        the device buffer holds (default: those of the run).  Collective with more than one rank: every point must have
        exactly one owning block (ValueError naming the first that has not)."""
        if kind not in self._GAUGE_KINDS:
            raise ValueError("gauge kinds are %s, not %r" % (", ".join(repr(k) for k in self._GAUGE_KINDS), kind))
        if kind == "rotation" and self.dimension == 1:
            raise ValueError("no rotation in one dimension")
        if int(every) < 1 or (capacity is not None and int(capacity) < 0):
            raise ValueError("set_gauges needs every >= 1 and capacity >= 0")
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, self.dimension)
        from .backend import locate_points
        from .functionspace import block_config
        cell, _ = locate_points(block_config(self.mesh, self.degree), pts)
        owners = allreduce_sum_array((cell >= 0).astype(np.float64))
        for k in range(len(pts)):
            if owners[k] != 1:
                raise ValueError("gauge %d at %r has %d owning blocks, not one (outside the mesh?)"
                                 % (k, tuple(pts[k]), int(owners[k])))
        self._gauges = (pts, int(every), self._GAUGE_KINDS[kind], None if capacity is None else int(capacity))
        self._fibre = None

    def gauge_traces(self):
        """(times [n], values [n, R] + the kind's value shape) of the gauges of the last run: sample j after step
        (j + 1) * every, at t = times[j]; "strain_rate" and "gradient": (dim, dim) with [i, j] = d u_i / d x_j, "dilatation": (),
        "rotation": (3,) in 3-D, () in 2-D."""
        if self._gauges is None:
            raise RuntimeError("no gauges: call set_gauges before run")
        pts, every, kind, capacity = self._gauges
        d = self.dimension
        tr = allreduce_sum_array(self._block.get_gauges())        # rows of the other blocks' gauges are 0 here
        n = tr.shape[0]
        value = {0: (d, d), 1: (), 2: (3,) if d == 3 else (), 3: (d, d)}[kind]
        return np.array(self._gauge_times[:n]), tr.reshape((n, len(pts)) + value)

    def _arm_gauges(self, times):
        if self._gauges is None:
            return
        pts, every, kind, capacity = self._gauges
        self._block.set_gauges(pts, kind, every, len(times) // every if capacity is None else capacity)
        self._gauge_times = list(times[every - 1::every])

    def set_fibre(self, p0, p1, nchannels, gauge_length, nq=4, every=1):
        """A straight fibre from `p0` to `p1` with `nchannels` channels at equal spacing (the first at p0, the last at p1; one
        channel: the midpoint).  Channel c records the axial strain rate t . eps . t, t the unit tangent, averaged over its
        gauge length by `nq` Gauss-Legendre points: strain-rate gauges (set_gauges) at those points, combined from their
        traces on the host (fibre_traces).  Replaces the gauges armed before."""
        pts, t, w = fibre_points(self.dimension, p0, p1, nchannels, gauge_length, nq)
        self.set_gauges(pts, "strain_rate", every)
        self._fibre = (t, w, int(nchannels), int(nq))

    def fibre_traces(self):
        """(times [n], axial strain rate [n, nchannels]) of the fibre of the last run"""
        if self._fibre is None:
            raise RuntimeError("no fibre: call set_fibre before run")
        t, w, nchannels, nq = self._fibre
        times, eps = self.gauge_traces()
        return times, fibre_combine(t, w, nchannels, nq, eps)

    # ---- injectors: force and stress series at points (sg_inject / sg_set_injectors) -----------------
    _INJECT_WHAT = {"velocity": 1, "stress": 2}

    def _injector_args(self, points, amp, what, lead):
        if what not in self._INJECT_WHAT:
            raise ValueError("injectors add to 'velocity' or to 'stress', not %r" % (what,))
        d = self.dimension
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, d)
        amp = np.ascontiguousarray(amp, dtype=np.float64)
        amp = amp.reshape(lead + (len(pts), d if what == "velocity" else d * d))
        from .backend import locate_points
        from .functionspace import block_config
        cell, _ = locate_points(block_config(self.mesh, self.degree), pts)
        owners = allreduce_sum_array((cell >= 0).astype(np.float64))
        for k in range(len(pts)):
            if owners[k] != 1:
                raise ValueError("injector %d at %r has %d owning blocks, not one (outside the mesh?)"
                                 % (k, tuple(pts[k]), int(owners[k])))
        return pts, amp, self._INJECT_WHAT[what]

    # What was injected through this object, so that `rewind` can take it out again: (position, points, amp, what) of every
    # entry added, the position being the number of forward steps the fields have behind them - the library's own step
    # count (sg_get_counters, so el.block.step() counts too) less the steps re-wound.
    def _position(self):
        return self._block.counters()["steps"] - self._rewound

    def _log_armed_series(self):
        """move the entries that the armed series has added so far into the log"""
        if self._armed is None:
            return
        at, pts, amp, w = self._armed
        added = len(amp) - self._block.injector_entries_left()
        self._injected += [(at + k + 1, pts, amp[k], w) for k in range(added)]
        self._armed = (at + added, pts, amp[added:], w) if added < len(amp) else None

    def inject(self, points, amp, what="velocity"):
        """Add amp[r] * delta(x - points[r]), L2-projected onto the cell that holds the point, to the velocity (amp [R, dim])
        or the stress (amp [R, dim, dim]) as they stand now (sg_inject).  The library adds exactly amp * psi: 1/rho and dt of
        a force are the caller's.  Collective with more than one rank: every block is handed all points."""
        pts, amp, w = self._injector_args(points, amp, what, ())
        self._block.inject(pts, amp, w)
        self._injected.append((self._position(), pts, amp.copy(), w))
        self._agree_on_stress_storage()

    def set_injectors(self, points, series, what="velocity"):
        """A series at `points` [R, dim]: series[k] ([R, dim] or [R, dim, dim]) is the entry BEFORE step k + 1 counted from
        this call, k = 0 .. K - 1 - series[0] is added now (sg_inject), series[k] at the end of step k on the device inside
        the time loop (sg_set_injectors), behind that step's receiver and monitor samples.  An empty series disarms."""
        K = 0 if series is None else len(series)
        self._log_armed_series()
        if K == 0:
            self._block.set_injectors(np.zeros((0, self.dimension)), None)
            self._armed = None
            return
        pts, amp, w = self._injector_args(points, series, what, (K,))
        self._block.inject(pts, amp[0], w)
        self._injected.append((self._position(), pts, amp[0].copy(), w))
        self._block.set_injectors(pts, amp[1:], w)
        self._armed = (self._position(), pts, amp[1:].copy(), w) if K > 1 else None
        self._agree_on_stress_storage()

    def rewind(self, nsteps):
        """Undo `nsteps` steps exactly (to round-off): the INVERSE of a step is the stages in the order (SH1, UTEMP, S1, UH1,
        STEMP, U1) with dt negated - the stress update undone first, then the velocity update.  (Stepping on with -dt in the
        normal order is something else: the adjoint of a step in the energy inner product, what an adjoint field is stepped
        with; it re-winds only up to O(dt).)  What `inject` and `set_injectors` of this object added is taken out again
        before the step it followed is undone: a forced run x_k = A x_{k-1} + q_k psi re-winds as A^-1 (x_k - q_k psi), so
        after rewind(n) the fields are those the run held n steps earlier, the entry of that moment included.  A re-wound
        step is no step of the run: it ends without sg_end_step, so receivers and the monitor take no sample, their traces
        stay as the run left them, and the library's step count does not move.  Host-driven, single blocks only; ValueError
        with a source or a sponge (the inverse does not exist) or while a series still has entries to add."""
        if self.mesh.partition.world > 1:
            raise ValueError("rewind drives a single block")
        if self.source:
            raise ValueError("rewind with a source: the source's steps cannot be run backwards")
        if self.absorption_function is not None:
            raise ValueError("rewind with a sponge: an absorbed field cannot be recovered")
        self._log_armed_series()
        if self._armed is not None:
            raise ValueError("rewind with injectors armed: the series has %d entries left (set_injectors(points, None) disarms)"
                             % len(self._armed[2]))
        for name in ("density", "dt", "mu", "l"):
            if getattr(self, name) is None:
                raise ValueError("ElasticLF4.%s must be set before rewind()" % name)
        self._upload_params(-self.dt)
        try:
            for _ in range(int(nsteps)):
                here = self._position()
                for at, pts, amp, w in reversed([e for e in self._injected if e[0] >= here]):
                    self._block.inject(pts, -amp, w)
                self._injected = [e for e in self._injected if e[0] < here]
                for stage in (_lib.STAGE_SH1, _lib.STAGE_UTEMP, _lib.STAGE_S1, _lib.STAGE_UH1, _lib.STAGE_STEMP, _lib.STAGE_U1):
                    self._block.run_stage(stage)
                self._rewound += 1
                self._step_index -= 1
        finally:
            self._upload_params(self.dt)

    # ---- monitor: L2 norms and elastic energy inside the time loop (sg_set_monitor) -----------------
    def energy_weights(self):
        """The weights of the monitor's energies from `density`, `mu`, `l` (monitor_weights)."""
        for name in ("density", "mu", "l"):
            if getattr(self, name) is None:
                raise ValueError("ElasticLF4.%s must be set before the energy can be weighted" % name)
        return monitor_weights(self.dimension, self.density, self.mu, self.l, self._block.ncells)

    def set_monitor(self, every=1):
        """Record the L2 norms of (u1, s1) and the kinetic and strain energy after every `every`-th step of the next runs,
        on the device inside the time loop; every = 0: no monitor."""
        if int(every) < 0:
            raise ValueError("set_monitor needs every >= 0")
        self._monitor = int(every) or None

    def monitor_trace(self):
        """(times [n], {"u_l2", "s_l2", "kinetic", "strain", "energy"}: [n] each) of the last run: sample j after step
        (j + 1) * every at t = times[j] (u1 at t, s1 at t + dt/2).  Collective with more than one rank: the blocks' sums
        are added."""
        if self._monitor is None:
            raise RuntimeError("no monitor: call set_monitor before run")
        tr = allreduce_sum_array(self._block.get_monitor())
        return np.array(self._monitor_times[:tr.shape[0]]), self._monitor_quantities(tr)

    @staticmethod
    def _monitor_quantities(tr):
        return {"u_l2": np.sqrt(tr[..., 0]), "s_l2": np.sqrt(tr[..., 1]), "kinetic": tr[..., 3].copy(), "strain": tr[..., 4].copy(),
                "energy": tr[..., 3] + tr[..., 4]}

    def energy(self):
        """The quantities of monitor_trace of the fields as they stand now (one sg_measure); collective."""
        return {k: float(v) for k, v in self._monitor_quantities(allreduce_sum_array(self._block.measure(self.energy_weights()))).items()}

    def _arm_monitor(self, times):
        if self._monitor is None:
            return
        every = self._monitor
        self._block.set_monitor(every, max(1, len(times) // every), self.energy_weights())
        self._monitor_times = list(times[every - 1::every])

    # ---- spectra: running Fourier transforms inside the time loop (sg_set_spectra) ---------------------
    def set_spectra(self, freqs, every=1, nsamples=None, fields=("velocity", "stress"), window=None):
        """Accumulate the Fourier transforms of `fields` ("velocity" = VelocityNew at t, "stress" = StressNew at t + dt/2) at
        the frequencies `freqs` (Hz) over the next runs, on the device inside the time loop: sample j after step
        (j + 1) * every with the weights of spectra_weights (the rectangle rule, t from 0 at the start of the run, stagger
        dt / 2 for the stress), `nsamples` of them (None: all the run has).  No frequencies: none.  It works with a source
        and a sponge, and keeps 2 (dim + dim^2) doubles per node and frequency."""
        freqs = np.atleast_1d(np.asarray([] if freqs is None else freqs, dtype=np.float64)).ravel()
        if freqs.size == 0:
            self._spectra = None
            return
        what = 0
        for f in fields:
            if f not in ("velocity", "stress"):
                raise ValueError("spectra fields are 'velocity' and 'stress', not %r" % (f,))
            what |= 1 if f == "velocity" else 2
        if what == 0 or int(every) < 1 or freqs.size > _lib.SPECTRA_MAX_FREQ:
            raise ValueError("set_spectra needs at least one field, every >= 1 and at most %d frequencies" % _lib.SPECTRA_MAX_FREQ)
        self._spectra = (freqs, int(every), None if nsamples is None else int(nsamples), what, window)

    def _arm_spectra(self, times):
        if self._spectra is None:
            if self._spectra_freqs is not None:
                self._block.set_spectra(None, None)
                self._spectra_freqs = None
            return
        freqs, every, nsamples, what, window = self._spectra
        n = len(times) // every if nsamples is None else nsamples
        if n < 1:
            raise ValueError("set_spectra: the run has no sample step (every = %d, %d steps)" % (every, len(times)))
        wu = spectra_weights(freqs, self.dt, every, n, window=window) if what & 1 else None
        ws = spectra_weights(freqs, self.dt, every, n, stagger=0.5 * self.dt, window=window) if what & 2 else None
        self._block.set_spectra(wu, ws, every)
        self._spectra_freqs = freqs

    def _spectrum_index(self, f):
        if self._spectra_freqs is None:
            raise RuntimeError("no spectra: call set_spectra before run")
        k = np.nonzero(self._spectra_freqs == float(f))[0]
        if k.size == 0:
            raise ValueError("frequency %r is none of the armed ones %r" % (f, list(self._spectra_freqs)))
        return int(k[0])

    def spectrum(self, field, f):
        """The transform of `field` ("velocity" or "stress") at the armed frequency `f` as accumulated so far: a complex array
        in the shape of the Function's data ([nodes, dim] or [nodes, dim, dim]), of this rank's block."""
        if field not in ("velocity", "stress"):
            raise ValueError("spectra fields are 'velocity' and 'stress', not %r" % (field,))
        d = self.dimension
        out = self._block.get_spectrum(0 if field == "velocity" else 1, self._spectrum_index(f))
        return out.reshape((-1, d) if field == "velocity" else (-1, d, d))

    def spectrum_torch(self, field, f):
        """`spectrum` as a complex128 torch tensor on the block's device, moved on the device (no host copy)."""
        if field not in ("velocity", "stress"):
            raise ValueError("spectra fields are 'velocity' and 'stress', not %r" % (field,))
        d = self.dimension
        out = self._block.get_spectrum_dev(0 if field == "velocity" else 1, self._spectrum_index(f))
        return out.reshape((-1, d) if field == "velocity" else (-1, d, d))

    def correlate_spectra(self, other, f, f_other=None, weights=(1.0, 1.0, 1.0), z=1 + 0j):
        """Add weights * Re(z conj(a^(f)) . b^(f_other)) in the forms (uu, ss, tt) of `correlate` - a^ this solver's spectra,
        b^ `other`'s (f_other = None: the same frequency) - to this block's per-cell accumulator (correlation,
        reset_correlation): the frequency-domain imaging condition is the sum of these calls over the frequencies."""
        fo = f if f_other is None else f_other
        self._block.correlate_spectra(other._block, self._spectrum_index(f), other._spectrum_index(fo), weights, z)

    # ---- peak maps: per-node maxima of |u|^2 and s:s inside the time loop (sg_set_peaks) ---------------
    def set_peaks(self, fields=("velocity",), every=1, nsamples=None):
        """Keep, over the next runs, per node the largest |u| ("velocity" = VelocityNew at t) and / or the largest
        sqrt(s:s) ("stress" = StressNew at t + dt/2) and the time it was reached, on the device inside the time loop: sample
        j after step (j + 1) * every, `nsamples` of them (None: all the run has).  No fields: none.  It works with a source
        and a sponge, and keeps 12 bytes per node and field."""
        what = 0
        for f in fields or ():
            if f not in ("velocity", "stress"):
                raise ValueError("peak fields are 'velocity' and 'stress', not %r" % (f,))
            what |= 1 if f == "velocity" else 2
        if what == 0:
            self._peaks = None
            return
        if int(every) < 1:
            raise ValueError("set_peaks needs every >= 1")
        self._peaks = (what, int(every), None if nsamples is None else int(nsamples))

    def _arm_peaks(self, times):
        if self._peaks is None:
            if self._peaks_armed is not None:
                self._block.set_peaks(0)
                self._peaks_armed = None
            return
        what, every, nsamples = self._peaks
        n = len(times) // every if nsamples is None else nsamples
        if n < 1:
            raise ValueError("set_peaks: the run has no sample step (every = %d, %d steps)" % (every, len(times)))
        self._block.set_peaks(what, every, n)
        self._peaks_armed = (what, every)

    def _peak_field(self, field):
        if field not in ("velocity", "stress"):
            raise ValueError("peak fields are 'velocity' and 'stress', not %r" % (field,))
        if self._peaks_armed is None or not self._peaks_armed[0] & (1 if field == "velocity" else 2):
            raise RuntimeError("no peak map of the %s: call set_peaks before run" % field)
        return (0 if field == "velocity" else 1), self._peaks_armed[1], (0.0 if field == "velocity" else 0.5 * self.dt)

    def peak_map(self, field):
        """The peak map of `field` ("velocity" or "stress") as recorded so far, of this rank's block, per node in the order
        of the Function's data: {"amplitude": the largest |u| or sqrt(s:s), "time": when it was reached - (sample + 1) *
        every * dt from the start of the run, + dt / 2 for the stress; NaN where the node never moved -, "sample": the
        0-based sample, -1 there}."""
        k, every, stagger = self._peak_field(field)
        value, sample = self._block.get_peaks(k)
        value, sample = value.ravel(), sample.ravel()
        time = np.where(sample >= 0, (sample.astype(np.float64) + 1.0) * every * self.dt + stagger, np.nan)
        return {"amplitude": np.sqrt(value), "time": time, "sample": sample}

    def peak_map_torch(self, field):
        """`peak_map` as torch tensors on the block's device, moved on the device (no host copy)."""
        import torch
        k, every, stagger = self._peak_field(field)
        value, sample = self._block.get_peaks_dev(k)
        value, sample = value.reshape(-1), sample.reshape(-1)
        time = torch.where(sample >= 0, (sample.to(torch.float64) + 1.0) * every * self.dt + stagger,
                           torch.full_like(value, float("nan")))
        return {"amplitude": torch.sqrt(value), "time": time, "sample": sample}

    # ---- correlation with another solver's fields, cell by cell (sg_correlate) ------------------------
    def correlate(self, other, weights=(1.0, 1.0, 1.0)):
        """Add weights * (uu, ss, tt) of this solver's (u1, s1) against `other`'s - an ElasticLF4 on the same mesh and
        device, e.g. the forward field being re-wound beside the adjoint - to this block's per-cell accumulator.  The
        caller drives the call between steps; the correlation with a time derivative is two calls with weights -+ 1/dt."""
        self._block.correlate(other._block, weights)

    def correlation(self):
        """{"uu", "ss", "tt"}: [ncells] each, of this rank's block (nothing to reduce across ranks)."""
        acc = self._block.get_correlation()
        return {"uu": acc[:, 0].copy(), "ss": acc[:, 1].copy(), "tt": acc[:, 2].copy()}

    def reset_correlation(self):
        self._block.reset_correlation()

    # ---- derivatives of the velocity at the nodes, on the device (sg_get_gradient_dev) ------------------
    def strain_rate(self, out=None, dtype=None):
        """The symmetric strain rate 1/2 (grad u + grad u^T) of u1 at the nodes of this rank's block - what a fibre or a
        strainmeter records - as a torch tensor [cells, nodes, dim, dim] on the device (Function.gradient)."""
        return self._block.get_gradient_dev(_lib.FIELD_U, "strain", out=out, dtype=dtype)

    def dilatation(self, out=None, dtype=None):
        """The dilatation rate div u1 [cells, nodes]: the P wave alone."""
        return self._block.get_gradient_dev(_lib.FIELD_U, "div", out=out, dtype=dtype)

    def rotation(self, out=None, dtype=None):
        """The rotation rate curl u1, [cells, nodes, 3] in 3-D and [cells, nodes] in 2-D: the S wave alone."""
        return self._block.get_gradient_dev(_lib.FIELD_U, "curl", out=out, dtype=dtype)

    # ---- frames: images of the wavefield taken inside the time loop (sg_get_frame_dev) ----------------
    def set_frames(self, function="velocity", m=1, slice=None, every=1, dtype=None):
        """Take a frame of `function` ("velocity" = VelocityNew or "stress" = StressNew; Function.frame has `m` and `slice`)
        after every `every`-th step of the next runs: frame j after step (j + 1) * every, into one pre-allocated torch
        tensor [nframes, ...] on the device (`dtype`: torch.float64, the default, or torch.float32), which frames() returns.
        The run advances in chunks of `every` steps, a frame queued behind each; the remaining steps follow at the end.
        function = None: no frames, and run takes the path it takes without this call.  Single-rank meshes only."""
        if function is None:
            self._frames = None
            self._frame_stack = None
            return
        if function not in ("velocity", "stress"):
            raise ValueError("frames are taken of 'velocity' or 'stress', not %r" % (function,))
        if int(every) < 1:
            raise ValueError("set_frames: every >= 1")
        if self.output:
            raise ValueError("set_frames: not with output=True, whose loop writes a file per step")
        if self.mesh.partition.world > 1:
            raise NotImplementedError("set_frames: single-rank meshes only (the blocks of a partitioned mesh hold parts of the image)")
        self._frames = (function, m, None if slice is None else dict(slice), int(every), dtype)
        self._frame_stack = None

    def frames(self):
        """The frames of the last run: a torch tensor [nframes] + Function.frame's shape on the device."""
        if self._frame_stack is None:
            raise RuntimeError("no frames: call set_frames before run")
        return self._frame_stack

    def _advance_with_frames(self, nsteps):
        import torch
        function, m, slice, every, dtype = self._frames
        field = _lib.FIELD_U if function == "velocity" else _lib.FIELD_S
        blk = self._block
        nframes = nsteps // every
        self._frame_stack = torch.empty((nframes,) + blk.frame_shape(field, m, slice), dtype=dtype or torch.float64, device=blk._torch_device())
        for j in range(nframes):
            self._advance(every)
            blk.get_frame_dev(field, m=m, slice=slice, out=self._frame_stack[j])
        if nsteps - nframes * every:
            self._advance(nsteps - nframes * every)

    # ---- time loop (elastic.py:267-315) ----------------------------------------------------------
    def step_times(self, T):
        """The values of `t` visited by the reference loop ``t = dt; while t <= T + 1e-12``."""
        times = []
        t = self.dt
        while t <= T + 1e-12:
            times.append(t)
            t += self.dt
        return times

    def _advance(self, nsteps):
        if self._exchanger is not None:
            if os.environ.get("SEIGEN_HALO_SCHEDULE", "pipelined") == "plain":
                self._exchanger.step_unpipelined(nsteps)      # input traces || interior, then the shell
            else:
                self._exchanger.step(nsteps)
        else:
            self._block.step(nsteps)
        self._step_index += nsteps

    def _agree_on_stress_storage(self):
        """A block leaves symmetric-stress storage when IT is handed a non-symmetric stress or
        source; its neighbours read its traces, so all blocks of the mesh must store alike."""
        if self.mesh.partition.world > 1:
            mine = 0 if self._block.is_sym() else 1
            if allreduce_sum(mine) > 0 and not mine:
                self._block.leave_sym()

    def run(self, T):
        """Run the elastic wave simulation until t = T; returns (u1, s1)."""
        # Write out the initial condition.
        self.write(self.u1, self.s1)

        # Call solver-specific setup
        self.setup()

        with timed_region('timestepping'):
            times = self.step_times(T)
            with timed_region('source term update'):
                self.upload_source(times)
            self._agree_on_stress_storage()
            self._arm_receivers(times)
            self._arm_gauges(times)
            self._arm_monitor(times)
            self._arm_spectra(times)
            self._arm_peaks(times)
            with self.loop_context():
                if self.output:
                    for t in times:
                        log("t = %f" % t)
                        self._advance(1)
                        self.write(self.u1, self.s1)
                elif self._frames is not None:
                    self._advance_with_frames(len(times))
                else:
                    # the eight solves + two assigns of every step, without returning to Python
                    self._advance(len(times))
            self._block.sync()
            if self.source and self.source_expression is not None and times and \
                    self.source_time_function is None and \
                    "t" in getattr(self.source_expression, "_params", {}):
                self.source_expression.t = times[-1]
                self.source = self.source_expression
        return self.u1, self.s1


class ImplicitElasticLF4(ElasticLF4):
    r"""``solver='implicit'`` (``seigen/elastic.py:318-332``): the reference wraps each of the eight
    forms in a ``LinearVariationalSolver``.  Every left-hand side is a DG mass matrix - block diagonal,
    one dense block per cell - so what the KSP converges to is the element-wise inverse applied to the
    assembled right-hand side: the arithmetic of the explicit path, which the GPU kernels fuse into the
    stage launches (no iteration, no tolerance; the reference's answer differs from it by its KSP
    tolerance).  What does differ between the two reference classes is ``form_u1``: the implicit one
    keeps the density on the left (``:175-178``: rho (u - u0)/dt = uh1 + dt^2/24 uh2), the explicit one
    multiplies u0 by it (``:341-345``).  This class therefore runs the same six launches with
    ``density_physical = True``; for rho = 1 (every reference test) the two coincide."""

    def __init__(self, *args, **kwargs):
        super(ImplicitElasticLF4, self).__init__(*args, **kwargs)
        self.density_physical = True


class ExplicitElasticLF4(ElasticLF4):
    r"""Explicit solves: RHS assembly and element-wise inverse mass fused on the GPU
    (``seigen/elastic.py:335-385``)."""
    pass


class TilingElasticLF4(ExplicitElasticLF4):
    r"""'parloop' / 'fusion' / 'tiling' of the reference (``seigen/elastic.py:388-515``)
    differ from 'explicit' only in HOW the CPU executes the same arithmetic (per-cell
    mat-vec par_loop, PyOP2 loop fusion, SLOPE tiling).  On the GPU that role is played
    by kernel fusion inside libseigen_hip, so these modes share the explicit path."""

    loop_chain_length = 28
    num_solves = 8
    tile_size = 1000
    extra_halo = 0

    def __init__(self, mesh, *args, **kwargs):
        self.tiling_mode = kwargs.pop("tiling_mode", None)
        self.num_unroll = 0 if self.tiling_mode is None else 1
        super(TilingElasticLF4, self).__init__(mesh, *args, **kwargs)

    def calculate_sdepth(self, num_solves, num_unroll, extra_halo):
        """Halo depth the reference would request (``seigen/elastic.py:422-436``); the HIP
        path always exchanges depth-1 facet traces per stage."""
        if world()[1] > 1:
            return 1 + num_solves * num_unroll + extra_halo
        return 1
