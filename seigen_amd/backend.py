"""Thin object wrapper around one `sg_handle` (one mesh block on one GPU)."""
import ctypes as C
import numpy as np

from . import _lib
from ._lib import SgConfig, SgFrame, SgInfo, SgCounters, check


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def comm_unique_id():
    """A fresh RCCL unique id (bytes) for sg_comm_init: made on one rank, handed to all ranks of the block grid."""
    buf = C.create_string_buffer(_lib.COMM_ID_BYTES)
    check(_lib.load().sg_comm_get_unique_id(buf, _lib.COMM_ID_BYTES))
    return bytes(buf.raw)


def comm_library():
    """(path, version) of the RCCL the native exchange is bound to (sg_comm_library / sg_comm_version); raises where
    there is none."""
    buf = C.create_string_buffer(1024)
    check(_lib.load().sg_comm_library(buf, len(buf)))
    v = C.c_int()
    check(_lib.load().sg_comm_version(C.byref(v)))
    return buf.value.decode(), int(v.value)


def locate_points(cfg, points):
    """(cell [npts], xi [npts, dim]) of the points [npts, dim] in the block `cfg` (an SgConfig) describes: the block-local
    cell that owns each point, -1 where another block or no block of the mesh does (sg_locate_points; device-free)."""
    pts = _f64(points).reshape(-1, cfg.dim)
    cell = np.empty(len(pts), dtype=np.int64)
    xi = np.empty((len(pts), cfg.dim))
    check(_lib.load().sg_locate_points(C.byref(cfg), len(pts), pts.ctypes.data, cell.ctypes.data, xi.ctypes.data))
    return cell, xi


def injector_weights(cfg, points, nd):
    """(cell [npts], psi [npts, nd]) of the points [npts, dim] in the block `cfg` (an SgConfig) describes: the owning cell
    as locate_points gives it and psi = Mhat^-1 phi(xi) / |det J|, what an injector of unit amplitude adds to that cell's
    nodes (sg_injector_weights; device-free); nd: scalar nodes per cell."""
    pts = _f64(points).reshape(-1, cfg.dim)
    cell = np.empty(len(pts), dtype=np.int64)
    psi = np.zeros((len(pts), int(nd)))
    check(_lib.load().sg_injector_weights(C.byref(cfg), len(pts), pts.ctypes.data, cell.ctypes.data, psi.ctypes.data))
    return cell, psi


def make_frame(dim, m=1, slice=None):
    """The sg_frame of `m` pixels per cube (an int or a per-axis tuple) and `slice` = {axis: coordinate} (the plane
    x_axis = coordinate; m is ignored along a sliced axis)."""
    fr = SgFrame()
    ms = [int(m)] * dim if np.isscalar(m) else [int(x) for x in m]
    if len(ms) != dim:
        raise ValueError("m: an int or one value per axis (%d)" % dim)
    slice = dict(slice or {})
    if any(not (0 <= int(a) < dim) for a in slice):
        raise ValueError("slice: axes 0 .. %d" % (dim - 1))
    for a in range(3):
        fr.m[a] = ms[a] if a < dim else 1
        fr.fixed[a] = 0
        fr.at[a] = 0.0
    for a, x in slice.items():
        fr.fixed[int(a)] = 1
        fr.at[int(a)] = float(x)
    return fr


def frame_plan(cfg, fr):
    """sg_frame_plan of the frame `fr` (make_frame) on the block `cfg` (an SgConfig) describes, as a dict (device-free);
    `groups`: the listed cube groups"""
    out = np.zeros(12, dtype=np.int64)
    check(_lib.load().sg_frame_plan(C.byref(cfg), C.byref(fr), out.ctypes.data))
    p = {"P": tuple(int(x) for x in out[:3]), "Q": int(out[3]), "owns": bool(out[4]), "layer": tuple(int(x) for x in out[5:8]),
         "ngroups": int(out[8]), "units": int(out[9]), "grid": int(out[10]), "gw": int(out[11])}
    groups = np.zeros(max(1, p["ngroups"]), dtype=np.int32)
    n = _lib.load().sg_frame_groups(C.byref(cfg), C.byref(fr), groups.ctypes.data, len(groups))
    if n != p["ngroups"]:
        raise _lib.SeigenHipError("sg_frame_groups returned %d, the plan has %d groups" % (n, p["ngroups"]))
    p["groups"] = groups[:n]
    return p


def frame_weights(cfg, degree, fr, nd):
    """(cls [Q], xi [Q, dim], phi [Q, nd]) of the in-cube pixels of the frame (sg_frame_weights; device-free)"""
    Q = frame_plan(cfg, fr)["Q"]
    cls = np.zeros(Q, dtype=np.int32)
    xi = np.zeros((Q, cfg.dim))
    phi = np.zeros((Q, int(nd)))
    check(_lib.load().sg_frame_weights(C.byref(cfg), int(degree), C.byref(fr), cls.ctypes.data, xi.ctypes.data, phi.ctypes.data))
    return cls, xi, phi


GRADIENT_KINDS = {"grad": 0, "div": 1, "curl": 2, "strain": 3}


def gradient_kind(kind):
    """the `kind` of sg_get_gradient_dev from its name or number"""
    k = GRADIENT_KINDS.get(kind, kind)
    if k not in (0, 1, 2, 3):
        raise ValueError("kind: %s or 0 .. 3" % ", ".join(repr(n) for n in GRADIENT_KINDS))
    return int(k)


def gradient_tables(cfg):
    """(C [dim, nd, nd], J [ncls, 3, 3]) of the block `cfg` (an SgConfig) describes: C[r, a, b] = d(phi_b)/d(xi_r) at node a,
    J[k, r, j] = d(xi_r)/d(x_j) of class k - the tables of sg_get_gradient_dev (sg_gradient_tables; device-free)"""
    L = _lib.load()
    size = L.sg_gradient_tables(C.byref(cfg), None, None)
    if size < 0:
        raise _lib.SeigenHipError("sg_gradient_tables refuses the configuration")
    d = cfg.dim
    nd = int(round((size // d) ** 0.5))
    ncls = 1 if cfg.diagonal == 2 else {1: 1, 2: 2, 3: 6}[d]
    Ct, J = np.zeros((d, nd, nd)), np.zeros((ncls, 3, 3))
    if L.sg_gradient_tables(C.byref(cfg), Ct.ctypes.data, J.ctypes.data) != size:
        raise _lib.SeigenHipError("sg_gradient_tables failed")
    return Ct, J


def gauge_weights(cfg, points, nd):
    """(cell [npts], D [npts, dim, nd]) of the points [npts, dim] in the block `cfg` (an SgConfig) describes: the owning cell as
    locate_points gives it and D[k, r, a] = d(phi_a)/d(xi_r) at the point - the dense rows of a gauge (sg_gauge_weights;
    device-free); nd: scalar nodes per cell."""
    pts = _f64(points).reshape(-1, cfg.dim)
    cell = np.empty(len(pts), dtype=np.int64)
    D = np.zeros((len(pts), cfg.dim, int(nd)))
    got = _lib.load().sg_gauge_weights(C.byref(cfg), len(pts), pts.ctypes.data, cell.ctypes.data, D.ctypes.data)
    if got != int(nd):
        raise _lib.SeigenHipError("sg_gauge_weights returned %d, the cells have %d nodes" % (got, int(nd)))
    return cell, D


def mfma_class_frame(cfg, operators=False):
    """the class frame of the 3-D matrix-pipe F stages for the block `cfg` (an SgConfig) describes (sg_mfma_class_frame;
    device-free): p [6, 3], s [6, 3], cn [6, 4, 2], own [6, 2, 9], trace [6, 2, 4, 6], vel [6, 3] - line offsets in values of
    the field type, storage 0 = full tensor, 1 = symmetric - and, with operators, E and Ed [3, nd, nd]"""
    L = _lib.load()
    nd = L.sg_mfma_class_frame(C.byref(cfg), None, None, None, None, None, None)
    if nd < 0:
        raise _lib.SeigenHipError("sg_mfma_class_frame refuses the configuration")
    p, s, cn = np.zeros((6, 3), dtype=np.int32), np.zeros((6, 3)), np.zeros((6, 4, 2))
    lines = np.zeros((6, 2, 36), dtype=np.int32)
    E, Ed = np.zeros((3, nd, nd)), np.zeros((3, nd, nd))
    if L.sg_mfma_class_frame(C.byref(cfg), p.ctypes.data, s.ctypes.data, cn.ctypes.data, lines.ctypes.data,
                             E.ctypes.data if operators else None, Ed.ctypes.data if operators else None) != nd:
        raise _lib.SeigenHipError("sg_mfma_class_frame failed")
    out = {"p": p, "s": s, "cn": cn, "own": lines[:, :, :9].copy(), "trace": lines[:, :, 9:33].reshape(6, 2, 4, 6).copy(),
           "vel": lines[:, 0, 33:].copy()}
    if operators:
        out.update(E=E, Ed=Ed)
    return out


def gradient_plan(gw, ncls, nd, dim, ncomp, dev_bytes=8, caller_bytes=8, cell0=0, ncells=0):
    """sg_gradient_plan as a dict (device-free)"""
    out = np.zeros(6, dtype=np.int64)
    check(_lib.load().sg_gradient_plan(gw, ncls, nd, dim, ncomp, dev_bytes, caller_bytes, cell0, ncells, out.ctypes.data))
    return dict(zip(("item0", "nitems", "nodes_per_slice", "slices", "grid", "lds_bytes"), (int(x) for x in out)))


class HipBlock(object):
    def __init__(self, dim, degree, n, h, origin, diagonal="left", nbr_mask=0, device=0, stream=None, dtype="f64",
                 cube0=None):
        """origin: the block's low corner - or, with `cube0` (the block's first cube counted from there), the origin
        of the whole mesh: node coordinates are then bitwise those of the unpartitioned mesh (sg_config::cube0)."""
        self.lib = _lib.load()
        if dtype not in ("f64", "f32"):
            raise ValueError("dtype must be 'f64' or 'f32'")
        self.dtype = dtype
        cfg = SgConfig()
        cfg.dim, cfg.degree = dim, degree
        cfg.dtype = 1 if dtype == "f32" else 0
        for a in range(3):
            cfg.n[a] = int(n[a]) if a < dim else 1
            cfg.h[a] = float(h[a]) if a < dim else 1.0
            cfg.origin[a] = float(origin[a]) if a < dim else 0.0
            cfg.cube0[a] = int(cube0[a]) if (cube0 is not None and a < dim) else 0
        cfg.diagonal = {"left": 0, "right": 1, "quadrilateral": 2}[diagonal]   # 2: the squares are the cells
        cfg.nbr_mask = int(nbr_mask)
        cfg.device = int(device)
        cfg.stream = C.c_void_p(stream) if stream else None
        hp = C.c_void_p()
        rc = self.lib.sg_create(C.byref(cfg), C.byref(hp))
        if rc != 0:
            raise _lib.SeigenHipError("sg_create failed (%d): %s" %
                                      (rc, (self.lib.sg_last_error(None) or b"").decode()))
        self.h = hp
        info = SgInfo()
        check(self.lib.sg_get_info(self.h, C.byref(info)), self.h)
        self.dim, self.degree = dim, degree
        self.n = tuple(int(n[a]) for a in range(dim))
        self.nd, self.nf, self.nfaces, self.ncls = info.nd, info.nf, info.nfaces, info.nclasses
        self.ncells = int(info.ncells)
        self.u_dofs, self.s_dofs = int(info.u_dofs), int(info.s_dofs)
        self.halo_faces = [int(x) for x in info.halo_faces]
        self.nbr_mask = int(nbr_mask)
        self._device = int(device)
        self._inj = None                # (what, entries, the library's step count at the arming call) of set_injectors

    def stream_ptr(self):
        """hipStream_t (as an integer) the block launches on."""
        p = C.c_void_p()
        check(self.lib.sg_get_stream(self.h, C.byref(p)), self.h)
        return p.value or 0

    def stream2_ptr(self):
        """hipStream_t of the stream that SG_REGION_SECOND launches of a split stage run on, or 0."""
        p = C.c_void_p()
        check(self.lib.sg_get_second_stream(self.h, C.byref(p)), self.h)
        return p.value or 0

    def close(self):
        if getattr(self, "h", None):
            self.lib.sg_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- shapes ---------------------------------------------------------------------
    def field_shape(self, field):
        d = self.dim
        if field in (_lib.FIELD_S, _lib.FIELD_SH):
            return (self.ncells, self.nd, d, d)
        return (self.ncells, self.nd, d)

    def node_coords(self, degree=None):
        degree = self.degree if degree is None else int(degree)
        nq = {1: degree + 1, 2: (degree + 1) * (degree + 2) // 2,
              3: (degree + 1) * (degree + 2) * (degree + 3) // 6}[self.dim]
        if self.nfaces == 2 * self.dim and self.dim > 1:      # tensor-product cells
            nq = (degree + 1) ** self.dim
        out = np.empty((self.ncells, nq, self.dim))
        check(self.lib.sg_node_coords(self.h, degree, out.ctypes.data, out.nbytes), self.h)
        return out

    # ---- data -------------------------------------------------------------------------
    def set_field(self, field, arr):
        arr = _f64(arr).reshape(self.field_shape(field))
        check(self.lib.sg_set_field(self.h, field, arr.ctypes.data, arr.nbytes), self.h)

    def get_field(self, field):
        out = np.empty(self.field_shape(field))
        check(self.lib.sg_get_field(self.h, field, out.ctypes.data, out.nbytes), self.h)
        return out

    def set_field_range(self, field, cell0, arr):
        arr = _f64(arr)
        ncells = arr.shape[0]
        check(self.lib.sg_set_field_range(self.h, field, int(cell0), int(ncells), arr.ctypes.data, arr.nbytes), self.h)

    def get_field_range(self, field, cell0, ncells, out=None):
        """`out`: a C-contiguous float64 array to fill (re-used buffers skip the page faults of a fresh one)"""
        shape = (int(ncells),) + self.field_shape(field)[1:]
        if out is None:
            out = np.empty(shape)
        elif out.shape != shape or out.dtype != np.float64 or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous float64 array of shape %r" % (shape,))
        check(self.lib.sg_get_field_range(self.h, field, int(cell0), int(ncells), out.ctypes.data, out.nbytes), self.h)
        return out

    # ---- device transfers (sg_get_field_dev / sg_set_field_dev / sg_get_spectrum_dev) -------------------------
    def _torch_device(self):
        import torch
        return torch.device("cuda", self._device)

    def _on_stream(self, tensor, call):
        """Run `call` - one queued-only library call that reads or writes `tensor` - ordered against torch's current stream in
        both directions, without a host wait: the handle's stream first waits for torch's current stream, torch's current
        stream then waits for the handle's.  The caching allocator is told that the CURRENT stream uses the tensor, not the
        handle's: the current stream has just been put behind the handle's launch, so memory freed and handed out again is
        behind it too - and the allocator records an event on every stream it was told of when the tensor is freed, which
        may be after sg_destroy has destroyed a stream the handle owned."""
        import torch
        with torch.cuda.device(self._device):
            mine = torch.cuda.ExternalStream(self.stream_ptr(), device=self._device)
            cur = torch.cuda.current_stream(self._device)
            if mine.cuda_stream != cur.cuda_stream:
                mine.wait_stream(cur)
            call()
            if mine.cuda_stream != cur.cuda_stream:
                cur.wait_stream(mine)
            tensor.record_stream(cur)

    def _dev_tensor(self, t, shape, who):
        import torch
        if not isinstance(t, torch.Tensor) or t.device != self._torch_device() or t.dtype not in (torch.float64, torch.float32) \
                or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
            raise ValueError("%s takes a contiguous float64 or float32 tensor of shape %r on %s" % (who, tuple(shape), self._torch_device()))
        return 1 if t.dtype == torch.float32 else 0

    def get_field_dev(self, field, out=None, dtype=None, cell0=0, ncells=None):
        """Cells cell0 .. cell0 + ncells - 1 (default: to the last) of a field as a torch tensor [ncells, nd, comps...] on the
        block's device, float64 or float32 (`dtype`, default float64, or that of `out`), moved on the device: the launch is
        queued on the block's stream between torch's current stream before and after, and nothing waits on the host."""
        import torch
        ncells = self.ncells - int(cell0) if ncells is None else int(ncells)
        shape = (ncells,) + self.field_shape(field)[1:]
        if out is None:
            out = torch.empty(shape, dtype=dtype or torch.float64, device=self._torch_device())
        elif dtype is not None and out.dtype != dtype:
            raise ValueError("out is %s, dtype asks for %s" % (out.dtype, dtype))
        code = self._dev_tensor(out, shape, "get_field_dev")
        nbytes = out.numel() * out.element_size()
        self._on_stream(out, lambda: check(self.lib.sg_get_field_dev(self.h, int(field), int(cell0), ncells, C.c_void_p(out.data_ptr()),
                                                                     code, nbytes), self.h))
        return out

    def set_field_dev(self, field, tensor, cell0=0):
        """The cells from `cell0` of a field from a contiguous float64 or float32 tensor [ncells, nd, comps...] of the block's
        device, moved on the device.  Queued like get_field_dev - but a stress handed to a block in symmetric storage makes
        the host wait once for the answer whether it is symmetric (include/seigen_hip.h sg_set_field_dev)."""
        import torch
        if not isinstance(tensor, torch.Tensor) or tensor.dim() < 1:
            raise ValueError("set_field_dev takes a torch tensor [ncells, nd, comps...]")
        shape = (int(tensor.shape[0]),) + self.field_shape(field)[1:]
        code = self._dev_tensor(tensor, shape, "set_field_dev")
        nbytes = tensor.numel() * tensor.element_size()
        self._on_stream(tensor, lambda: check(self.lib.sg_set_field_dev(self.h, int(field), int(cell0), shape[0], C.c_void_p(tensor.data_ptr()),
                                                                        code, nbytes), self.h))

    def get_spectrum_dev(self, field, freq):
        """get_spectrum as a complex128 torch tensor on the block's device, moved on the device (sg_get_spectrum_dev)."""
        import torch
        k = {0: 0, 1: 1, _lib.FIELD_S: 1}[int(field)]
        shape = self.field_shape(_lib.FIELD_S if k else _lib.FIELD_U)
        parts = [torch.empty(shape, dtype=torch.float64, device=self._torch_device()) for _ in range(2)]
        for part, t in enumerate(parts):
            self._on_stream(t, lambda: check(self.lib.sg_get_spectrum_dev(self.h, k, int(freq), part, C.c_void_p(t.data_ptr()), 0,
                                                                          t.numel() * 8), self.h))
        return torch.complex(parts[0], parts[1])

    # ---- frames (sg_get_frame_dev) ---------------------------------------------------------------------------
    def frame_shape(self, field, m=1, slice=None):
        """value shape + (P_{d-1}, ..., P_0) of get_frame_dev, the sliced axes dropped"""
        fr = make_frame(self.dim, m, slice)
        value = (self.dim, self.dim) if field in (_lib.FIELD_S, _lib.FIELD_SH) else (self.dim,)
        return value + tuple(self.n[a] * fr.m[a] for a in reversed(range(self.dim)) if not fr.fixed[a])

    def get_frame_dev(self, field, m=1, slice=None, out=None, dtype=None):
        """A field rastered on a pixel lattice aligned with the block's cubes, as a torch tensor on the block's device: `m`
        pixels per cube along every axis (an int or a per-axis tuple), `slice` = {axis: coordinate} for the plane x_axis =
        coordinate.  Shape: value shape + (P_{d-1}, ..., P_0), P_a = n_a * m_a, the sliced axes dropped; float64 or float32
        (`dtype`, default float64, or that of `out`).  `out` may be a strided view - several blocks write into views of
        one image - whose value axes of a stress are laid out row-major (stride of i = dim * stride of j).  Queued like
        get_field_dev: on the block's stream between torch's current stream before and after, no host wait (a frame
        specification the block has not just used builds its tables first).  A block that does not hold a slice's layer
        leaves `out` as it is."""
        import torch
        fr = make_frame(self.dim, m, slice)
        shape = self.frame_shape(field, m, slice)
        if out is None:
            out = torch.empty(shape, dtype=dtype or torch.float64, device=self._torch_device())
        elif dtype is not None and out.dtype != dtype:
            raise ValueError("out is %s, dtype asks for %s" % (out.dtype, dtype))
        if not isinstance(out, torch.Tensor) or out.device != self._torch_device() or out.dtype not in (torch.float64, torch.float32) \
                or tuple(out.shape) != tuple(shape):
            raise ValueError("get_frame_dev takes a float64 or float32 tensor of shape %r on %s" % (tuple(shape), self._torch_device()))
        st = [int(s) for s in out.stride()]
        nv = len(shape) - sum(1 for a in range(self.dim) if not fr.fixed[a])
        if nv == 2 and self.dim > 1 and st[0] != self.dim * st[1]:
            raise ValueError("get_frame_dev: the value axes of `out` must be row-major (stride of i = dim * stride of j)")
        if any(s < 0 for s in st):
            raise ValueError("get_frame_dev: negative strides")
        axis = {}
        for k, a in enumerate(a for a in reversed(range(self.dim)) if not fr.fixed[a]):
            axis[a] = st[nv + k]
        stride = (C.c_int64 * 4)(st[nv - 1], axis.get(2, 0), axis.get(1, 0), axis.get(0, 0))
        nbytes = out.untyped_storage().nbytes() - out.storage_offset() * out.element_size()
        code = 1 if out.dtype == torch.float32 else 0
        self._on_stream(out, lambda: check(self.lib.sg_get_frame_dev(self.h, int(field), C.byref(fr), C.c_void_p(out.data_ptr()), code,
                                                                     stride, nbytes), self.h))
        return out

    # ---- gradient (sg_get_gradient_dev / sg_get_gradient) ------------------------------------------------------
    def gradient_shape(self, kind, ncells=None):
        """[ncells, nd] + the value shape of a kind: (dim, dim) of "grad" and "strain", () of "div", (3,) / () of "curl"""
        k = gradient_kind(kind)
        d = self.dim
        if k == 2 and d == 1:
            raise ValueError("no curl in one dimension")
        value = {0: (d, d), 1: (), 2: (3,) if d == 3 else (), 3: (d, d)}[k]
        return (self.ncells if ncells is None else int(ncells), self.nd) + value

    def get_gradient_dev(self, field, kind, out=None, dtype=None, cell0=0, ncells=None):
        """The broken gradient of a velocity field (FIELD_U, FIELD_UH) at the nodes of cells cell0 .. cell0 + ncells - 1, or
        its divergence, curl or symmetric part (`kind`: 0 / "grad", 1 / "div", 2 / "curl", 3 / "strain"), as a torch tensor of
        gradient_shape(kind, ncells) on the block's device, float64 or float32.  Queued like get_field_dev: on the block's
        stream between torch's current stream before and after, no host wait."""
        import torch
        k = gradient_kind(kind)
        ncells = self.ncells - int(cell0) if ncells is None else int(ncells)
        shape = self.gradient_shape(k, ncells)
        if out is None:
            out = torch.empty(shape, dtype=dtype or torch.float64, device=self._torch_device())
        elif dtype is not None and out.dtype != dtype:
            raise ValueError("out is %s, dtype asks for %s" % (out.dtype, dtype))
        code = self._dev_tensor(out, shape, "get_gradient_dev")
        nbytes = out.numel() * out.element_size()
        self._on_stream(out, lambda: check(self.lib.sg_get_gradient_dev(self.h, int(field), k, int(cell0), ncells,
                                                                        C.c_void_p(out.data_ptr()), code, nbytes), self.h))
        return out

    def get_gradient(self, field, kind, cell0=0, ncells=None):
        """get_gradient_dev as a float64 numpy array, through a temporary device buffer and one blocking copy"""
        k = gradient_kind(kind)
        ncells = self.ncells - int(cell0) if ncells is None else int(ncells)
        out = np.empty(self.gradient_shape(k, ncells))
        check(self.lib.sg_get_gradient(self.h, int(field), k, int(cell0), ncells, out.ctypes.data, out.nbytes), self.h)
        return out

    def set_params(self, density, dt, lam, mu):
        lam_a, mu_a = _f64(np.atleast_1d(lam)).ravel(), _f64(np.atleast_1d(mu)).ravel()
        per_cell = int(lam_a.size > 1 or mu_a.size > 1)
        if per_cell:
            lam_a = _f64(np.broadcast_to(lam_a, (self.ncells,)))
            mu_a = _f64(np.broadcast_to(mu_a, (self.ncells,)))
        check(self.lib.sg_set_params(self.h, float(density), float(dt), lam_a.ctypes.data, mu_a.ctypes.data,
                                     per_cell), self.h)

    def set_density(self, rho, physical=False):
        """Scalar or per-cell density; physical=False: the explicit reference's u1 = rho*u0 + ...,
        True: u1 = u0 + (...)/rho (include/seigen_hip.h, sg_set_density)."""
        rho_a = _f64(np.atleast_1d(rho)).ravel()
        per_cell = int(rho_a.size > 1)
        if per_cell and rho_a.size != self.ncells:
            raise ValueError("per-cell density needs one value per cell of the block (%d), got %d" % (self.ncells, rho_a.size))
        check(self.lib.sg_set_density(self.h, rho_a.ctypes.data, per_cell, int(bool(physical))), self.h)

    def is_sym(self):
        v = C.c_int()
        check(self.lib.sg_get_sym(self.h, C.byref(v)), self.h)
        return bool(v.value)

    def leave_sym(self):
        check(self.lib.sg_leave_sym(self.h), self.h)

    def set_absorption(self, sigma_nodes, sigma_degree):
        if sigma_nodes is None:
            check(self.lib.sg_set_absorption(self.h, None, 0), self.h)
            return
        s = _f64(sigma_nodes).reshape(self.ncells, -1)
        check(self.lib.sg_set_absorption(self.h, s.ctypes.data, int(sigma_degree)), self.h)

    def set_source(self, nodes, values, static=False):
        """nodes: flat scalar node indices [nnz]; values [nsteps, nnz, d, d] for the next nsteps steps,
        or (static=True) [1, nnz, d, d] holding at every step."""
        nodes = np.ascontiguousarray(nodes, dtype=np.int64).ravel()
        if nodes.size == 0 or values is None or len(values) == 0:
            check(self.lib.sg_set_source(self.h, 0, None, 0, None), self.h)
            return
        values = _f64(values).reshape(-1, nodes.size, self.dim, self.dim)
        if static and values.shape[0] != 1:
            raise ValueError("a static source is one time slice")
        check(self.lib.sg_set_source(self.h, nodes.size, nodes.ctypes.data, -1 if static else values.shape[0],
                                     values.ctypes.data), self.h)

    def set_source_box_ricker(self, lo, hi, a, t0, t_first, dt_step, nsteps):
        """The reference's box-Ricker source from its parameters (sg_set_source_box_ricker, include/seigen_hip.h)."""
        lo, hi = _f64(lo).ravel(), _f64(hi).ravel()
        if lo.size != self.dim or hi.size != self.dim:
            raise ValueError("lo and hi hold one coordinate per dimension")
        check(self.lib.sg_set_source_box_ricker(self.h, lo.ctypes.data, hi.ctypes.data, float(a), float(t0),
                                                float(t_first), float(dt_step), int(nsteps)), self.h)

    def set_source_separable(self, nodes, pattern, weights):
        """S(node, step k) = weights[k] * pattern[node]: nodes [nnz], pattern [nnz, d, d], weights [nsteps]."""
        nodes = np.ascontiguousarray(nodes, dtype=np.int64).ravel()
        weights = _f64(weights).ravel()
        if nodes.size == 0 or weights.size == 0:
            check(self.lib.sg_set_source(self.h, 0, None, 0, None), self.h)
            return
        pattern = _f64(pattern).reshape(nodes.size, self.dim, self.dim)
        check(self.lib.sg_set_source_separable(self.h, nodes.size, nodes.ctypes.data, pattern.ctypes.data, weights.size,
                                               weights.ctypes.data), self.h)

    # ---- hot path ---------------------------------------------------------------------
    def step(self, nsteps=1):
        check(self.lib.sg_step(self.h, int(nsteps)), self.h)

    def run_stage(self, stage, region=_lib.REGION_ALL):
        check(self.lib.sg_run_stage(self.h, int(stage), int(region)), self.h)

    def end_step(self):
        """End a host-driven step.  Returns whether an armed stress series added an entry to s1: a host that exchanges the
        halo itself sends the traces of s1 again before the next step (include/seigen_hip.h)."""
        due = self._inj is not None and (self._inj[0] & 2) and self.injector_entries_left() > 0
        check(self.lib.sg_end_step(self.h), self.h)
        return bool(due)

    def injector_entries_left(self):
        """Entries of the armed series not added yet: entry k goes in at the end of step k + 1 counted from the arming
        call, and the steps are the library's own count (sg_get_counters: sg_step and sg_end_step alike)."""
        if self._inj is None:
            return 0
        what, entries, at = self._inj
        return max(0, entries - (self.counters()["steps"] - at))

    # ---- injectors (sg_inject / sg_set_injectors) -------------------------------------------------
    def _ncomp(self, what):
        if int(what) not in (1, 2, 3):
            raise ValueError("what is 1 (velocity), 2 (stress) or 3 (both)")
        return (self.dim if what & 1 else 0) + (self.dim * self.dim if what & 2 else 0)

    def inject(self, points, amp, what=1):
        """field += amp at the physical `points` [npts, dim], once, behind everything queued: amp [npts, ncomp] holds per
        point the velocity's dim values (what bit 0) and then the stress's dim * dim (bit 1).  Every block of a mesh is
        handed all points and adds the ones it owns."""
        pts = _f64(points).reshape(-1, self.dim)
        amp = _f64(amp).reshape(len(pts), self._ncomp(what))
        check(self.lib.sg_inject(self.h, len(pts), pts.ctypes.data, int(what), amp.ctypes.data), self.h)

    def set_injectors(self, points, series, what=1):
        """Arm a series at `points` [npts, dim]: series[k] [npts, ncomp] is added at the end of step k + 1 counted from
        this call.  No points or no entries: disarm.  Returns owned [npts] (bool)."""
        pts = _f64(points).reshape(-1, self.dim)
        nsteps = 0 if series is None else len(series)
        if len(pts) == 0 or nsteps == 0:
            check(self.lib.sg_set_injectors(self.h, 0, None, 0, 0, None, None), self.h)
            self._inj = None
            return np.zeros(len(pts), dtype=bool)
        amp = _f64(series).reshape(nsteps, len(pts), self._ncomp(what))
        owned = np.zeros(len(pts), dtype=np.int32)
        check(self.lib.sg_set_injectors(self.h, len(pts), pts.ctypes.data, int(what), nsteps, amp.ctypes.data,
                                        owned.ctypes.data), self.h)
        self._inj = (int(what), nsteps, self.counters()["steps"])
        return owned.astype(bool)

    # ---- receivers (sg_set_receivers / sg_get_receivers) ----------------------------------------
    def set_receivers(self, points, what=1, every=1, capacity=0):
        """Arm receivers at `points` [nrec, dim] - all of the mesh's: the block records the ones it owns - sampling the
        velocity (what bit 0) and / or the stress (bit 1) after every `every`-th step, room for `capacity` samples.
        No points: disarm.  Returns owned [nrec] (bool)."""
        pts = _f64(points).reshape(-1, self.dim)
        owned = np.zeros(len(pts), dtype=np.int32)
        check(self.lib.sg_set_receivers(self.h, len(pts), pts.ctypes.data, int(what), int(every), int(capacity),
                                        owned.ctypes.data), self.h)
        ncomp = (self.dim if what & 1 else 0) + (self.dim * self.dim if what & 2 else 0)
        self._rec_shape = (int(capacity), len(pts), ncomp) if len(pts) else (0, 0, 0)
        return owned.astype(bool)

    def get_receivers(self):
        """The samples taken so far, [n, nrec, ncomp]: per receiver the velocity's dim values, then the stress's dim * dim
        (row-major); rows of receivers the block does not own are 0."""
        out = np.zeros(getattr(self, "_rec_shape", (0, 0, 0)))
        n = C.c_int64()
        check(self.lib.sg_get_receivers(self.h, out.ctypes.data, out.nbytes, C.byref(n)), self.h)
        return out[:n.value]

    # ---- gauges (sg_set_gauges / sg_get_gauges / sg_probe_gradient) ------------------------------------
    def gauge_shape(self, kind):
        """the value shape of a gauge of `kind`, flat: (ncomp,)"""
        return (int(np.prod(self.gradient_shape(kind, 0)[2:], dtype=np.int64)),)

    def set_gauges(self, points, kind=3, every=1, capacity=0):
        """Arm gauges at `points` [npts, dim] - all of the mesh's: the block records the ones it owns - sampling the broken
        gradient of the velocity u1, or its divergence, curl or symmetric part (`kind` as get_gradient_dev's), after every
        `every`-th step, room for `capacity` samples.  No points: disarm.  Returns owned [npts] (bool)."""
        pts = _f64(points).reshape(-1, self.dim)
        k = gradient_kind(kind) if len(pts) else 0
        ncomp = self.gauge_shape(k)[0] if len(pts) else 0
        owned = np.zeros(len(pts), dtype=np.int32)
        check(self.lib.sg_set_gauges(self.h, len(pts), pts.ctypes.data, k, int(every), int(capacity), owned.ctypes.data), self.h)
        self._gauge_shape = (int(capacity), len(pts), ncomp) if len(pts) else (0, 0, 0)
        return owned.astype(bool)

    def get_gauges(self):
        """The samples taken so far, [n, npts, ncomp] in the component order of get_gradient_dev; rows of gauges the block does
        not own are 0."""
        out = np.zeros(getattr(self, "_gauge_shape", (0, 0, 0)))
        n = C.c_int64()
        check(self.lib.sg_get_gauges(self.h, out.ctypes.data, out.nbytes, C.byref(n)), self.h)
        return out[:n.value]

    def probe_gradient(self, field, kind, points):
        """(values [npts, ncomp], owned [npts]): the gauges' arithmetic once, on `field` (FIELD_U, FIELD_UH) as it stands behind
        everything queued; rows of points the block does not own are 0 (sg_probe_gradient)."""
        pts = _f64(points).reshape(-1, self.dim)
        k = gradient_kind(kind)
        out = np.zeros((len(pts),) + self.gauge_shape(k))
        owned = np.zeros(len(pts), dtype=np.int32)
        check(self.lib.sg_probe_gradient(self.h, int(field), k, len(pts), pts.ctypes.data, out.ctypes.data, out.nbytes,
                                         owned.ctypes.data), self.h)
        return out, owned.astype(bool)

    # ---- monitor (sg_measure / sg_set_monitor / sg_get_monitor) ------------------------------------
    def _weights(self, w):
        """(pointer, per_cell, array kept alive) of the weights (wk, ws, wt): None, one triple, or [ncells, 3]"""
        if w is None:
            return None, 0, None
        w = _f64(w)
        if w.shape == (3,):
            return w.ctypes.data, 0, w
        if w.shape != (self.ncells, 3):
            raise ValueError("weights are one (wk, ws, wt) or one per cell of the block [%d, 3], not %r" % (self.ncells, w.shape))
        return w.ctypes.data, 1, w

    def measure(self, w=None):
        """One sample { U2, S2, T2, EK, ES } of u and s as they stand now, taken on the device (sg_measure)."""
        ptr, per_cell, keep = self._weights(w)
        out = np.zeros(5)
        check(self.lib.sg_measure(self.h, ptr, per_cell, out.ctypes.data), self.h)
        return out

    def set_monitor(self, every, capacity, w=None):
        """Arm the monitor: a sample after every `every`-th step, room for `capacity` samples; every = 0 disarms."""
        ptr, per_cell, keep = self._weights(w)
        check(self.lib.sg_set_monitor(self.h, int(every), int(capacity), ptr, per_cell), self.h)
        self._mon_capacity = int(capacity) if int(every) > 0 else 0

    def get_monitor(self):
        """The samples taken so far, [n, 5]."""
        out = np.zeros((getattr(self, "_mon_capacity", 0), 5))
        n = C.c_int64()
        check(self.lib.sg_get_monitor(self.h, out.ctypes.data, out.nbytes, C.byref(n)), self.h)
        return out[:n.value]

    # ---- correlation (sg_correlate / sg_get_correlation / sg_reset_correlation) -----------------------
    def correlate(self, other, w=None):
        """acc[c] += w * |det J| * (Buu_c, Bss_c, Btt_c) of this block's (u, s) against `other`'s (another HipBlock of the
        same shape on the same device, or this one), cell by cell on the device (sg_correlate); w: one triple, None = 1."""
        if w is not None:
            w = _f64(w)
            if w.shape != (3,):
                raise ValueError("weights are one (w_uu, w_ss, w_tt), not %r" % (w.shape,))
        check(self.lib.sg_correlate(self.h, other.h, None if w is None else w.ctypes.data), self.h)

    def get_correlation(self):
        """The accumulator [ncells, 3] = (uu, ss, tt) in host cell order."""
        out = np.empty((self.ncells, 3))
        check(self.lib.sg_get_correlation(self.h, out.ctypes.data, out.nbytes), self.h)
        return out

    def reset_correlation(self, release=False):
        """Zero the accumulator; release: free it (get_correlation then raises until the next correlate)."""
        check(self.lib.sg_reset_correlation(self.h, int(bool(release))), self.h)

    # ---- spectra (sg_set_spectra / sg_get_spectrum / sg_spectra_samples / sg_correlate_spectra) ---------
    def set_spectra(self, wu=None, ws=None, every=1):
        """Arm running Fourier transforms: sample j is taken after step (j + 1) * every counted from this call, behind the
        recorder and the monitor and before the injectors, and adds w[j][f] * field to accumulator f.  wu / ws: the complex
        weights [nsamples, nfreq] of the velocity / the stress (or real [nsamples, nfreq, 2]); None: the field is not
        selected.  Both None: disarm and free."""
        tabs = []
        for w in (wu, ws):
            if w is None:
                tabs.append(None)
                continue
            w = np.asarray(w)
            if np.iscomplexobj(w):
                w = np.stack([w.real, w.imag], axis=-1)
            w = _f64(w)
            if w.ndim != 3 or w.shape[2] != 2:
                raise ValueError("weights are complex [nsamples, nfreq] or real [nsamples, nfreq, 2], not %r" % (w.shape,))
            tabs.append(w)
        given = [w for w in tabs if w is not None]
        if not given:
            check(self.lib.sg_set_spectra(self.h, 0, 0, 1, 0, None, None), self.h)
            self._spc = None
            return
        if len(given) == 2 and given[0].shape != given[1].shape:
            raise ValueError("the two weight tables differ in shape: %r and %r" % (given[0].shape, given[1].shape))
        nsamples, nfreq = given[0].shape[:2]
        what = (1 if tabs[0] is not None else 0) | (2 if tabs[1] is not None else 0)
        check(self.lib.sg_set_spectra(self.h, int(nfreq), what, int(every), int(nsamples),
                                      None if tabs[0] is None else tabs[0].ctypes.data,
                                      None if tabs[1] is None else tabs[1].ctypes.data), self.h)
        self._spc = (what, int(nfreq))

    def get_spectrum(self, field, freq):
        """The accumulator of frequency `freq` of the velocity (field 0 / FIELD_U) or the stress (1 / FIELD_S) as a complex
        array of the field's host shape."""
        k = {0: 0, 1: 1, _lib.FIELD_S: 1}[int(field)]
        shape = self.field_shape(_lib.FIELD_S if k else _lib.FIELD_U)
        re, im = np.empty(shape), np.empty(shape)
        check(self.lib.sg_get_spectrum(self.h, k, int(freq), 0, re.ctypes.data, re.nbytes), self.h)
        check(self.lib.sg_get_spectrum(self.h, k, int(freq), 1, im.ctypes.data, im.nbytes), self.h)
        return re + 1j * im

    def spectra_samples(self):
        """Samples taken since the arming call (0: nothing armed)."""
        n = C.c_int64()
        check(self.lib.sg_spectra_samples(self.h, C.byref(n)), self.h)
        return int(n.value)

    def correlate_spectra(self, other, f, f_other=None, w=None, z=1.0):
        """acc[c] += w * |det J| * Re(z conj(a^_f) . b^_f_other) in the forms (uu, ss, tt) of correlate(), of this block's
        spectra against `other`'s, into the accumulator of correlate() (get_correlation / reset_correlation)."""
        if w is not None:
            w = _f64(w)
            if w.shape != (3,):
                raise ValueError("weights are one (w_uu, w_ss, w_tt), not %r" % (w.shape,))
        z = complex(z)
        zz = _f64([z.real, z.imag])
        check(self.lib.sg_correlate_spectra(self.h, int(f), other.h, int(f if f_other is None else f_other),
                                            None if w is None else w.ctypes.data, zz.ctypes.data), self.h)

    # ---- peak maps (sg_set_peaks / sg_get_peaks / sg_get_peaks_dev / sg_peaks_samples) -----------------------
    def set_peaks(self, what, every=1, nsamples=1):
        """Arm the peak maps: bit 0 of `what` the velocity (|u|^2), bit 1 the stress (s:s).  Sample j is taken after step
        (j + 1) * every counted from this call, behind the spectra and before the injectors; every node keeps the largest
        squared magnitude and the sample that reached it, `nsamples` samples long.  what = 0: disarm and free."""
        check(self.lib.sg_set_peaks(self.h, int(what), int(every), int(nsamples)), self.h)

    def get_peaks(self, field):
        """(value, sample) of the velocity (field 0 / FIELD_U) or the stress (1 / FIELD_S): value[ncells, nd] the maxima of the
        SQUARES (float64), sample[ncells, nd] the 0-based sample that reached them (int32; -1: never above zero)."""
        k = {0: 0, 1: 1, _lib.FIELD_S: 1}[int(field)]
        value = np.empty((self.ncells, self.nd))
        sample = np.empty((self.ncells, self.nd), dtype=np.int32)
        check(self.lib.sg_get_peaks(self.h, k, value.ctypes.data, sample.ctypes.data, value.size), self.h)
        return value, sample

    def get_peaks_dev(self, field, dtype=None):
        """get_peaks as torch tensors on the block's device (value float64 or float32, sample int32), moved on the device:
        queued on the block's stream between torch's current stream before and after, as get_field_dev."""
        import torch
        k = {0: 0, 1: 1, _lib.FIELD_S: 1}[int(field)]
        shape = (self.ncells, self.nd)
        value = torch.empty(shape, dtype=dtype or torch.float64, device=self._torch_device())
        sample = torch.empty(shape, dtype=torch.int32, device=self._torch_device())
        code = self._dev_tensor(value, shape, "get_peaks_dev")
        self._on_stream(value, lambda: check(self.lib.sg_get_peaks_dev(self.h, k, C.c_void_p(value.data_ptr()), code,
                                                                       C.c_void_p(sample.data_ptr()), value.numel()), self.h))
        sample.record_stream(torch.cuda.current_stream(self._device))
        return value, sample

    def peaks_samples(self):
        """Samples taken since the arming call (0: nothing armed)."""
        n = C.c_int64()
        check(self.lib.sg_peaks_samples(self.h, C.byref(n)), self.h)
        return int(n.value)

    def apply_F(self, s_in, u_abs, u_out):
        check(self.lib.sg_apply_F(self.h, s_in, u_abs, u_out), self.h)

    def apply_G(self, u_in, s_out, use_source=False):
        check(self.lib.sg_apply_G(self.h, u_in, s_out, int(use_source)), self.h)

    def sync(self):
        check(self.lib.sg_sync(self.h), self.h)

    def last_step_ms(self):
        ms = C.c_double()
        check(self.lib.sg_last_step_ms(self.h, C.byref(ms)), self.h)
        return ms.value

    def enable_timing(self, on=True):
        check(self.lib.sg_enable_timing(self.h, int(on)), self.h)

    def counters(self):
        c = SgCounters()
        check(self.lib.sg_get_counters(self.h, C.byref(c)), self.h)
        return dict(kernel_ms=list(c.kernel_ms), launches=list(c.launches), steps=int(c.steps),
                    halo_pack_ms=float(c.halo_pack_ms), halo_pack_launches=int(c.halo_pack_launches),
                    halo_bytes_packed=int(c.halo_bytes_packed))

    def stage_kernel_name(self, stage, region=0, short=True):
        """The kernel a launch of `stage` over `region` runs, named by the library itself (sg_stage_kernel_name): as
        rocprofv3 prints it, or (short) without the `void ` in front and the argument list behind."""
        buf = C.create_string_buffer(512)
        check(self.lib.sg_stage_kernel_name(self.h, int(stage), int(region), buf, len(buf)), self.h)
        name = buf.value.decode()
        if short:
            if name.startswith("void "):
                name = name[5:]
            if name.endswith(")") and "(" in name:
                name = name[:name.rindex("(")]
        return name

    # ---- halo ---------------------------------------------------------------------------
    def halo_bytes(self, field, side):
        nb = C.c_size_t()
        check(self.lib.sg_halo_bytes(self.h, field, side, C.byref(nb)), self.h)
        return nb.value

    def halo_pack(self, field, side, dev_ptr):
        check(self.lib.sg_halo_pack(self.h, field, side, C.c_void_p(dev_ptr)), self.h)

    def halo_pack_sides(self, field, ptrs):
        """ptrs: {side: device pointer}; every listed side in one launch."""
        arr = (C.c_void_p * 6)(*[C.c_void_p(ptrs.get(s)) if ptrs.get(s) else None for s in range(6)])
        check(self.lib.sg_halo_pack_sides(self.h, int(field), arr), self.h)

    # ---- native exchange over RCCL (csrc/comm.cpp): step() then runs the whole pipelined schedule in the library
    def comm_init(self, unique_id, rank, nranks, peers):
        """peers: rank of the face neighbour per block side (2 * axis + hi), -1 / None where there is none."""
        buf = C.create_string_buffer(bytes(unique_id), _lib.COMM_ID_BYTES)
        _lib.check(self.lib.sg_comm_init(self.h, buf, _lib.COMM_ID_BYTES, int(rank), int(nranks), self._peer_array(peers)), self.h)

    def _peer_array(self, peers):
        return (C.c_int32 * 6)(*[(-1 if (i >= len(peers) or peers[i] is None) else int(peers[i])) for i in range(6)])

    def comm_check(self, rank, nranks, peers):
        """what sg_comm_init would refuse without talking to another rank (raises); call on every rank and agree on the
        outcome before the collective comm_init"""
        _lib.check(self.lib.sg_comm_check(self.h, int(rank), int(nranks), self._peer_array(peers)), self.h)

    def comm_selftest(self):
        """collective: pattern exchange; number of values that did not arrive from the facing side of the right neighbour"""
        bad = C.c_int64()
        _lib.check(self.lib.sg_comm_selftest(self.h, C.byref(bad)), self.h)
        return int(bad.value)

    def comm_finalize(self):
        _lib.check(self.lib.sg_comm_finalize(self.h), self.h)

    def comm_stats(self, reset=False):
        st = _lib.SgCommStats()
        _lib.check(self.lib.sg_comm_get_stats(self.h, C.byref(st), 1 if reset else 0), self.h)
        return {"exchanges": int(st.exchanges), "bytes_sent": int(st.bytes_sent), "exposed_wait_ms": float(st.exposed_wait_ms)}

    def comm_exchange(self, field):
        _lib.check(self.lib.sg_comm_exchange(self.h, field), self.h)

    def comm_buffers(self, kind, side):
        """(send pointer, receive pointer, bytes) of a side's device buffers; kind 0: velocity-like, 1: stress-like."""
        a, b, n = C.c_void_p(), C.c_void_p(), C.c_size_t()
        _lib.check(self.lib.sg_comm_buffers(self.h, kind, side, C.byref(a), C.byref(b), C.byref(n)), self.h)
        return a.value, b.value, n.value

    def halo_attach(self, field, side, dev_ptr):
        check(self.lib.sg_halo_attach(self.h, field, side, C.c_void_p(dev_ptr)), self.h)
