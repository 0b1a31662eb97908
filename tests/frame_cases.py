"""Blocks, frames and the host-side restatement shared by tests/test_frame_host.py and tests/test_frame_gpu.py (a helper, no
test itself).  A frame (include/seigen_hip.h sg_frame) is written (m, slice) as HipBlock.get_frame_dev takes it."""
import numpy as np

from seigen_amd.backend import frame_plan, frame_weights, make_frame
from tests.test_injectors_host import make_cfg, nodes_of


def block_cfg(dim, degree, n, diagonal="left", cube0=None, mesh_n=None):
    """the SgConfig of a block of n cubes with h = 1 / (the mesh's cubes): the unit box where the block is the mesh"""
    mesh_n = n if mesh_n is None else mesh_n
    cfg = make_cfg(dim, degree, n, [1.0 / k for k in mesh_n], diagonal == "quadrilateral", cube0=cube0)
    cfg.diagonal = {"left": 0, "right": 1, "quadrilateral": 2}[diagonal]
    return cfg


def frames_of(dim, n):
    """the frames the tests walk on a block of the unit box with n cubes: (m, slice) pairs"""
    if dim == 1:
        return [(1, None), (4, None), (8, None)]
    if dim == 2:
        return [(1, None), ((2, 3), None), (4, None)]
    out = [((2, 2, 2), None)]
    nz = n[2]
    for z in (0.4 / nz,                 # inside the first layer of cubes
              1.0 / nz,                 # an interior grid plane: the lower layer
              0.0, 1.0):                # both mesh faces
        out.append(((2, 2, 1), {2: z}))
    out.append(((3, 1, 2), {1: 1.0 / n[1]}))      # a y slice on a grid plane
    out.append(((1, 2, 2), {0: 2.5 / n[0]}))      # an x slice through the middle of a cube: every group holds cubes of it
    return out


def pixels(cfg, m, slice):
    """Every pixel of the frame on the block: dict of P (extents, axis order 0, 1, 2), cube [npix], q [npix], index [npix, 3]
    (p0, p1, p2), centre [npix, dim] (the physical pixel centres), owns."""
    d = cfg.dim
    fr = make_frame(d, m, slice)
    plan = frame_plan(cfg, fr)
    n = [cfg.n[a] for a in range(3)]
    mm = [1 if (a >= d or fr.fixed[a]) else fr.m[a] for a in range(3)]
    out = {"P": plan["P"], "Q": plan["Q"], "owns": plan["owns"], "plan": plan, "frame": fr}
    if not plan["owns"]:
        return out
    rng = []
    for a in range(3):
        if a < d and fr.fixed[a]:
            rng.append(np.array([plan["layer"][a]]))
        else:
            rng.append(np.arange(n[a]))
    c2, c1, c0, j2, j1, j0 = [x.ravel() for x in np.meshgrid(rng[2], rng[1], rng[0], np.arange(mm[2]), np.arange(mm[1]), np.arange(mm[0]),
                                                             indexing="ij")]
    c = [c0, c1, c2]
    j = [j0, j1, j2]
    out["cube"] = c0 + n[0] * (c1 + n[1] * c2)
    out["q"] = j0 + mm[0] * (j1 + mm[1] * j2)
    out["index"] = np.stack([np.zeros_like(c0) if (a < d and fr.fixed[a]) else c[a] * mm[a] + j[a] for a in range(3)], axis=-1)
    centre = np.empty((len(c0), d))
    for a in range(d):
        if fr.fixed[a]:
            centre[:, a] = fr.at[a]
        else:
            # the integers first, as the node coordinates of a block (sg_config::cube0)
            centre[:, a] = cfg.origin[a] + ((cfg.cube0[a] + c[a]).astype(np.float64) + (j[a] + 0.5) / mm[a]) * cfg.h[a]
    out["centre"] = centre
    return out


def host_frame(cfg, degree, quad, m, slice, values):
    """The frame of `values` [ncells, nd, comps...] (what sg_get_field returns) by the receivers' definition on the host:
    phi[q] @ values[cube * ncls + cls[q]], shaped comps + (P2, P1, P0); and the pixel table"""
    px = pixels(cfg, m, slice)
    nd = nodes_of(cfg.dim, degree, quad)
    cls, xi, phi = frame_weights(cfg, degree, px["frame"], nd)
    ncls = values.shape[0] // (cfg.n[0] * cfg.n[1] * cfg.n[2])
    cell = px["cube"] * ncls + cls[px["q"]]
    comps = values.shape[2:]
    v = values.reshape(values.shape[0], nd, -1)
    pix = np.einsum("pa,pac->pc", phi[px["q"]], v[cell])
    P = px["P"]
    img = np.zeros((v.shape[2], P[2], P[1], P[0]))
    i = px["index"]
    img[:, i[:, 2], i[:, 1], i[:, 0]] = pix.T
    px.update(cls=cls, xi=xi, phi=phi, cell=cell)
    return img.reshape(comps + (P[2], P[1], P[0])), px
