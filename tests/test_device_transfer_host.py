"""CPU-only tests of the device transfers (include/seigen_hip.h sg_get_field_dev / sg_set_field_dev / sg_get_spectrum_dev):
the kernel objects of namespace sg::xfer in the built library are the listed ones, each with the GPU row that launches it;
the launch plan (sg_xfer_plan, hostlogic.hpp xfer_plan) covers every (cell of the range, row) exactly once and nothing else,
within the LDS a block gets and the grid's cap - walked for small blocks, by arithmetic for one past 2^31 words; the entry
points refuse a null handle or buffer without a device."""
import os
import re
import subprocess

import numpy as np
import pytest

from seigen_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Every kernel object of namespace sg::xfer (kernels_xfer.hip) with the rows of tests/test_device_transfer_gpu.py that launch
# it.  tests/test_host_logic.py pins the objects named sg::name(; this list keeps the same rule for the nested namespace.
XFER_KERNELS = {
    "sg::xfer::tiled<double, double, 0>": "set, double tensor: every f64 row with gw = 16 or 64 (mfma-*, tile-*, hexm-*, lane-*, hex-DQ2-lane)",
    "sg::xfer::tiled<double, double, 1>": "get, double tensor: the same rows; spectra of every interleaved row, f32 ones included",
    "sg::xfer::tiled<double, float, 0>": "set, float tensor: the same rows",
    "sg::xfer::tiled<double, float, 1>": "get, float tensor: the same rows",
    "sg::xfer::tiled<float, double, 0>": "set, double tensor: rows mfma-P3-f32, tile-tri-P3-f32, tile-tri-P3-f32-groups",
    "sg::xfer::tiled<float, double, 1>": "get, double tensor: the f32 rows",
    "sg::xfer::tiled<float, float, 0>": "set, float tensor: the f32 rows",
    "sg::xfer::tiled<float, float, 1>": "get, float tensor: the f32 rows",
    "sg::xfer::flat<double, float, 0>": "set, float tensor: row generic-2d-P2 (double tensors are a device-to-device copy)",
    "sg::xfer::flat<double, float, 1>": "get, float tensor: row generic-2d-P2",
}


def _head(sig):
    """a demangled signature up to the `(` that opens the argument list, template arguments skipped"""
    depth = 0
    for i, c in enumerate(sig):
        if c == "<":
            depth += 1
        elif c == ">":
            depth -= 1
        elif c == "(" and depth == 0:
            return sig[:i]
    return sig


def _xfer_objects():
    readelf = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "llvm-readelf")
    assert os.path.exists(readelf), "llvm-readelf (shipped with ROCm) not found at %s: set ROCM_PATH" % readelf
    out = subprocess.run([readelf, "--dyn-syms", "--demangle", _lib.lib_path()], capture_output=True, text=True, check=True).stdout
    found = []
    for line in out.splitlines():
        f = line.split(None, 7)
        if len(f) < 8 or f[3] != "OBJECT":
            continue
        head = _head(f[7])
        if "sg::xfer::" in head:
            found.append(head[head.index("sg::xfer::"):])
    return found


def test_xfer_kernel_objects_are_the_listed_ones():
    found = _xfer_objects()
    assert len(found) == len(set(found)), "a kernel object appears twice"
    assert not set(found) - set(XFER_KERNELS), "in the library but not listed: %s" % sorted(set(found) - set(XFER_KERNELS))
    assert not set(XFER_KERNELS) - set(found), "listed but not in the library: %s" % sorted(set(XFER_KERNELS) - set(found))
    assert all(XFER_KERNELS.values())


def _cap():
    hdr = open(os.path.join(ROOT, "include", "seigen_hip.h")).read()
    return int(re.search(r"#define SG_XFER_GRID_CAP (\d+)", hdr).group(1))


def _plan(gw, ncls, nd, ncomp, dev_bytes, caller_bytes, cell0, ncells):
    out = np.zeros(6, dtype=np.int64)
    rc = _lib.load().sg_xfer_plan(gw, ncls, nd, ncomp, dev_bytes, caller_bytes, cell0, ncells, out.ctypes.data)
    assert rc == 0
    return dict(zip(("item0", "nitems", "rows_per_slice", "slices", "grid", "lds"), (int(x) for x in out)))


# (ncls, nd, ncomp) of the velocity and the stress of every row of tests/test_device_transfer_gpu.py
SHAPES = sorted({
    (6, 35, 3), (6, 35, 9),     # 3-D P4
    (6, 20, 3), (6, 20, 9),     # 3-D P3
    (2, 10, 2), (2, 10, 4),     # triangles P3
    (1, 9, 2), (1, 9, 4),       # quadrilaterals P2
    (1, 64, 3), (1, 64, 9),     # hexahedra DQ_3
    (2, 6, 2), (2, 6, 4),       # triangles P2
    (1, 27, 3), (1, 27, 9),     # hexahedra DQ_2: 243 rows of 64 lanes, the item that must be sliced
})


def _ranges(gw, ncls, ncube):
    """whole block; start and end inside a cube; inside a group and across a group boundary; one cell; the last cells"""
    n = ncube * ncls
    r = [(0, n), (1, n - 2), (n - 1, 1), (0, 1)]
    if gw > 1:
        r += [(gw * ncls - 3, 7), (gw * ncls + 1, ncls + 1), (3 * ncls + ncls // 2, 2 * ncls), (gw * ncls, gw * ncls)]
    return sorted({(max(0, c0), min(k, n - max(0, c0))) for c0, k in r if k > 0 and max(0, c0) < n})


@pytest.mark.parametrize("gw", [1, 16, 64])
@pytest.mark.parametrize("dev_bytes", [8, 4])
def test_plan_covers_the_range_exactly_once(gw, dev_bytes):
    cap = _cap()
    for ncls, nd, ncomp in SHAPES:
        rows = nd * ncomp
        ncube = 2 * gw + 5 if gw > 1 else 37     # three groups, the last one partly padding
        for cell0, ncells in _ranges(gw, ncls, ncube):
            p = _plan(gw, ncls, nd, ncomp, dev_bytes, 8, cell0, ncells)
            assert p["lds"] <= 65536 and 1 <= p["grid"] <= cap, p
            assert p == _plan(gw, ncls, nd, ncomp, dev_bytes, 4, cell0, ncells)     # the image is in the block's type
            if gw == 1:
                assert (p["item0"], p["nitems"], p["lds"]) == (cell0, ncells, 0)
                assert p["grid"] == min(cap, -(-ncells * rows // 256))
                continue
            assert p["lds"] == p["rows_per_slice"] * (gw + 1) * dev_bytes
            assert p["grid"] == min(cap, p["nitems"] * p["slices"])
            # the kernel's walk: unit (item, slice), lane w of the item is cell ((item // ncls) * gw + w) * ncls + item % ncls
            hits = np.zeros((ncube * ncls + 2 * gw * ncls, rows), dtype=np.int32)
            for item in range(p["item0"], p["item0"] + p["nitems"]):
                cells = ((item // ncls) * gw + np.arange(gw)) * ncls + item % ncls
                cells = cells[(cells >= cell0) & (cells < cell0 + ncells)]
                for s in range(p["slices"]):
                    r0 = s * p["rows_per_slice"]
                    assert r0 < rows, "an empty slice"
                    hits[np.ix_(cells, np.arange(r0, min(rows, r0 + p["rows_per_slice"])))] += 1
            want = np.zeros_like(hits)
            want[cell0:cell0 + ncells] = 1
            assert np.array_equal(hits, want), (gw, ncls, nd, ncomp, cell0, ncells, p)


def test_plan_of_an_empty_range_and_bad_arguments():
    p = _plan(16, 6, 35, 9, 8, 8, 5, 0)
    assert p["grid"] == 0 and p["nitems"] == 0
    out = np.zeros(6, dtype=np.int64)
    L = _lib.load()
    for args in ((3, 6, 35, 9, 8, 8, 0, 1), (16, 0, 35, 9, 8, 8, 0, 1), (16, 6, 35, 9, 2, 8, 0, 1), (16, 6, 35, 9, 8, 3, 0, 1),
                 (16, 6, 35, 9, 8, 8, -1, 1), (16, 6, 35, 9, 8, 8, 0, -1)):
        assert L.sg_xfer_plan(*args, out.ctypes.data) == -1, args
    assert L.sg_xfer_plan(16, 6, 35, 9, 8, 8, 0, 1, None) == -1


@pytest.mark.parametrize("gw,ncls,nd,ncomp", [(16, 6, 35, 9), (64, 1, 27, 9), (1, 2, 6, 4)])
def test_plan_past_2_31_words_by_arithmetic(gw, ncls, nd, ncomp):
    """a block of 2.2e9 stress words: nothing is allocated, the plan's numbers are checked against the layout's"""
    rows = nd * ncomp
    ncells = -(-2200000000 // rows)
    assert ncells * rows >= 2.2e9 > 2 ** 31
    cap = _cap()
    for cell0, k in ((0, ncells), (ncells - 1000, 1000), (12345, ncells - 23456)):
        p = _plan(gw, ncls, nd, ncomp, 8, 8, cell0, k)
        assert p["lds"] <= 65536 and 1 <= p["grid"] <= cap
        if gw == 1:
            assert (p["item0"], p["nitems"]) == (cell0, k) and p["grid"] == min(cap, -(-k * rows // 256))
            continue
        first, last = cell0 // ncls // gw, (cell0 + k - 1) // ncls // gw            # groups of the first and the last cell
        assert p["item0"] == first * ncls and p["nitems"] == (last - first + 1) * ncls
        assert (p["slices"] - 1) * p["rows_per_slice"] < rows <= p["slices"] * p["rows_per_slice"]
        assert p["grid"] == min(cap, p["nitems"] * p["slices"])
        assert (p["item0"] + p["nitems"]) * rows * gw >= (cell0 + k) * rows        # the last word lies in the last item


def test_entry_points_refuse_null_handle_and_null_buffer_without_a_device():
    L = _lib.load()
    buf = np.zeros(8)
    for name in ("sg_get_field_dev", "sg_set_field_dev", "sg_get_spectrum_dev"):
        assert name in _lib.SYMBOLS and hasattr(L, name)
    assert L.sg_get_field_dev(None, 0, 0, 1, buf.ctypes.data, 0, 64) == -1
    assert L.sg_set_field_dev(None, 0, 0, 1, buf.ctypes.data, 0, 64) == -1
    assert L.sg_get_spectrum_dev(None, 0, 0, 0, buf.ctypes.data, 0, 64) == -1
    assert L.sg_get_field_dev(None, 0, 0, 1, None, 0, 64) == -1
    assert L.sg_set_field_dev(None, 0, 0, 1, None, 0, 64) == -1
    assert L.sg_get_spectrum_dev(None, 0, 0, 0, None, 0, 64) == -1
