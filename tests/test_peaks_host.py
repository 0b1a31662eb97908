"""CPU-only tests of the peak maps (include/seigen_hip.h sg_set_peaks / sg_get_peaks / sg_get_peaks_dev / sg_peaks_samples):
the kernel objects of namespace sg::peak in the built library are the listed ones, each with the GPU rows that launch it; the
symbols are bound and refuse a NULL handle; and peak_reference, the numpy restatement of the device's arithmetic that
tests/test_peaks_gpu.py holds the maps equal to bit for bit, against a plain Python loop."""
import ctypes as C
import math

import numpy as np

from seigen_amd import _lib
from tests.test_spectra_host import _name_of

# Every kernel object of namespace sg::peak (kernels_peak.hip) with the rows of tests/test_peaks_gpu.py (ROWS: the nine of
# tests/gradient_loop.py and lane-1d-P2) that launch it: the rule of tests/test_spectra_host.py SPECTRA_KERNELS.
PEAK_KERNELS = {
    "sg::peak::update<double>": "test_bitwise_against_a_twin: rows mfma-P4-sym, mfma-P3-sym (symmetric lines), tile-*, hexm-DQ3, "
                                "lane-2d-P2, lane-1d-P2 (gw = 64), generic-2d-P2 (gw = 1: the scalar path)",
    "sg::peak::update<float>": "test_bitwise_against_a_twin: rows mfma-P3-f32 (symmetric lines), tile-tri-P3-f32",
    "sg::peak::gather<double>": "every get_peaks of tests/test_peaks_gpu.py, all rows; test_device_getter (float64)",
    "sg::peak::gather<float>": "test_device_getter of tests/test_peaks_gpu.py (float32)",
}


def _peak_objects():
    import os
    import subprocess
    readelf = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "llvm-readelf")
    assert os.path.exists(readelf), "llvm-readelf (shipped with ROCm) not found at %s: set ROCM_PATH" % readelf
    out = subprocess.run([readelf, "--dyn-syms", "--demangle", _lib.lib_path()], capture_output=True, text=True, check=True).stdout
    found = []
    for line in out.splitlines():
        f = line.split(None, 7)
        if len(f) < 8 or f[3] != "OBJECT":
            continue
        name = _name_of(f[7], "sg::peak::")
        if name:
            found.append(name)
    return found


def test_peak_kernel_objects_are_the_listed_ones():
    found = _peak_objects()
    assert len(found) == len(set(found)), "a kernel object appears twice"
    assert not set(found) - set(PEAK_KERNELS), "in the library but not listed: %s" % sorted(set(found) - set(PEAK_KERNELS))
    assert not set(PEAK_KERNELS) - set(found), "listed but not in the library: %s" % sorted(set(PEAK_KERNELS) - set(found))
    assert all(PEAK_KERNELS.values())


def test_peak_symbols_are_bound_and_refuse_null():
    L = _lib.load()
    for name in ("sg_set_peaks", "sg_get_peaks", "sg_get_peaks_dev", "sg_peaks_samples"):
        assert name in _lib.SYMBOLS and hasattr(L, name)
    n = C.c_int64(7)
    buf = np.zeros(4)
    smp = np.zeros(4, dtype=np.int32)
    assert L.sg_set_peaks(None, 1, 1, 1) == -1
    assert L.sg_get_peaks(None, 0, buf.ctypes.data, smp.ctypes.data, 4) == -1
    assert L.sg_get_peaks_dev(None, 0, None, 0, None, 4) == -1
    assert L.sg_peaks_samples(None, C.byref(n)) == -1 and n.value == 7


# ---- the restatement -------------------------------------------------------------------------------------------------------

def stress_lines(dim, sym):
    """the stress lines c = i * dim + j the device reads, ascending (sg_spectra_lines)"""
    lines = np.full(9, -1, dtype=np.int32)
    n = _lib.load().sg_spectra_lines(int(dim), int(bool(sym)), lines.ctypes.data, 9)
    assert n > 0
    return [int(c) for c in lines[:n]]


def peak_terms(x, dim, sym, stress=None):
    """m of one sample: x [..., dim] a velocity or [..., dim, dim] a stress (`stress`; None: told by the trailing shape, which
    a caller whose node count may equal dim must not rely on), converted to double first; m = x_0 x_0, then
    m = m + (x_c x_c) over the lines ascending, each product and each sum rounded on its own (numpy has no fma); in
    symmetric storage an off-diagonal line enters as 2.0 * (x * x) and the i > j lines are not read."""
    x = np.asarray(x, dtype=np.float64)
    if stress is None:
        stress = x.ndim >= 2 and x.shape[-2:] == (dim, dim)
    if stress:
        assert x.shape[-2:] == (dim, dim)
        x = x.reshape(x.shape[:-2] + (dim * dim,))
        lines = [(c, 2.0 if (sym and c // dim < c % dim) else 1.0) for c in stress_lines(dim, sym)]
    else:
        assert x.shape[-1] == dim
        lines = [(c, 1.0) for c in range(dim)]
    m = None
    for c, weight in lines:
        t = x[..., c] * x[..., c]
        if weight == 2.0:
            t = 2.0 * t
        m = t if m is None else m + t
    return m


def peak_reference(samples, dim, sym, value=None, sample=None, j0=0, stress=None):
    """(value, sample) after the samples [n, ...] in their order, from the state (value, sample) armed maps start with (0.0
    and -1) or the one given, the first sample being number j0: if (m > value) { value = m; sample = j; } - strict, so the
    earliest sample wins a tie, a NaN never enters and a node that never moved keeps -1."""
    samples = np.asarray(samples)
    first = peak_terms(samples[0], dim, sym, stress)
    value = np.zeros(first.shape) if value is None else np.array(value, dtype=np.float64)
    sample = np.full(first.shape, -1, dtype=np.int32) if sample is None else np.array(sample, dtype=np.int32)
    for k in range(len(samples)):
        m = first if k == 0 else peak_terms(samples[k], dim, sym, stress)
        with np.errstate(invalid="ignore"):
            up = m > value
        value = np.where(up, m, value)
        sample = np.where(up, np.int32(j0 + k), sample).astype(np.int32)
    return value, sample


def _loop_reference(samples, dim, sym, stress):
    """the same with Python floats, node by node"""
    n, nodes = samples.shape[0], samples.shape[1]
    value, sample = [0.0] * nodes, [-1] * nodes
    for j in range(n):
        for a in range(nodes):
            x = [float(v) for v in samples[j, a].reshape(-1)]
            if stress:
                terms = []
                for i in range(dim):
                    for k in range(dim):
                        if sym and i > k:
                            continue
                        t = x[i * dim + k] * x[i * dim + k]
                        terms.append(2.0 * t if (sym and i < k) else t)
            else:
                terms = [v * v for v in x]
            m = terms[0]
            for t in terms[1:]:
                m = m + t
            if m > value[a]:
                value[a], sample[a] = m, j
    return np.array(value), np.array(sample, dtype=np.int32)


def test_reference_against_a_plain_loop():
    rng = np.random.default_rng(3)
    for dim in (1, 2, 3):
        for stress in (False, True):
            for sym in ((False, True) if stress else (False,)):
                shape = (6, 9, dim, dim) if stress else (6, 9, dim)
                x = rng.uniform(-1.0, 1.0, shape)
                if stress and sym:
                    x = 0.5 * (x + np.swapaxes(x, -1, -2))
                x[1, 1] = x[3, 1] = 2.0               # an exact tie at the maximum: the earlier sample keeps the node
                x[:, 2] = 0.0                         # a node that never moves
                x[2, 3] = np.nan                      # a NaN sample never enters
                x[4, 4] = 5.0                         # ... and a late maximum does
                x[0, 5] = 7.0                         # ... an early one stays
                if stress and not sym and dim > 1:
                    x[5, 6, 1, 0] = 9.0               # full storage reads the i > j lines
                got = peak_reference(x, dim, sym, stress=stress)
                want = _loop_reference(x, dim, sym, stress)
                assert got[0].dtype == np.float64 and got[1].dtype == np.int32
                assert np.array_equal(got[0].view(np.int64), want[0].view(np.int64)) and np.array_equal(got[1], want[1]), (dim, stress, sym)
                assert got[1][1] == 1 and got[1][2] == -1 and got[0][2] == 0.0 and got[1][3] != 2 and got[1][4] == 4 and got[1][5] == 0
                assert not np.isnan(got[0]).any()
                if stress and not sym and dim > 1:
                    assert got[1][6] == 5
                if stress and sym and dim > 1:
                    # the doubling: equal to the full sum of a symmetric tensor up to rounding, and exactly twice the product
                    full = peak_reference(x, dim, False, stress=True)
                    ok = ~np.isnan(x).any(axis=(0, 2, 3))
                    assert np.allclose(got[0][ok], full[0][ok], rtol=1e-14, atol=0.0)
    # continued from a state: the same as in one go
    x = rng.uniform(-1.0, 1.0, (8, 5, 2, 2))
    v1, s1 = peak_reference(x[:3], 2, False)
    v2, s2 = peak_reference(x[3:], 2, False, v1, s1, 3)
    v, s = peak_reference(x, 2, False)
    assert np.array_equal(v, v2) and np.array_equal(s, s2)
    assert math.isclose(float(peak_terms(np.array([3.0, 4.0]), 2, False)), 25.0)
