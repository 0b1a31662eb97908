"""CPU-only tests of the spectra (include/seigen_hip.h sg_set_spectra / sg_get_spectrum / sg_spectra_samples /
sg_correlate_spectra): the kernel objects of namespace sg::spectra in the built library are the listed ones, each with the GPU
rows that launch it; the weights the solver class hands the library are exp(-i omega t) by the rectangle rule; the
convention of correlate_spectra is Parseval's; the clock and the list of accumulated lines against brute force."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from seigen_amd import _lib
from seigen_amd.elastic import spectra_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Every kernel object of namespace sg::spectra (kernels_spectra.hip) with the rows of tests/test_spectra_gpu.py
# test_transform_of_every_row (tests/gradient_loop.py ROWS) that launch it: the rule of tests/test_monitor_host.py
# MEASURE_KERNELS for this nested namespace.
SPECTRA_KERNELS = {
    "sg::spectra::accumulate<double>": "rows mfma-P4-sym, mfma-P3-sym (lines skipped), tile-*, hexm-DQ3, lane-2d-P2, generic-2d-P2 (gw = 1)",
    "sg::spectra::accumulate<float>": "rows mfma-P3-f32 (lines skipped), tile-tri-P3-f32",
}


def _name_of(sig, ns):
    """`ns::name<args>` of a demangled signature whose function NAME lies in `ns`, else None"""
    depth, head = 0, sig
    for i, c in enumerate(sig):
        if c == "<":
            depth += 1
        elif c == ">":
            depth -= 1
        elif c == "(" and depth == 0:
            head = sig[:i]
            break
    return head[head.index(ns):] if ns in head else None


def _spectra_objects():
    readelf = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "llvm-readelf")
    assert os.path.exists(readelf), "llvm-readelf (shipped with ROCm) not found at %s: set ROCM_PATH" % readelf
    out = subprocess.run([readelf, "--dyn-syms", "--demangle", _lib.lib_path()], capture_output=True, text=True, check=True).stdout
    found = []
    for line in out.splitlines():
        f = line.split(None, 7)
        if len(f) < 8 or f[3] != "OBJECT":
            continue
        name = _name_of(f[7], "sg::spectra::")
        if name:
            found.append(name)
    return found


def test_signature_parser():
    assert _name_of("void sg::spectra::accumulate<double>(double const*, sg::spectra::Args)", "sg::spectra::") == "sg::spectra::accumulate<double>"
    assert _name_of("void sg::other<float>(sg::spectra::Args)", "sg::spectra::") is None


def test_spectra_kernel_objects_are_the_listed_ones():
    found = _spectra_objects()
    assert len(found) == len(set(found)), "a kernel object appears twice"
    assert not set(found) - set(SPECTRA_KERNELS), "in the library but not listed: %s" % sorted(set(found) - set(SPECTRA_KERNELS))
    assert not set(SPECTRA_KERNELS) - set(found), "listed but not in the library: %s" % sorted(set(SPECTRA_KERNELS) - set(found))
    assert all(SPECTRA_KERNELS.values())


def test_spectra_symbols_are_bound():
    L = _lib.load()
    for name in ("sg_set_spectra", "sg_get_spectrum", "sg_spectra_samples", "sg_correlate_spectra", "sg_spectra_clock", "sg_spectra_lines"):
        assert name in _lib.SYMBOLS and hasattr(L, name)
    hdr = open(os.path.join(ROOT, "include", "seigen_hip.h")).read()
    assert "#define SG_SPECTRA_MAX_FREQ %d" % _lib.SPECTRA_MAX_FREQ in hdr


def test_weights_against_numpy_exp():
    freqs, dt, every, n = [0.0, 1.7, 12.5], 3.1e-3, 3, 7
    for t0, stagger, window in ((0.0, 0.0, None), (0.25, 0.5 * dt, np.hanning(n + 2)[1:-1])):
        w = spectra_weights(freqs, dt, every, n, t0=t0, stagger=stagger, window=window)
        assert w.shape == (n, 3, 2) and w.dtype == np.float64 and w.flags.c_contiguous
        for j in range(n):
            t = t0 + (j + 1) * every * dt + stagger
            for k, f in enumerate(freqs):
                want = every * dt * (1.0 if window is None else window[j]) * np.exp(-2j * np.pi * f * t)
                assert abs(w[j, k, 0] + 1j * w[j, k, 1] - want) <= 4 * np.finfo(float).eps * abs(want) + 1e-300
        # f = 0: the quadrature weight alone
        assert np.array_equal(w[:, 0, 1], np.zeros(n))
    with pytest.raises(ValueError):
        spectra_weights(freqs, dt, 0, n)
    with pytest.raises(ValueError):
        spectra_weights(freqs, dt, 1, n, window=np.ones(n + 1))


def test_convention_of_correlate_spectra():
    """With unit-modulus weights exp(-2 pi i f j / N) and the full set of N frequencies, sum_j x_j y_j = (1 / N) sum_f
    Re(conj(X_f) Y_f) (Parseval); z = i picks -(Xr Yi - Xi Yr): the (re, im) pairing with -z_i and (im, re) with +z_i."""
    rng = np.random.default_rng(5)
    N = 12
    x, y = rng.uniform(-1, 1, N), rng.uniform(-1, 1, N)
    # the weights of N samples at dt = 1, every = 1 and the frequencies k / N, shifted back by one sample: t_j = j
    w = spectra_weights(np.arange(N) / N, 1.0, 1, N, t0=-1.0)
    w = w[..., 0] + 1j * w[..., 1]
    assert np.abs(w - np.exp(-2j * np.pi * np.outer(np.arange(N), np.arange(N)) / N)).max() < 1e-14
    X, Y = w.T @ x, w.T @ y
    assert np.abs(X - np.fft.fft(x)).max() < 1e-13

    def device_terms(X, Y, z):
        """what sg_correlate_spectra adds for one frequency, the forms being plain products here"""
        zr, zi = z.real, z.imag
        t = zr * (X.real * Y.real) + zr * (X.imag * Y.imag)
        if zi != 0.0:
            t += -zi * (X.real * Y.imag) + zi * (X.imag * Y.real)
        return t

    assert abs(np.sum(device_terms(X, Y, 1 + 0j)) / N - np.dot(x, y)) < 1e-13
    for z in (1j, 0.3 - 0.8j):
        assert np.abs(device_terms(X, Y, z) - (z * np.conj(X) * Y).real).max() < 1e-13
    # z = i: the cross terms alone, with these signs
    assert np.abs(device_terms(X, Y, 1j) - (-(X.real * Y.imag) + X.imag * Y.real)).max() < 1e-15


def test_clock_against_brute_force():
    L = _lib.load()
    out = (C.c_int64 * 4)()
    for every in (1, 2, 3, 5):
        for nsamples in (0, 1, 3, 4):
            sample_steps = [(j + 1) * every for j in range(nsamples)]
            for steps in range(0, 24):
                for more in (0, 1, 7):
                    assert L.sg_spectra_clock(every, nsamples, steps, more, out) == 0
                    due = (steps + 1) in sample_steps
                    assert out[0] == int(due)
                    assert out[1] == (sample_steps.index(steps + 1) if due else -1)
                    assert out[2] == int(any(s > steps for s in sample_steps))
                    assert out[3] == sum(1 for s in sample_steps if s <= steps + more)
    assert L.sg_spectra_clock(0, 1, 0, 0, out) == -1 and L.sg_spectra_clock(1, 1, 0, 0, None) == -1


def test_line_lists_against_brute_force():
    L = _lib.load()
    for dim in (1, 2, 3):
        for sym in (0, 1):
            lines = np.full(9, -1, dtype=np.int32)
            n = L.sg_spectra_lines(dim, sym, lines.ctypes.data, 9)
            want = [i * dim + j for i in range(dim) for j in range(dim) if not sym or i <= j]
            assert n == len(want) and list(lines[:n]) == want and np.all(lines[n:] == -1)
    assert L.sg_spectra_lines(3, 0, np.zeros(4, dtype=np.int32).ctypes.data, 4) == -1
    assert L.sg_spectra_lines(4, 0, np.zeros(16, dtype=np.int32).ctypes.data, 16) == -1
