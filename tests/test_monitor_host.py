"""CPU-only tests of the monitor (include/seigen_hip.h sg_measure / sg_set_monitor): the kernel objects of its namespace in
the built library are the listed ones, each with the GPU test that launches it; the weights the solver class hands the
library are the header's formulas; the sanitizer driver that walks the monitor's clock still builds."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from seigen_amd import _lib
from seigen_amd.elastic import monitor_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Every kernel object of namespace sg::measure (kernels_measure.hip) with the rows of tests/test_monitor_gpu.py
# test_every_layout_measures_what_the_oracle_does that launch it.  tests/test_host_logic.py pins the objects named sg::name(;
# this list keeps the same rule for the nested namespace: no kernel joins the library without a decision about who tests it.
MEASURE_KERNELS = {
    "sg::measure::pass1_reg<double, 20>": "rows mfma-P3-sym, mfma-P3-full",
    "sg::measure::pass1_reg<float, 20>": "row mfma-P3-f32",
    "sg::measure::pass1_reg<double, 35>": "rows mfma-P4-sym, mfma-P4-full",
    "sg::measure::pass1_reg<float, 35>": "row mfma-P4-f32",
    "sg::measure::pass1_lds<double>": "rows generic-*, lane-*, tile-*, hexm-* (gw = 1, 64, 16; hexm-DQ4: two items at a time)",
    "sg::measure::pass1_lds<float>": "row tile-tri-P3-f32",
    "sg::measure::pass2": "every row; more partials than threads: row generic-1d-P1-1030",
}


def _signature_name(sig):
    """`ns::name<args>` of a demangled function signature that names namespace sg::measure: from `sg::measure::` to the
    `(` that opens the argument list, template arguments (nested ones included) skipped"""
    start = sig.index("sg::measure::")
    depth = 0
    for i in range(start, len(sig)):
        c = sig[i]
        if c == "<":
            depth += 1
        elif c == ">":
            depth -= 1
        elif c == "(" and depth == 0:
            return sig[start:i]
    return sig[start:]


def _measure_objects():
    """every OBJECT symbol of the library whose function NAME lies in sg::measure (an argument type there does not count),
    whatever its return type and template arguments"""
    readelf = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "llvm-readelf")
    assert os.path.exists(readelf), "llvm-readelf (shipped with ROCm) not found at %s: set ROCM_PATH" % readelf
    out = subprocess.run([readelf, "--dyn-syms", "--demangle", _lib.lib_path()], capture_output=True, text=True, check=True).stdout
    found = []
    for line in out.splitlines():
        f = line.split(None, 7)
        if len(f) < 8 or f[3] != "OBJECT" or "sg::measure::" not in f[7]:
            continue
        sig = f[7]
        # the function's own name is what stands in front of the top-level argument list
        depth, head = 0, sig
        for i, c in enumerate(sig):
            if c == "<":
                depth += 1
            elif c == ">":
                depth -= 1
            elif c == "(" and depth == 0:
                head = sig[:i]
                break
        if "sg::measure::" in head:
            found.append(_signature_name(sig))
    return found


def test_signature_parser():
    assert _signature_name("void sg::measure::pass1_reg<double, 35>(double const*, sg::measure::Args)") == "sg::measure::pass1_reg<double, 35>"
    assert _signature_name("sg::measure::pass2(sg::measure::Args)") == "sg::measure::pass2"
    assert _signature_name("int sg::measure::k<std::pair<int, int>, 3>(int)") == "sg::measure::k<std::pair<int, int>, 3>"


def test_measure_kernel_objects_are_the_listed_ones():
    found = _measure_objects()
    assert len(found) == len(set(found)), "a kernel object appears twice"
    assert not set(found) - set(MEASURE_KERNELS), "in the library but not listed: %s" % sorted(set(found) - set(MEASURE_KERNELS))
    assert not set(MEASURE_KERNELS) - set(found), "listed but not in the library: %s" % sorted(set(MEASURE_KERNELS) - set(found))
    assert all(MEASURE_KERNELS.values())


def test_monitor_symbols_are_bound():
    L = _lib.load()
    for name in ("sg_measure", "sg_set_monitor", "sg_get_monitor"):
        assert name in _lib.SYMBOLS and hasattr(L, name)
    assert L.sg_abi_version() == 2
    hdr = open(os.path.join(ROOT, "include", "seigen_hip.h")).read()
    assert re.search(r"#define SG_MONITOR_CHUNK_ITEMS \d+", hdr)


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_weights_are_the_formulas_of_the_header(dim):
    rho, mu, lam = 1.3, 0.25, 0.5
    w = monitor_weights(dim, rho, mu, lam, 10)
    assert w.shape == (3,) and w.flags.c_contiguous
    assert w[0] == rho / 2 and w[1] == 1 / (4 * mu) and w[2] == -lam / (4 * mu * (dim * lam + 2 * mu))
    rng = np.random.default_rng(3)
    rc, mc, lc = (rng.uniform(0.5, 2.0, 10) for _ in range(3))
    for args in ((rc, mc, lc), (rho, mc, lam), (rc, mu, lam), (rho, mu, lc)):
        w = monitor_weights(dim, args[0], args[1], args[2], 10)
        r, m, l = (np.broadcast_to(a, (10,)) for a in args)
        assert w.shape == (10, 3) and w.flags.c_contiguous and w.dtype == np.float64
        assert np.array_equal(w[:, 0], r / 2) and np.array_equal(w[:, 1], 1 / (4 * m))
        assert np.array_equal(w[:, 2], -l / (4 * m * (dim * l + 2 * m)))
    # the compliance energy: with these weights ws |s|^2 + wt tr(s)^2 = 1/2 s : strain for a random symmetric tensor
    s = rng.uniform(-1, 1, (dim, dim))
    s = s + s.T
    eps = (s - lam / (dim * lam + 2 * mu) * np.trace(s) * np.eye(dim)) / (2 * mu)
    w = monitor_weights(dim, rho, mu, lam, 1)
    assert abs(w[1] * np.sum(s * s) + w[2] * np.trace(s) ** 2 - 0.5 * np.sum(s * eps)) < 1e-13


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_host_asan_driver_still_builds():
    """`make host-asan` builds the driver that walks the monitor's clock and component order; tests/test_host_asan.py runs it"""
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "seigen_amd", "csrc"), "host-asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert os.path.exists(os.path.join(ROOT, "build_tools", "host_asan_driver"))
