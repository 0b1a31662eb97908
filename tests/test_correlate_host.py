"""CPU-only tests of the correlation (include/seigen_hip.h sg_correlate / sg_get_correlation / sg_reset_correlation): the
three exports are bound; the kernel objects of namespace sg::xcorr in the built library are the listed ones, each with the GPU
row that launches it; `sensitivity` is the derivative of the weighted sum it documents."""
import os
import subprocess

import numpy as np
import pytest

from seigen_amd import _lib
from seigen_amd.elastic import sensitivity

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Every kernel object of namespace sg::xcorr (kernels_xcorr.hip) with the rows of tests/test_correlate_gpu.py
# test_every_layout_correlates_what_the_host_does that launch it.  tests/test_host_logic.py pins the objects named sg::name(,
# tests/test_monitor_host.py those of sg::measure; this list keeps the same rule for this namespace.
XCORR_KERNELS = {
    "sg::xcorr::xcorr_mfma<double, 20>": "rows mfma-P3-sym, mfma-P3-full",
    "sg::xcorr::xcorr_mfma<float, 20>": "row mfma-P3-f32",
    "sg::xcorr::xcorr_mfma<double, 35>": "rows mfma-P4-sym, mfma-P4-full; test_a_wave_of_the_persistent_grid_takes_more_than_one_item",
    "sg::xcorr::xcorr_mfma<float, 35>": "row mfma-P4-f32",
    "sg::xcorr::xcorr_lds<double>": "rows generic-*, lane-*, tile-*, hexm-* (gw = 1, 64, 16; hexm-DQ4: one item per workgroup); "
                                    "SEIGEN_HIP_XCORR=lds on mfma-P4-sym, mfma-P3-sym",
    "sg::xcorr::xcorr_lds<float>": "row tile-tri-P3-f32",
}


def _top_level_head(sig):
    """what stands in front of the argument list of a demangled signature: return type, name, template arguments"""
    depth = 0
    for i, c in enumerate(sig):
        if c == "<":
            depth += 1
        elif c == ">":
            depth -= 1
        elif c == "(" and depth == 0:
            return sig[:i]
    return sig


def _xcorr_objects():
    """every OBJECT symbol of the library whose function NAME lies in sg::xcorr (an argument type there does not count)"""
    readelf = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "llvm-readelf")
    assert os.path.exists(readelf), "llvm-readelf (shipped with ROCm) not found at %s: set ROCM_PATH" % readelf
    out = subprocess.run([readelf, "--dyn-syms", "--demangle", _lib.lib_path()], capture_output=True, text=True, check=True).stdout
    found = []
    for line in out.splitlines():
        f = line.split(None, 7)
        if len(f) < 8 or f[3] != "OBJECT" or "sg::xcorr::" not in f[7]:
            continue
        head = _top_level_head(f[7])
        if "sg::xcorr::" in head:
            found.append(head[head.index("sg::xcorr::"):])
    return found


def test_head_parser():
    assert _top_level_head("void sg::xcorr::xcorr_mfma<double, 35>(sg::xcorr::Args)") == "void sg::xcorr::xcorr_mfma<double, 35>"
    assert _top_level_head("sg::f(sg::xcorr::Args)") == "sg::f"


def test_correlation_symbols_are_bound():
    L = _lib.load()
    for name in ("sg_correlate", "sg_get_correlation", "sg_reset_correlation"):
        assert name in _lib.SYMBOLS and hasattr(L, name)
    assert L.sg_abi_version() == 2
    hdr = open(os.path.join(ROOT, "include", "seigen_hip.h")).read()
    for name in ("sg_correlate", "sg_get_correlation", "sg_reset_correlation"):
        assert "int %s(" % name in hdr


def test_xcorr_kernel_objects_are_the_listed_ones():
    found = _xcorr_objects()
    assert len(found) == len(set(found)), "a kernel object appears twice"
    assert not set(found) - set(XCORR_KERNELS), "in the library but not listed: %s" % sorted(set(found) - set(XCORR_KERNELS))
    assert not set(XCORR_KERNELS) - set(found), "listed but not in the library: %s" % sorted(set(XCORR_KERNELS) - set(found))
    assert all(XCORR_KERNELS.values())


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_sensitivity_is_the_derivative_of_the_weighted_sum(dim):
    """central differences of f = rho uu + ss / (2 mu) - lambda / (2 mu (d lambda + 2 mu)) tt, relative step 1e-6: the
    truncation error is ~1e-12 / mu^2, the round-off ~1e-16 |f| / (1e-6 mu) <= 3e-9; asserted to 1e-7 (relative where |K| > 1)"""
    rng = np.random.default_rng(11 + dim)
    for _ in range(20):
        lam, mu = rng.uniform(0.2, 2.0, 2)
        rho = rng.uniform(0.5, 2.0)
        c = {k: rng.uniform(-1.0, 1.0) for k in ("uu", "ss", "tt")}

        def f(r, l, m):
            return r * c["uu"] + c["ss"] / (2 * m) - l / (2 * m * (dim * l + 2 * m)) * c["tt"]

        K = sensitivity(dim, rho, lam, mu, c)
        e = 1e-6
        fd = {"rho": (f(rho * (1 + e), lam, mu) - f(rho * (1 - e), lam, mu)) / (2 * e * rho),
              "lambda": (f(rho, lam * (1 + e), mu) - f(rho, lam * (1 - e), mu)) / (2 * e * lam),
              "mu": (f(rho, lam, mu * (1 + e)) - f(rho, lam, mu * (1 - e))) / (2 * e * mu)}
        for k in ("rho", "lambda", "mu"):
            assert abs(K[k] - fd[k]) <= 1e-7 * max(1.0, abs(K[k])), (dim, k, K[k], fd[k])
    # per cell: arrays in, arrays out
    n = 7
    lam, mu = rng.uniform(0.2, 2.0, (2, n))
    corr = {k: rng.uniform(-1.0, 1.0, n) for k in ("uu", "ss", "tt")}
    K = sensitivity(dim, 1.0, lam, mu, corr)
    for j in range(n):
        one = sensitivity(dim, 1.0, lam[j], mu[j], {k: v[j] for k, v in corr.items()})
        for k in ("rho", "lambda", "mu"):
            assert K[k].shape == (n,) and K[k][j] == one[k]
