"""The host code of the gradient - grad.cpp and the host half of kernels_grad.hip - on the CPU under ASan and UBSan, linked
against the HIP runtime double of tests/fake_hip instead of a device: build_tools/host_runtime_grad, a program of its own beside
build_tools/host_runtime_driver and build_tools/host_runtime_peaks, built by the same `make host-runtime-asan` over the same
objects (tools/host_runtime_grad.cpp has the checks).  The driver's kernel objects are a closed list (tests/test_host_runtime.py)
and the peaks program counts its own against the driver's (tests/test_peaks_runtime.py); nothing but the two entry points
reaches the gradient, so neither links it and this program holds its kernels against GRAD_KERNELS.  Nothing is loaded into
Python, nothing runs on a GPU.

On a 3-D MFMA, a lane, a tile f32 and a generic block the program calls both getters for both velocity fields, every kind, both
buffer types, whole blocks and ranges - every launch of sg::grad:: with its grid, LDS and scalars against sg_gradient_plan and its
pointers against the extents the kernel walks - between stepping calls too, and injects a failure into every runtime call of
both getters, with tables built before and not: the error code, a message, nothing leaked, the tables as they were."""
import functools
import os
import subprocess

from tests.host_runtime_program import BAD, ROOT, _instrumented, build, needs_toolchain
from tests.test_grad_host import GRAD_KERNELS
from tests.test_host_runtime import _name

pytestmark = needs_toolchain

EXE = os.path.join(ROOT, "build_tools", "host_runtime_grad")
BLOCKS = ["mfma-P4-f64", "lane-2d-P2", "tile-tri-P3-f32", "generic-1d-P2"]


@functools.lru_cache(maxsize=None)
def _output():
    """the program's output: it was built with the driver, exited 0, said `clean`, and no sanitizer spoke"""
    build()
    assert os.path.exists(EXE) and _instrumented(EXE)
    env = {k: v for k, v in os.environ.items() if not k.startswith("SEIGEN_HIP_")}   # (the program sets the ones it needs)
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=900, env=env)
    tail = "\n".join(line for line in (r.stdout + r.stderr).splitlines() if not line.startswith("kernel: "))[-6000:]
    assert r.returncode == 0, tail
    assert "host_runtime_grad: clean" in r.stdout, tail
    assert not any(b in r.stdout + r.stderr for b in BAD), tail
    return r.stdout


def test_gradient_host_code_clean_over_the_runtime_double():
    """its blocks in order, more than 100 failures injected and no error"""
    out = _output()
    tail = "\n".join(line for line in out.splitlines() if not line.startswith("kernel: "))[-6000:]
    assert [ln.split(":")[0] for ln in out.splitlines() if ln.endswith(" gradient calls")] == BLOCKS, tail
    line = [ln for ln in out.splitlines() if "failures injected" in ln]
    assert len(line) == 1 and int(line[0].split()[1]) > 100 and line[0].endswith(" 0 errors"), tail


def test_gradient_kernel_objects_register_with_the_runtime():
    """the kernel objects of namespace sg::grad that the host half registers are GRAD_KERNELS, no other and none missing; the
    driver itself registers none of them, and everything else this program registers is the driver's"""
    found = [_name(ln[len("kernel: "):]) for ln in _output().splitlines() if ln.startswith("kernel: ")]
    assert len(found) == len(set(found)), "a kernel object registers twice"
    grad = {k for k in found if k.startswith("sg::grad::")}
    assert grad == set(GRAD_KERNELS), (sorted(grad - set(GRAD_KERNELS)), sorted(set(GRAD_KERNELS) - grad))
    driver = subprocess.run([os.path.join(ROOT, "build_tools", "host_runtime_driver"), "kernels"], capture_output=True, text=True).stdout
    others = [ln for ln in driver.splitlines() if ln.startswith("kernel: ")]
    assert len(others) == len(found) - len(grad) and not any("sg::grad::" in ln for ln in others)
