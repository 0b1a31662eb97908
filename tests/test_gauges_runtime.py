"""The host code of the gauges - gauge.cpp, the sixth end-of-step hook of stages.cpp and the host half of kernels_gauge.hip - on
the CPU under ASan and UBSan, linked against the HIP runtime double of tests/fake_hip instead of a device:
build_tools/host_runtime_gauges, a program of its own beside build_tools/host_runtime_driver, built by the same
`make host-runtime-asan` over the same objects (tools/host_runtime_gauges.cpp has the checks).  The driver's kernel objects are
a closed list (tests/test_host_runtime.py); the gauges' kernel is no part of it, and stages.cpp reaches the gauges through the
armed tables alone, so the driver links without them and this program holds its own kernels against GAUGE_KERNELS.  Nothing
is loaded into Python, nothing runs on a GPU.

On a 3-D MFMA, a lane, a tile f32 and a generic block the program arms gauges, steps eagerly and through captured graphs,
through sg_step and through sg_end_step, up to the capacity and into the refusal beyond it (nothing queued, nothing counted),
reads out, probes once, arms again and disarms - every launch of sg::gauge:: under the pointer audit against the extents the
kernel walks, the launches of graph replay equal to those of eager steps - and injects a failure into every runtime call of
sg_set_gauges, sg_get_gauges and sg_probe_gradient: the error code, a message, nothing leaked, the gauges armed before and their
count as they were."""
import functools
import os
import subprocess

from tests.host_runtime_program import BAD, ROOT, _instrumented, build, needs_toolchain
from tests.test_gauges_host import GAUGE_KERNELS
from tests.test_host_runtime import _name

pytestmark = needs_toolchain

EXE = os.path.join(ROOT, "build_tools", "host_runtime_gauges")
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
    assert "host_runtime_gauges: clean" in r.stdout, tail
    assert not any(b in r.stdout + r.stderr for b in BAD), tail
    return r.stdout


def test_gauge_host_code_clean_over_the_runtime_double():
    """its blocks in order, more than 100 failures injected and no error"""
    out = _output()
    tail = "\n".join(line for line in out.splitlines() if not line.startswith("kernel: "))[-6000:]
    assert [ln.split(":")[0] for ln in out.splitlines() if ln.endswith(" read-outs")] == BLOCKS, tail
    line = [ln for ln in out.splitlines() if "failures injected" in ln]
    assert len(line) == 1 and int(line[0].split()[1]) > 100 and line[0].endswith(" 0 errors"), tail


def test_gauge_kernel_objects_register_with_the_runtime():
    """the kernel objects of namespace sg::gauge that the host half registers are GAUGE_KERNELS, no other and none missing; the
    driver itself registers none of them"""
    found = [_name(ln[len("kernel: "):]) for ln in _output().splitlines() if ln.startswith("kernel: ")]
    assert len(found) == len(set(found)), "a kernel object registers twice"
    mine = {k for k in found if k.startswith("sg::gauge::")}
    assert mine == set(GAUGE_KERNELS), (sorted(mine - set(GAUGE_KERNELS)), sorted(set(GAUGE_KERNELS) - mine))
    driver = subprocess.run([os.path.join(ROOT, "build_tools", "host_runtime_driver"), "kernels"], capture_output=True, text=True).stdout
    others = [ln for ln in driver.splitlines() if ln.startswith("kernel: ")]
    assert len(others) == len(found) - len(mine) and not any("sg::gauge::" in ln for ln in others)
