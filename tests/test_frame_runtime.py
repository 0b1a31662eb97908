"""The host code of the frames - frame.cpp and the host half of kernels_frame.hip - on the CPU under ASan and UBSan, linked
against the HIP runtime double of tests/fake_hip instead of a device (`make -C seigen_amd/csrc host-frame-asan`, ROCm's clang++
throughout; tools/host_frame_driver.cpp has the checks).  A stand-alone program of its own beside host_runtime_driver and
host_xfer_driver, whose lists of registered kernel objects it leaves alone: nothing is loaded into Python, nothing runs on a GPU.

On a 3-D MFMA, a lane, a tile f32 and a generic block the driver drives sg_get_frame_dev under the pointer audit - volumes and
slices, velocity and stress, both buffer types, contiguous and strided, the tables cached and not - checks every launch against
sg_frame_plan, and injects a failure into every runtime call it makes: the error code, a message, nothing leaked, the handle
and its cached tables as they were."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = ("AddressSanitizer", "runtime error:", "LeakSanitizer")
CLANG = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "clang++")
EXE = os.path.join(ROOT, "build_tools", "host_frame_driver")

pytestmark = pytest.mark.skipif(not os.path.exists(CLANG) or shutil.which("make") is None, reason="needs ROCm's clang++ and make")


def _instrumented(path):
    """the static sanitizer runtimes are linked in (no LD_PRELOAD): their entry points are DEFINED in the executable"""
    out = subprocess.run(["nm", "--defined-only", path], capture_output=True, text=True).stdout
    return "__asan_init" in out and "__ubsan_handle" in out


def test_frame_host_code_clean_over_the_runtime_double():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "seigen_amd", "csrc"), "-j", str(min(16, os.cpu_count() or 1)),
                        "host-frame-asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert _instrumented(EXE)
    env = {k: v for k, v in os.environ.items() if not k.startswith("SEIGEN_HIP_")}   # (the driver sets the ones it needs)
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=600, env=env)
    tail = (r.stdout + r.stderr)[-6000:]
    assert r.returncode == 0, tail
    assert "host_frame_driver: clean" in r.stdout, tail
    assert not any(b in r.stdout + r.stderr for b in BAD), tail
    blocks = [ln.split(":")[0] for ln in r.stdout.splitlines() if ln.endswith(" frames")]
    assert blocks == ["mfma-P4-f64", "lane-2d-P2", "tile-tri-P3-f32", "generic-1d-P2"], tail
    line = [ln for ln in r.stdout.splitlines() if "failures injected" in ln]
    assert len(line) == 1 and int(line[0].split()[1]) > 100 and line[0].endswith(" 0 errors"), tail
