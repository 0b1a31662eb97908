"""build_tools/host_runtime_driver for the tests that run it (test_host_runtime.py, test_device_transfer_runtime.py,
test_frame_runtime.py): the device-facing host code of libseigen_hip on the CPU under ASan and UBSan, linked against the HIP
runtime double of tests/fake_hip instead of a device (`make -C seigen_amd/csrc host-runtime-asan`, ROCm's clang++ throughout;
tools/host_runtime_driver.cpp, host_runtime_xfer.cpp and host_runtime_frame.cpp have the checks).  A stand-alone program with
the static sanitizer runtimes linked in: nothing is loaded into Python, nothing runs on a GPU."""
import functools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = ("AddressSanitizer", "runtime error:", "LeakSanitizer")
CLANG = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "clang++")
EXE = os.path.join(ROOT, "build_tools", "host_runtime_driver")

needs_toolchain = pytest.mark.skipif(not os.path.exists(CLANG) or shutil.which("make") is None, reason="needs ROCm's clang++ and make")


def _instrumented(path):
    """the static sanitizer runtimes are linked in (no LD_PRELOAD): their entry points are DEFINED in the executable"""
    out = subprocess.run(["nm", "--defined-only", path], capture_output=True, text=True).stdout
    return "__asan_init" in out and "__ubsan_handle" in out


@functools.lru_cache(maxsize=None)
def build():
    """the program, built once per session"""
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "seigen_amd", "csrc"), "-j", str(min(16, os.cpu_count() or 1)),
                        "host-runtime-asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert _instrumented(EXE)
    return EXE


def run(*args):
    """the program's output: it exited 0, said `clean`, and no sanitizer spoke"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("SEIGEN_HIP_")}   # (the driver sets the ones it needs)
    r = subprocess.run([build(), *args], capture_output=True, text=True, timeout=900, env=env)
    tail = "\n".join(line for line in (r.stdout + r.stderr).splitlines() if not line.startswith("kernel: "))[-6000:]
    assert r.returncode == 0, tail
    assert "host_runtime_driver: clean" in r.stdout, tail
    assert not any(b in r.stdout + r.stderr for b in BAD), tail
    return r.stdout


def run_suite(name, counted, blocks):
    """one feature suite (`xfer`, `frames`): its blocks in order - the lines `NAME: N <counted>` - more than 100 failures
    injected and no error"""
    out = run(name)
    tail = "\n".join(line for line in out.splitlines() if not line.startswith("kernel: "))[-6000:]
    assert [ln.split(":")[0] for ln in out.splitlines() if ln.endswith(" " + counted)] == blocks, tail
    line = [ln for ln in out.splitlines() if "failures injected" in ln]
    assert len(line) == 1 and int(line[0].split()[1]) > 100 and line[0].endswith(" 0 errors"), tail
