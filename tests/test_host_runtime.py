"""The device-facing host code of libseigen_hip - api.cpp, stages.cpp, transfer.cpp, comm.cpp, devxfer.cpp, frame.cpp and the
host halves of every kernels*.hip: launch wrappers, stage_kernel_* choices, grid sizing - on the CPU under ASan and UBSan,
linked against the HIP runtime double of tests/fake_hip instead of a device (tests/host_runtime_program.py builds and runs the
program; tools/host_runtime_driver.cpp has the checks).  A stand-alone program: nothing is loaded into Python, nothing runs on
a GPU.

Per block - the smallest of each kernel family - the driver runs a whole life of a handle with every launch's device
pointers audited against the live allocations, compares the launches of graph replay with those of SEIGEN_HIP_GRAPH=0, and
injects a failure into every allocation, copy or fill, object creation and launch of every entry point: the error code,
the message, nothing leaked, the handle as it was, the next steps launching what a twin's launch.  (The program's suites for
the device transfers and the frames: tests/test_device_transfer_runtime.py, tests/test_frame_runtime.py.)

Running time, measured on 16 CPU cores (the build: 16 s with -j16, once per session): the whole
sweep takes 127 s - mfma-P4-f64 57 s, hexm-DQ3 21 s, mfma-P2-f32 14 s, mfma-P3-nbr 13 s, the four 1-D / 2-D blocks 4 - 7 s
each - against 9 s of host_asan_driver, so it is split by block into one test each; nothing of the sweep is left out."""
import subprocess

import pytest

from tests.host_runtime_program import build, needs_toolchain, run

BLOCKS = ["mfma-P4-f64", "mfma-P2-f32", "tile-tri-P3", "tile-quad-DQ2", "hexm-DQ3", "lane-2d-P2", "generic-1d-P2", "mfma-P3-nbr"]

pytestmark = needs_toolchain


def _name(sig):
    """`sg::name<args>` of a demangled kernel signature: what stands between the return type and the parameter list"""
    depth, at = 0, len(sig) - 1
    assert sig.endswith(")"), sig
    while at >= 0:
        depth += {")": 1, "(": -1}.get(sig[at], 0)
        if depth == 0:
            break
        at -= 1
    head = sig[:at]
    return head[head.index("sg::"):]


def test_name_of_a_signature():
    assert _name("void sg::measure::pass1_reg<double, 35>(double const*, sg::measure::Args)") == "sg::measure::pass1_reg<double, 35>"
    assert _name("sg::measure::pass2(sg::measure::Args)") == "sg::measure::pass2"
    assert _name("void sg::tile2d_stage<3, 0, 0, 1, 0, 0, double>(sg::StageArgs, sg::T2Const)") == "sg::tile2d_stage<3, 0, 0, 1, 0, 0, double>"
    assert _name("sg::step_counter_kernel(long*, long, int)") == "sg::step_counter_kernel"


def test_every_block_of_the_driver_is_swept():
    """BLOCKS is the driver's kBlocks: a block added there alone would never be run by the test below"""
    assert subprocess.run([build(), "blocks"], capture_output=True, text=True).stdout.split() == BLOCKS


@pytest.mark.parametrize("block", BLOCKS)
def test_device_facing_host_code_clean_over_the_runtime_double(block):
    """(a) a life under the pointer audit, (b) replay equals eager, (c) the failure sweep, (d) sizes that cannot be met - of
    one block; the driver asserts that no failure index was skipped and reports how many it injected"""
    out = run(block)
    line = [ln for ln in out.splitlines() if ln.startswith("host_runtime_driver: block %s:" % block)]
    assert len(line) == 1, out[-2000:]
    launches, injected = int(line[0].split()[3]), int(line[0].split()[8])
    assert launches > 100 and injected > 100, line[0]


def test_every_kernel_object_registers_with_the_runtime():
    """(e) the kernel objects the host halves register with the runtime are the ones the suite's lists name: the lists of
    tests/test_host_logic.py and tests/test_monitor_host.py (642) and those of the correlation, the injectors and the
    spectra (10), the device transfers (10) and the frames (6) - a kernel in no list cannot be launched unseen, and every
    listed one is reachable from the host code"""
    from tests.test_correlate_host import XCORR_KERNELS
    from tests.test_device_transfer_host import XFER_KERNELS
    from tests.test_frame_host import FRAME_KERNELS
    from tests.test_hex_family_gpu import HEXM_KERNELS, HEX_LANE_KERNELS
    from tests.test_host_logic import AUX_KERNELS
    from tests.test_injectors_host import INJECT_KERNELS
    from tests.test_lane_generic_family_gpu import GENERIC_KERNELS, LANE_KERNELS
    from tests.test_mfma_family_gpu import MFMA_KERNELS
    from tests.test_monitor_host import MEASURE_KERNELS
    from tests.test_spectra_host import SPECTRA_KERNELS
    from tests.test_tile2d_family_gpu import TILE2D_KERNELS
    out = run("kernels")
    sigs = [ln[len("kernel: "):] for ln in out.splitlines() if ln.startswith("kernel: ")]
    found = [_name(sig) for sig in sigs]
    assert len(found) == len(set(found)), "a kernel object registers twice"
    first = frozenset().union(MFMA_KERNELS, TILE2D_KERNELS, HEXM_KERNELS, HEX_LANE_KERNELS, LANE_KERNELS, GENERIC_KERNELS,
                              AUX_KERNELS, MEASURE_KERNELS)
    assert len(first) == 642
    listed = first | frozenset(XCORR_KERNELS) | frozenset(INJECT_KERNELS) | frozenset(SPECTRA_KERNELS) | frozenset(XFER_KERNELS) | frozenset(FRAME_KERNELS)
    assert len(listed) == 668
    assert not set(found) - listed, "registered but in no list: %s" % sorted(set(found) - listed)
    assert not listed - set(found), "listed but not registered: %s" % sorted(listed - set(found))
