"""The host code of the device transfers - devxfer.cpp and the host half of kernels_xfer.hip - on the CPU under ASan and UBSan,
linked against the HIP runtime double of tests/fake_hip instead of a device: the suite `xfer` of build_tools/host_runtime_driver
(tests/host_runtime_program.py builds and runs the program; tools/host_runtime_xfer.cpp has the checks).  Nothing is loaded
into Python, nothing runs on a GPU.

On a 3-D MFMA, a lane, a tile f32 and a generic block the driver drives sg_get_field_dev, sg_set_field_dev and
sg_get_spectrum_dev under the pointer audit - whole fields and ranges, both buffer types, a stress into a block in symmetric
storage, spectra armed and not armed - checks every launch against sg_xfer_plan, and injects a failure into every runtime
call they make: the error code, a message, nothing leaked, the handle as it was."""
from tests.host_runtime_program import needs_toolchain, run_suite

pytestmark = needs_toolchain


def test_device_transfer_host_code_clean_over_the_runtime_double():
    run_suite("xfer", "transfers", ["mfma-P4-f64", "lane-2d-P2", "tile-tri-P3-f32", "generic-1d-P2"])
