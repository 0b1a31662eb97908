"""The host code of the frames - frame.cpp and the host half of kernels_frame.hip - on the CPU under ASan and UBSan, linked
against the HIP runtime double of tests/fake_hip instead of a device: the suite `frames` of build_tools/host_runtime_driver
(tests/host_runtime_program.py builds and runs the program; tools/host_runtime_frame.cpp has the checks).  Nothing is loaded
into Python, nothing runs on a GPU.

On a 3-D MFMA, a lane, a tile f32 and a generic block the driver drives sg_get_frame_dev under the pointer audit - volumes and
slices, velocity and stress, both buffer types, contiguous and strided, the tables cached and not - checks every launch against
sg_frame_plan, and injects a failure into every runtime call it makes: the error code, a message, nothing leaked, the handle
and its cached tables as they were."""
from tests.host_runtime_program import needs_toolchain, run_suite

pytestmark = needs_toolchain


def test_frame_host_code_clean_over_the_runtime_double():
    run_suite("frames", "frames", ["mfma-P4-f64", "lane-2d-P2", "tile-tri-P3-f32", "generic-1d-P2"])
