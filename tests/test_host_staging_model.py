"""CPU: the host side of NUM_DEV = 1 ... 8 (the reference's DevicePool of NUM_DEV runners, host/src/fpga.cpp:1646-1673).

The REAL host half of the C-ABI (hexl-fpga_amd/csrc/host_staging.hip: staging pipeline, process-wide copy-thread pool, per-runner unpack lane) is
compiled with g++ against a CPU shim of the HIP host API (tests/cpp/hip_shim/: device memory = host memory, copy-engine transfers cost
nothing, streams / events are no-ops) and stub launchers (tests/cpp/stage_model_stubs.cpp: nothing computed, device time = 0 or a sleep),
under the REAL hexl_fpga_api.cpp -- so what runs is exactly the host work of the host-pointer entry points: runner threads, window
sharing, packing t_target into the slabs, adding the output into the callers' result arrays. tests/cpp/bench_cxx_api drives it like
benchmark/bench_keyswitch.cpp.

What it pins: with eight devices every runner takes a share of the window, nothing deadlocks, and the host side does not COLLAPSE under
eight runners + the shared pool (rate at NUM_DEV = 8 >= 0.6 x the rate at NUM_DEV = 1 on the same box). What it documents (printed, and
quoted in DESIGN.md section 6 from the GPU pool's hosts): the host side does not SCALE with NUM_DEV either -- a keyswitch through host
pointers costs ~6.4 MB of host memory traffic (pack 0.8 MB, read 1.6 MB of output, read-modify-write 1.6 MB of result), the copies are
memory-bound, and the pods run under a CPU quota; callers that want eight devices' worth keep their ciphertexts device-resident."""
import os
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "tests" / "cpp" / "_stage" / "bench_cxx_api"


def rate(num_dev, window, env=None):
    out = subprocess.run([str(EXE), str(window), "6", "0"], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, NUM_DEV=str(num_dev), FAKE_DEVICES="8", **(env or {})))
    assert out.returncode == 0, out.stderr[-1500:]
    m = re.search(r": (\d+) keyswitch/s", out.stdout)
    assert m, out.stdout[-500:]
    return float(m.group(1)), out.stderr


def test_host_side_of_eight_devices():
    subprocess.run(["make", "-C", str(EXE.parent.parent), "stage_model"], check=True, capture_output=True)
    r1, _ = rate(1, 256)
    r8, err = rate(8, 256, {"FPGA_DEBUG": "1"})
    devices = {int(d) for d in re.findall(r"device (\d+): \d+ x KeySwitch", err)}
    print(f"host-side staging model, window 256, L = 6: NUM_DEV=1 {r1:.0f} keyswitch/s, NUM_DEV=8 {r8:.0f} keyswitch/s; runners that took a share: {sorted(devices)}")
    assert devices == set(range(8)), "every device's runner takes a share of a 256-object window"
    assert r8 >= 0.6 * r1, "eight runners + the shared copy pool must not collapse the host side"


def test_modelled_device_time_overlaps_across_devices():
    """with a device that takes 100 us per keyswitch (10 k/s per device, slower than the host side) eight runners deliver several devices'
    worth: the runners really work concurrently, the host layer adds no serialisation of its own"""
    subprocess.run(["make", "-C", str(EXE.parent.parent), "stage_model"], check=True, capture_output=True)
    slow = {"HEXL_MODEL_DEVICE_US_PER_KS": "400"}
    r1, _ = rate(1, 128, slow)
    r8, _ = rate(8, 128, slow)
    print(f"modelled device at 2.5 k keyswitch/s: NUM_DEV=1 {r1:.0f}/s, NUM_DEV=8 {r8:.0f}/s")
    assert r1 < 2600 and r8 > 2.5 * r1
