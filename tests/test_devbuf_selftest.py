"""CPU: the host scaffold of hexl-fpga_amd/csrc/hexl_internal.hpp -- the owning buffer type every context and plan buffer is a member
of, and the argument-check vocabulary of the plan-level entry points -- through the real capi.hip on the CPU shim of the HIP host API
(tests/cpp/devbuf_selftest.cpp, with the stubs of the CPU staging model). The program is stand-alone and built with
-fsanitize=address,undefined: a buffer that escapes hexl_ks_plan_destroy / hexl_ctx_destroy is a leak report and a non-zero exit."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CPP = ROOT / "tests" / "cpp"
CSRC = ROOT / "hexl-fpga_amd" / "csrc"


def test_devbuf_selftest(tmp_path):
    exe = tmp_path / "devbuf_selftest"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-Wall",
                    "-Wno-unused-function", f"-I{CPP / 'hip_shim'}", "-o", str(exe), "-x", "c++", str(CPP / "devbuf_selftest.cpp"),
                    str(CSRC / "capi.hip"), str(CPP / "stage_model_stubs.cpp"), str(CSRC / "host_simd.cpp")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(out.stdout[-4000:])
    print(out.stderr[-4000:])
    assert out.returncode == 0 and "ALL PASSED" in out.stdout
    assert "ERROR: " not in out.stderr and "runtime error" not in out.stderr
