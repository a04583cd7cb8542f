"""CPU: the route of a standalone _NTT / _INTT launch -- hexl-fpga_amd/csrc/ntt_route.hpp, the pure host function ntt.hip executes:
kernel family, geometry, tier, persistence, grids, the prepare and redo launches and the hint clearing -- against routes written out
as literals (tests/cpp/ntt_route_selftest.cpp): every ring dimension and direction, both sides of every modulus threshold, batches
around the persistence threshold on 256 and on 4 CUs, hinted and not, an inverse with a scale factor that is not a residue, and each
HEXL_NTT_* knob off its default. The program is stand-alone and built with -fsanitize=address,undefined."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CPP = ROOT / "tests" / "cpp"


def test_ntt_route_selftest(tmp_path):
    exe = tmp_path / "ntt_route_selftest"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-Wall",
                    "-Wno-unused-function", "-o", str(exe), str(CPP / "ntt_route_selftest.cpp")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(out.stdout[-4000:])
    print(out.stderr[-4000:])
    assert out.returncode == 0 and "ALL PASSED" in out.stdout
    assert "ERROR: " not in out.stderr and "runtime error" not in out.stderr
