"""CPU: the sampler's host/device header (hexl-fpga_amd/csrc/sample_core.hpp) built for the host and run against RFC 8439's block vector,
the definitions of the two small maps, and unsigned __int128 % on the eleven selftest moduli (edges plus 4000 random values per
modulus) -- tests/cpp/sample_selftest.cpp, compiled here with the flags of pt_mul_selftest.cpp. The program is stand-alone: it is
also the one to give a host sanitizer."""
import subprocess
from pathlib import Path

from test_rns_ops_abi import selftest_moduli

ROOT = Path(__file__).resolve().parent.parent


def test_sample_core_host_replay(orc, tmp_path):
    exe = tmp_path / "sample_selftest"
    subprocess.run(["g++", "-O2", "-std=c++17", "-mfma", "-ffp-contract=off", "-Wall", "-o", str(exe),
                    str(ROOT / "tests" / "cpp" / "sample_selftest.cpp")], check=True)
    out = subprocess.run([str(exe), "4000"] + [str(q) for q in selftest_moduli(orc)], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:])
    assert out.returncode == 0 and "ALL PASSED" in out.stdout
