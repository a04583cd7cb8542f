"""CPU: the per-word chain of hexl_pk_encrypt (hexl-fpga_amd/csrc/sample_core.hpp pk_operand / pk_product / pk_c0 / pk_c1, what
k_pk_encrypt compiles) built for the host and run against unsigned __int128 on the eleven selftest moduli: operands at {0, 1, q/2, q - 2,
q - 1} in every position plus 4000 random ones per modulus, with the intermediate bounds the header states asserted on the way --
tests/cpp/pk_selftest.cpp, compiled here with the flags of sample_selftest.cpp. The program is stand-alone: it is also the one to give
a host sanitizer."""
import subprocess
from pathlib import Path

from test_rns_ops_abi import selftest_moduli

ROOT = Path(__file__).resolve().parent.parent


def test_pk_chain_host_replay(orc, tmp_path):
    exe = tmp_path / "pk_selftest"
    subprocess.run(["g++", "-O2", "-std=c++17", "-mfma", "-ffp-contract=off", "-Wall", "-o", str(exe),
                    str(ROOT / "tests" / "cpp" / "pk_selftest.cpp")], check=True)
    out = subprocess.run([str(exe), "4000"] + [str(q) for q in selftest_moduli(orc)], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:])
    assert out.returncode == 0 and "ALL PASSED" in out.stdout
