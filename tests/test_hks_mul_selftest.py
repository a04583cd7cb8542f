"""CPU: the scalar chains the hybrid multiply adds (hexl-fpga_amd/csrc/f64_arith.hpp hks_acc_pd and hks_down_rs, and hks_round at the
rescaling mod-down's halves -- what keyswitch_hybrid.hip compiles into k_hks_down_intt<., true> and k_hks_down<., true>) built for the host and run
against unsigned __int128 on the eleven selftest moduli, 27 bits to just below 2^52: canonical words 0 and q - 1, accumulators and
transform outputs at +-(q/2 + 2), with the intermediate bounds the header states asserted on the way -- tests/cpp/hks_mul_selftest.cpp.
The program is stand-alone, with its own main, and is built with -fsanitize=address,undefined."""
import subprocess
from pathlib import Path

from test_rns_ops_abi import selftest_moduli

ROOT = Path(__file__).resolve().parent.parent


def test_hks_multiply_chains_host_replay(orc, tmp_path):
    exe = tmp_path / "hks_mul_selftest"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-mfma", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-Wall", "-o", str(exe),
                    str(ROOT / "tests" / "cpp" / "hks_mul_selftest.cpp")], check=True)
    qs = selftest_moduli(orc)
    assert min(qs) < 1 << 27 and max(qs) > (1 << 52) - (1 << 20)
    out = subprocess.run([str(exe), "20000"] + [str(q) for q in qs], capture_output=True, text=True, timeout=300)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0 and "ALL PASSED" in out.stdout
