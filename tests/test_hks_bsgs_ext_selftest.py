"""CPU: the scalar chain hexl_hks_linear_transform_bsgs_ext adds (hexl-fpga_amd/csrc/f64_arith.hpp hks_ext_acc -- what keyswitch_hybrid.hip
compiles into k_hks_mac<., HKS_MAC_ACC> and k_hks_ext_add) built for the host and run against unsigned __int128 on the eleven selftest
moduli, 27 bits to just below 2^52: accumulators at +-(q/2 + 2), addends built by the kernels' own chains (hks_mac_term over the digits,
lt_mac / lt_mac_acc on plaintext words 0 and q - 1), the accumulation onto a reduce output and a rotated row's two additions in
sequence, with the largest |accumulator + product| reported against 2^53 -- tests/cpp/hks_bsgs_ext_selftest.cpp. The program is
stand-alone, with its own main, and is built with -fsanitize=address,undefined."""
import subprocess
from pathlib import Path

from test_rns_ops_abi import selftest_moduli

ROOT = Path(__file__).resolve().parent.parent


def test_hks_bsgs_ext_chains_host_replay(orc, tmp_path):
    exe = tmp_path / "hks_bsgs_ext_selftest"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-mfma", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-Wall", "-o", str(exe),
                    str(ROOT / "tests" / "cpp" / "hks_bsgs_ext_selftest.cpp")], check=True)
    qs = selftest_moduli(orc)
    assert len(qs) == 11 and min(qs) < 1 << 27 and max(qs) > (1 << 52) - (1 << 20)
    out = subprocess.run([str(exe), "20000"] + [str(q) for q in qs], capture_output=True, text=True, timeout=300)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0 and "ALL PASSED" in out.stdout and "limit 2^53" in out.stdout
