"""CPU: hexl_rns_from_f64 / hexl_rns_to_f64 / hexl_ckks_encode / hexl_ckks_decode exist in the built library and in the ctypes table
and refuse null handles and pointers, and the round-and-reduce chain of rns_from_f64 (f64_arith.hpp f64_to_residue) agrees with
__int128 on the host (tests/cpp/from_f64_selftest.cpp, compiled here)."""
import ctypes
import subprocess
from pathlib import Path

from test_rns_ops_abi import selftest_moduli

ROOT = Path(__file__).resolve().parent.parent
HEXL_E_BADARG = -1
NEW = ("hexl_rns_from_f64", "hexl_rns_to_f64", "hexl_ckks_encode", "hexl_ckks_decode")


def test_encode_entry_points_refuse_null_handles_and_pointers(hx):
    hx.build()
    lib = ctypes.CDLL(str(hx.LIB_PATH))
    for name in NEW:
        assert name in hx.C_ABI, f"{name} missing from the ctypes table"
        assert hasattr(lib, name), f"{name} not exported by {hx.LIB_PATH.name}"
        fn = getattr(lib, name)
        fn.argtypes = hx.C_ABI[name]
        fn.restype = ctypes.c_int
    assert hx.C_ABI["hexl_ckks_encode"][-1] is ctypes.c_double and hx.C_ABI["hexl_ckks_decode"][-1] is ctypes.c_double
    buf = (ctypes.c_uint64 * 16)()
    a, b = ctypes.addressof(buf), ctypes.addressof(buf) + 64
    for fn in (lib.hexl_rns_from_f64, lib.hexl_rns_to_f64):
        assert fn(None, a, b, 1, 1) == HEXL_E_BADARG                  # no plan
        assert fn(None, None, None, 0, 1) == HEXL_E_BADARG            # count == 0 does not excuse null pointers
        assert fn(None, a, None, 0, 1) == HEXL_E_BADARG
    for fn in (lib.hexl_ckks_encode, lib.hexl_ckks_decode):
        assert fn(None, a, b, 1, 1, 1024.0) == HEXL_E_BADARG
        assert fn(None, None, None, 0, 1, 1024.0) == HEXL_E_BADARG
        assert fn(None, a, b, 0, 1, 0.0) == HEXL_E_BADARG
        assert fn(None, a, b, 0, 1, float("nan")) == HEXL_E_BADARG
    for name in NEW:
        assert hasattr(hx.KeySwitchPlan, name[len("hexl_"):]), f"KeySwitchPlan.{name[len('hexl_'):]} missing"


def test_from_f64_host_replay(orc, tmp_path):
    exe = tmp_path / "from_f64_selftest"
    subprocess.run(["g++", "-O2", "-std=c++17", "-mfma", "-ffp-contract=off", "-Wall", "-o", str(exe),
                    str(ROOT / "tests" / "cpp" / "from_f64_selftest.cpp")], check=True)
    out = subprocess.run([str(exe), "400"] + [str(q) for q in selftest_moduli(orc)], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:])
    assert out.returncode == 0 and "ALL PASSED" in out.stdout
