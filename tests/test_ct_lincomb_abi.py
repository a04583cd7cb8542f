"""CPU: hexl_ct_lincomb exists in the built library and in the ctypes table and refuses null handles and pointers (batch == 0 does not
excuse them), and its scalar chains (f64_arith.hpp lc_term / lc_add / lc_finish) agree with 128-bit integers on the host
(tests/cpp/lincomb_selftest.cpp, compiled here with the flags of pt_mul_selftest.cpp)."""
import ctypes
import subprocess
from pathlib import Path

from test_rns_ops_abi import selftest_moduli

ROOT = Path(__file__).resolve().parent.parent
HEXL_E_BADARG = -1
NAME = "hexl_ct_lincomb"


def test_ct_lincomb_refuses_null_handles_and_pointers(hx):
    hx.build()
    lib = ctypes.CDLL(str(hx.LIB_PATH))
    assert NAME in hx.C_ABI, f"{NAME} missing from the ctypes table"
    assert hasattr(lib, NAME), f"{NAME} not exported by {hx.LIB_PATH.name}"
    fn = getattr(lib, NAME)
    fn.argtypes = hx.C_ABI[NAME]
    fn.restype = ctypes.c_int
    buf = (ctypes.c_uint64 * 24)()
    a, b = (ctypes.addressof(buf) + 8 * 8 * k for k in range(2))
    terms = (ctypes.c_void_p * 2)(b, b)
    holes = (ctypes.c_void_p * 2)(b, None)
    for batch in (1, 0):
        assert fn(None, a, terms, None, None, 2, None, 1, None, batch, 2, 1) == HEXL_E_BADARG          # no plan
        assert fn(None, None, terms, None, None, 2, None, 1, None, batch, 2, 1) == HEXL_E_BADARG       # no output
        assert fn(None, a, None, None, None, 2, None, 1, None, batch, 2, 1) == HEXL_E_BADARG           # no term array
        assert fn(None, a, holes, None, None, 2, None, 1, None, batch, 2, 1) == HEXL_E_BADARG          # a null term
        assert fn(None, a, terms, None, None, 0, None, 1, None, batch, 2, 1) == HEXL_E_BADARG          # no term
        assert fn(None, a, terms, None, None, 9, None, 1, None, batch, 2, 1) == HEXL_E_BADARG          # too many (the array is not read)
    assert fn(None, None, None, None, None, 0, None, 0, None, 0, 0, 0) == HEXL_E_BADARG


def test_lincomb_host_replay(orc, tmp_path):
    exe = tmp_path / "lincomb_selftest"
    subprocess.run(["g++", "-O2", "-std=c++17", "-mfma", "-ffp-contract=off", "-Wall", "-o", str(exe),
                    str(ROOT / "tests" / "cpp" / "lincomb_selftest.cpp")], check=True)
    out = subprocess.run([str(exe), "4000"] + [str(q) for q in selftest_moduli(orc)], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:])
    assert out.returncode == 0 and "ALL PASSED" in out.stdout
