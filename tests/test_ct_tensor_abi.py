"""CPU: hexl_ct_tensor_sum, hexl_relinearize and hexl_multiply_sum_relinearize exist in the built library and in the ctypes table with
their KeySwitchPlan wrappers and refuse null handles and pointers (batch == 0 does not excuse them), and the tensor sum's scalar chains
(f64_arith.hpp ts_operand / ts_mac / ts_finish) agree with 128-bit integers on the host (tests/cpp/tensor_selftest.cpp, compiled here
with the flags of lincomb_selftest.cpp)."""
import ctypes
import subprocess
from pathlib import Path

from test_rns_ops_abi import selftest_moduli

ROOT = Path(__file__).resolve().parent.parent
HEXL_E_BADARG = -1
NAMES = {"hexl_ct_tensor_sum": "ct_tensor_sum", "hexl_relinearize": "relinearize", "hexl_multiply_sum_relinearize": "multiply_sum_relinearize"}


def bound(hx, name):
    hx.build()
    lib = ctypes.CDLL(str(hx.LIB_PATH))
    assert name in hx.C_ABI, f"{name} missing from the ctypes table"
    assert hasattr(lib, name), f"{name} not exported by {hx.LIB_PATH.name}"
    fn = getattr(lib, name)
    fn.argtypes = hx.C_ABI[name]
    fn.restype = ctypes.c_int
    return fn


def test_symbols_table_and_wrappers(hx):
    for name, method in NAMES.items():
        bound(hx, name)
        assert callable(getattr(hx.KeySwitchPlan, method, None)), f"KeySwitchPlan.{method} missing"


def test_tensor_calls_refuse_null_handles_and_pointers(hx):
    buf = (ctypes.c_uint64 * 24)()
    a, b = (ctypes.addressof(buf) + 8 * 8 * k for k in range(2))
    terms = (ctypes.c_void_p * 2)(b, b)
    holes = (ctypes.c_void_p * 2)(b, None)
    tensor = bound(hx, "hexl_ct_tensor_sum")
    fused = bound(hx, "hexl_multiply_sum_relinearize")
    for batch in (1, 0):
        for fn, tail in ((tensor, (batch, 1)), (fused, (batch,))):
            assert fn(None, a, terms, terms, None, 2, *tail) == HEXL_E_BADARG          # no plan
            assert fn(None, None, terms, terms, None, 2, *tail) == HEXL_E_BADARG       # no output
            assert fn(None, a, None, terms, None, 2, *tail) == HEXL_E_BADARG           # no operand array
            assert fn(None, a, terms, None, None, 2, *tail) == HEXL_E_BADARG
            assert fn(None, a, holes, terms, None, 2, *tail) == HEXL_E_BADARG          # a null operand
            assert fn(None, a, terms, holes, None, 2, *tail) == HEXL_E_BADARG
            assert fn(None, a, terms, terms, None, 0, *tail) == HEXL_E_BADARG          # no term
            assert fn(None, a, terms, terms, None, 9, *tail) == HEXL_E_BADARG          # too many (the arrays are not read)
    assert tensor(None, None, None, None, None, 0, 0, 0) == HEXL_E_BADARG
    assert fused(None, None, None, None, None, 0, 0) == HEXL_E_BADARG
    relin = bound(hx, "hexl_relinearize")
    for batch in (1, 0):
        assert relin(None, a, b, batch) == HEXL_E_BADARG
        assert relin(None, None, b, batch) == HEXL_E_BADARG
        assert relin(None, a, None, batch) == HEXL_E_BADARG


def test_tensor_host_replay(orc, tmp_path):
    exe = tmp_path / "tensor_selftest"
    subprocess.run(["g++", "-O2", "-std=c++17", "-mfma", "-ffp-contract=off", "-Wall", "-o", str(exe),
                    str(ROOT / "tests" / "cpp" / "tensor_selftest.cpp")], check=True)
    out = subprocess.run([str(exe), "4000"] + [str(q) for q in selftest_moduli(orc)], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:])
    assert out.returncode == 0 and "ALL PASSED" in out.stdout
