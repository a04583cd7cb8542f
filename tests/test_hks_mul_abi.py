"""CPU: the hybrid multiply's entry points (hexl_hks_multiply_sum_relinearize, hexl_hks_relinearize_rescale,
hexl_hks_multiply_sum_rescale, hexl_hks_mul_scratch_bytes) exist in the header, in the built library and in the ctypes table with their
arities (8, 5, 8 and 2), the wrappers are there, the header states the definition and what the fused call is not word-identical to, and
null handles, pointers and arrays are refused for batch 1 and batch 0 without a device and without writing anything."""
import ctypes
import inspect
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
HEXL_E_BADARG = -1
ARITY = {"hexl_hks_multiply_sum_relinearize": 8, "hexl_hks_relinearize_rescale": 5, "hexl_hks_multiply_sum_rescale": 8,
         "hexl_hks_mul_scratch_bytes": 2}


def test_entry_points_are_declared_exported_and_bound(hx):
    header = (ROOT / "include" / "hexl_mi355x.h").read_text()
    hx.build()
    lib = ctypes.CDLL(str(hx.LIB_PATH))
    for name, arity in ARITY.items():
        decl = re.search(r"^(int|size_t)\s+%s\s*\(([^;]*)\);" % name, header, flags=re.M)
        assert decl, f"{name} is not declared in include/hexl_mi355x.h"
        assert len(decl.group(2).split(",")) == arity, name
        assert (decl.group(1) == "size_t") == name.endswith("_scratch_bytes")
        assert name in hx.C_ABI and len(hx.C_ABI[name]) == arity, name
        assert hasattr(lib, name), f"{name} not exported by {hx.LIB_PATH.name}"
    for text in ("R = P q_(l-1)", "out_k = round(X_k / R) - e with e an integer in [0, n_p]", "NOT word for word hexl_hks_relinearize",
                 "21 n sum_d |G_d| D_d / (P q_(l-1)) + (n_p + 1/2)(n + 1)", "the lower bound is 2 for the two rescaling calls",
                 "148 KiB of constants"):
        assert text in header, text


def test_wrappers_exist(hx):
    cls = hx.HybridKeySwitch
    assert list(inspect.signature(cls.multiply_sum_relinearize).parameters) == ["self", "out", "a_s", "b_s", "batch", "n_limbs", "in_limbs"]
    assert list(inspect.signature(cls.multiply_sum_rescale).parameters) == ["self", "out", "a_s", "b_s", "batch", "n_limbs", "in_limbs"]
    assert list(inspect.signature(cls.relinearize_rescale).parameters) == ["self", "out", "ct3", "batch", "n_limbs"]
    assert list(inspect.signature(cls.mul_scratch_bytes).parameters) == ["self", "batch"]


def test_null_handles_and_pointers_are_refused_and_nothing_is_written(hx):
    hx.build()
    lib = ctypes.CDLL(str(hx.LIB_PATH))
    for name in ARITY:
        getattr(lib, name).argtypes = hx.C_ABI[name]
        getattr(lib, name).restype = ctypes.c_size_t if name.endswith("_scratch_bytes") else ctypes.c_int
    buf = (ctypes.c_uint64 * 96)()
    a, b, c = (ctypes.addressof(buf) + 8 * 32 * k for k in range(3))
    ops = (ctypes.c_void_p * 2)(b, c)
    assert lib.hexl_hks_mul_scratch_bytes(None, 7) == 0
    for batch in (1, 0):
        for fn in (lib.hexl_hks_multiply_sum_relinearize, lib.hexl_hks_multiply_sum_rescale):
            assert fn(None, a, ops, ops, None, 2, batch, 2) == HEXL_E_BADARG
            assert fn(None, None, ops, ops, None, 2, batch, 2) == HEXL_E_BADARG
            assert fn(None, a, None, ops, None, 2, batch, 2) == HEXL_E_BADARG
            assert fn(None, a, ops, None, None, 2, batch, 2) == HEXL_E_BADARG
        assert lib.hexl_hks_relinearize_rescale(None, a, b, batch, 2) == HEXL_E_BADARG
        assert lib.hexl_hks_relinearize_rescale(None, None, b, batch, 2) == HEXL_E_BADARG
        assert lib.hexl_hks_relinearize_rescale(None, a, None, batch, 2) == HEXL_E_BADARG
    assert not any(buf), "a refused call wrote"
