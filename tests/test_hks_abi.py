"""CPU: the hybrid key switch's entry points exist in the header, in the built library and in the ctypes table with their arities, the
Python wrappers are there, and every entry point refuses null handles and pointers (batch == 0 does not excuse them) without a device
and without writing anything."""
import ctypes
import inspect
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
HEXL_E_BADARG = -1
ARITY = {"hexl_hks_create": 3, "hexl_hks_destroy": 1, "hexl_hks_set_keys_device": 2, "hexl_hks_keyswitch": 5, "hexl_hks_relinearize": 5,
         "hexl_hks_rotate": 6, "hexl_hks_scratch_bytes": 2}


def test_entry_points_are_declared_exported_and_bound(hx):
    header = (ROOT / "include" / "hexl_mi355x.h").read_text()
    assert re.search(r"^typedef struct hexl_hks hexl_hks;", header, flags=re.M), "the opaque handle is not declared"
    hx.build()
    lib = ctypes.CDLL(str(hx.LIB_PATH))
    for name, arity in ARITY.items():
        decl = re.search(r"^(int|size_t)\s+%s\s*\(([^;]*)\);" % name, header, flags=re.M)
        assert decl, f"{name} is not declared in include/hexl_mi355x.h"
        assert len(decl.group(2).split(",")) == arity, name
        assert (decl.group(1) == "size_t") == (name == "hexl_hks_scratch_bytes")
        assert name in hx.C_ABI and len(hx.C_ABI[name]) == arity, name
        assert hasattr(lib, name), f"{name} not exported by {hx.LIB_PATH.name}"
    # the contract's fine print is in the header
    for text in ("does NOT raise the input-range flag", "is NOT checked", "BEFORE the plan", "one key serves every level"):
        assert text in header, text


def test_wrappers_exist(hx):
    cls = hx.HybridKeySwitch
    assert list(inspect.signature(cls.__init__).parameters) == ["self", "plan", "digit_limbs"]
    assert list(inspect.signature(cls.set_keys_device).parameters) == ["self", "keys"]
    assert list(inspect.signature(cls.keyswitch).parameters) == ["self", "result", "t_target", "batch", "n_limbs"]
    assert list(inspect.signature(cls.relinearize).parameters) == ["self", "out", "ct3", "batch", "n_limbs"]
    assert list(inspect.signature(cls.rotate).parameters) == ["self", "out", "ct", "batch", "n_limbs", "g"]
    assert list(inspect.signature(cls.scratch_bytes).parameters) == ["self", "batch"]
    gen = inspect.signature(hx.KeySwitchPlan.gen_hybrid_key)
    assert list(gen.parameters) == ["self", "out", "secret", "digit_limbs", "from_poly", "seed", "stream", "first"]
    assert gen.parameters["stream"].default == 0 and gen.parameters["first"].default == 0 and gen.parameters["seed"].default is None
    assert "hexl_gen_hybrid_key" not in hx.C_ABI and "hexl_hks_gen_keys" not in hx.C_ABI      # a wrapper, not a C entry point
    assert "first + dnum - 1" in hx.KeySwitchPlan.gen_hybrid_key.__doc__ and "WARNING" in hx.KeySwitchPlan.gen_hybrid_key.__doc__
    assert "HybridKeySwitch" in hx.__all__


def test_null_handles_and_pointers_are_refused_and_nothing_is_written(hx):
    hx.build()
    lib = ctypes.CDLL(str(hx.LIB_PATH))
    for name, args in hx.C_ABI.items():
        if name.startswith("hexl_hks_"):
            getattr(lib, name).argtypes = args
            getattr(lib, name).restype = ctypes.c_size_t if name == "hexl_hks_scratch_bytes" else ctypes.c_int
    buf = (ctypes.c_uint64 * 64)()
    a, b = ctypes.addressof(buf), ctypes.addressof(buf) + 8 * 32
    out = ctypes.c_void_p(0x1234)
    assert lib.hexl_hks_create(None, 1, ctypes.byref(out)) == HEXL_E_BADARG and not out.value, "a refused create must leave *out NULL"
    assert lib.hexl_hks_create(None, 1, None) == HEXL_E_BADARG
    assert lib.hexl_hks_destroy(None) == HEXL_E_BADARG
    assert lib.hexl_hks_set_keys_device(None, a) == HEXL_E_BADARG
    assert lib.hexl_hks_scratch_bytes(None, 7) == 0
    for batch in (1, 0):
        assert lib.hexl_hks_keyswitch(None, a, b, batch, 1) == HEXL_E_BADARG
        assert lib.hexl_hks_keyswitch(None, None, None, batch, 1) == HEXL_E_BADARG
        assert lib.hexl_hks_relinearize(None, a, b, batch, 1) == HEXL_E_BADARG
        assert lib.hexl_hks_relinearize(None, None, b, batch, 1) == HEXL_E_BADARG
        assert lib.hexl_hks_rotate(None, a, b, batch, 1, 5) == HEXL_E_BADARG
        assert lib.hexl_hks_rotate(None, a, None, batch, 1, 5) == HEXL_E_BADARG
    assert not any(buf), "a refused call wrote"
