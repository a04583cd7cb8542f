"""CPU: hexl_hks_rotate_hoisted and hexl_hks_linear_transform exist in the header, in the built library and in the ctypes table with
their arities (7 and 9), the Python functions are there with their parameter lists, the header states the word identities, and both
entry points refuse null handle arrays, null entries and null pointers (batch == 0 does not excuse them) without a device and without
writing anything."""
import ctypes
import inspect
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
HEXL_E_BADARG = -1
ARITY = {"hexl_hks_rotate_hoisted": 7, "hexl_hks_linear_transform": 9, "hexl_hks_hoisted_scratch_bytes": 2}


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
    for text in ("NOT word for word hexl_hks_rotate", "does NOT raise the input-range flag", "for g = 1 hexl_hks_rotate_hoisted is word for word",
                 "one encoded plaintext serves every level", "hexl_hks_scratch_bytes itself is unchanged"):
        assert text in header, text


def test_wrappers_exist(hx):
    assert list(inspect.signature(hx.hks_rotate_hoisted).parameters) == ["hks_list", "galois_elts", "outs", "ct", "batch", "n_limbs"]
    assert list(inspect.signature(hx.hks_linear_transform).parameters) == ["hks_list", "galois_elts", "pts", "pt_identity", "out", "ct", "batch",
                                                                          "n_limbs"]
    assert list(inspect.signature(hx.HybridKeySwitch.hoisted_scratch_bytes).parameters) == ["self", "batch"]
    assert "hks_rotate_hoisted" in hx.__all__ and "hks_linear_transform" in hx.__all__


def test_null_arrays_entries_and_pointers_are_refused_and_nothing_is_written(hx):
    hx.build()
    lib = ctypes.CDLL(str(hx.LIB_PATH))
    for name in ARITY:
        getattr(lib, name).argtypes = hx.C_ABI[name]
        getattr(lib, name).restype = ctypes.c_size_t if name.endswith("_scratch_bytes") else ctypes.c_int
    buf = (ctypes.c_uint64 * 96)()
    a, b, c = (ctypes.addressof(buf) + 8 * 32 * k for k in range(3))
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    null_handles = (vp * 2)(None, None)                           # an array whose entries are null handles
    fake = (vp * 2)(a, a)                                         # stands for non-null output / plaintext pointers
    null_entries = (vp * 2)(a, None)
    gs = (u64 * 2)(5, 3)
    assert lib.hexl_hks_hoisted_scratch_bytes(None, 7) == 0
    for batch in (1, 0):
        rot, lt = lib.hexl_hks_rotate_hoisted, lib.hexl_hks_linear_transform
        assert rot(None, gs, 2, fake, b, batch, 1) == HEXL_E_BADARG
        assert rot(null_handles, None, 2, fake, b, batch, 1) == HEXL_E_BADARG
        assert rot(null_handles, gs, 2, None, b, batch, 1) == HEXL_E_BADARG
        assert rot(null_handles, gs, 2, fake, None, batch, 1) == HEXL_E_BADARG
        assert rot(null_handles, gs, 2, fake, b, batch, 1) == HEXL_E_BADARG            # null entries of hks
        assert rot(null_handles, gs, 2, null_entries, b, batch, 1) == HEXL_E_BADARG
        assert lt(None, gs, fake, 2, None, a, b, batch, 1) == HEXL_E_BADARG
        assert lt(null_handles, None, fake, 2, None, a, b, batch, 1) == HEXL_E_BADARG
        assert lt(null_handles, gs, None, 2, None, a, b, batch, 1) == HEXL_E_BADARG
        assert lt(null_handles, gs, fake, 2, None, None, b, batch, 1) == HEXL_E_BADARG
        assert lt(null_handles, gs, fake, 2, None, a, None, batch, 1) == HEXL_E_BADARG
        assert lt(null_handles, gs, fake, 2, c, a, b, batch, 1) == HEXL_E_BADARG          # null entries of hks
        assert lt(null_handles, gs, null_entries, 2, None, a, b, batch, 1) == HEXL_E_BADARG
        assert lt(null_handles, gs, fake, 0, None, a, b, batch, 1) == HEXL_E_BADARG       # no rotation at all
    assert not any(buf), "a refused call wrote"
