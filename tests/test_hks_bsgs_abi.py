"""CPU: hexl_hks_linear_transform_bsgs and hexl_hks_bsgs_scratch_bytes exist in the header, in the built library and in the ctypes table
with their arities (12 and 3), the Python functions are there with their parameter lists, the header states the definition and what the
call is not word-identical to, and the entry point refuses null arrays, null entries and null pointers (batch == 0 does not excuse them)
without a device and without writing anything."""
import ctypes
import inspect
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
HEXL_E_BADARG = -1
ARITY = {"hexl_hks_linear_transform_bsgs": 12, "hexl_hks_bsgs_scratch_bytes": 3}


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
    assert header.index("hexl_hks_linear_transform(") < header.index("hexl_hks_linear_transform_bsgs("), "next to hexl_hks_linear_transform"
    for text in ("The call is word for word that composition", "It is NOT word for", "does NOT raise the input-range flag (hexl_ks_range_check)",
                 "hexl_linear_transform_bsgs word for word on per-limb plans", "already rotated by G_j^-1",
                 "hexl_hks_hoisted_scratch_bytes are unchanged", "an unused one may lack them"):
        assert text in header, text


def test_wrappers_exist(hx):
    assert list(inspect.signature(hx.hks_linear_transform_bsgs).parameters) == ["baby_hks", "baby_elts", "giant_hks", "giant_elts", "pts",
                                                                               "pt_identity", "out", "ct", "batch", "n_limbs"]
    assert list(inspect.signature(hx.HybridKeySwitch.bsgs_scratch_bytes).parameters) == ["self", "n_baby", "batch"]
    assert "hks_linear_transform_bsgs" in hx.__all__


def test_null_arrays_entries_and_pointers_are_refused_and_nothing_is_written(hx):
    hx.build()
    lib = ctypes.CDLL(str(hx.LIB_PATH))
    for name in ARITY:
        getattr(lib, name).argtypes = hx.C_ABI[name]
        getattr(lib, name).restype = ctypes.c_size_t if name.endswith("_scratch_bytes") else ctypes.c_int
    buf = (ctypes.c_uint64 * 96)()
    a, b, c = (ctypes.addressof(buf) + 8 * 32 * k for k in range(3))
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    nulls = (vp * 2)(None, None)                                  # an array whose entries are null handles
    pts = (vp * 4)(c, c, c, c)                                    # stands for non-null plaintext pointers
    no_pts = (vp * 4)(None, None, None, None)
    ids = (vp * 2)(c, c)
    gs, ones = (u64 * 2)(5, 3), (u64 * 2)(1, 1)
    assert lib.hexl_hks_bsgs_scratch_bytes(None, 2, 7) == 0
    fn = lib.hexl_hks_linear_transform_bsgs
    for batch in (1, 0):
        assert fn(None, gs, 2, nulls, gs, 2, pts, None, a, b, batch, 1) == HEXL_E_BADARG
        assert fn(nulls, None, 2, nulls, gs, 2, pts, None, a, b, batch, 1) == HEXL_E_BADARG
        assert fn(nulls, gs, 2, None, gs, 2, pts, None, a, b, batch, 1) == HEXL_E_BADARG
        assert fn(nulls, gs, 2, nulls, None, 2, pts, None, a, b, batch, 1) == HEXL_E_BADARG
        assert fn(nulls, gs, 2, nulls, gs, 2, None, None, a, b, batch, 1) == HEXL_E_BADARG
        assert fn(nulls, gs, 2, nulls, gs, 2, pts, None, None, b, batch, 1) == HEXL_E_BADARG
        assert fn(nulls, gs, 2, nulls, gs, 2, pts, None, a, None, batch, 1) == HEXL_E_BADARG
        assert fn(nulls, gs, 2, nulls, gs, 0, pts, None, a, b, batch, 1) == HEXL_E_BADARG          # no giant step
        assert fn(nulls, gs, 2, nulls, gs, 2, pts, ids, a, b, batch, 1) == HEXL_E_BADARG           # no object at all
        assert fn(nulls, gs, 2, nulls, ones, 2, no_pts, ids, a, b, batch, 1) == HEXL_E_BADARG      # ... even where none would be used
        assert fn(nulls, gs, 0, nulls, ones, 2, no_pts, ids, a, b, batch, 1) == HEXL_E_BADARG
    assert not any(buf), "a refused call wrote"
