"""CPU: hexl_hks_linear_transform_bsgs_ext and hexl_hks_bsgs_ext_scratch_bytes exist in the header, in the built library and in the ctypes
table with their arities (13 and 4), the Python functions are there with their parameter lists, the header states the definition, the
facts and what the call is not word-identical to, and the entry point refuses null arrays, null entries and null pointers (batch == 0
does not excuse them) at every rescale value, in and out of range, without a device and without writing anything. Without a device there
is no keyed object, so every call here also carries a null handle or pointer: the refusal of rescale = 2, and of rescale = 1 at one
limb, on otherwise well-formed arguments is isolated in tests/test_gpu_hks_bsgs_ext.py::test_every_rejection."""
import ctypes
import inspect
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
HEXL_E_BADARG = -1
ARITY = {"hexl_hks_linear_transform_bsgs_ext": 13, "hexl_hks_bsgs_ext_scratch_bytes": 4}


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
    assert header.index("hexl_hks_linear_transform_bsgs(") < header.index("hexl_hks_linear_transform_bsgs_ext(") < header.index(
        "hexl_hks_multiply_sum_relinearize("), "next to hexl_hks_linear_transform_bsgs"
    for text in ("ONE division per call", "u_j[i] = kf_j[1][i] + down_P(inner_j[1])[i]", "the special rows included",
                 "X_k = P F_k + A_k modulo Q_l P", "word for word hexl_hks_linear_transform on row 0",
                 "word for word the flat hexl_hks_linear_transform over the concatenated non-NULL terms",
                 "out_k = round(X_k / R) - e with an integer e in", "NOT word for word hexl_hks_linear_transform_bsgs",
                 "NOT word for word that call followed by hexl_rescale", "#{G != 1} (E + P (n_p + 1/2) n)",
                 "rescale outside {0, 1}", "n_limbs < 2 with rescale == 1", "the four older *_scratch_bytes figures are unchanged"):
        assert text in header, text


def test_wrappers_exist(hx):
    assert list(inspect.signature(hx.hks_linear_transform_bsgs_ext).parameters) == [
        "baby_hks", "baby_elts", "giant_hks", "giant_elts", "pts", "pt_identity", "out", "ct", "batch", "n_limbs", "rescale"]
    assert list(inspect.signature(hx.HybridKeySwitch.bsgs_ext_scratch_bytes).parameters) == ["self", "n_baby", "batch", "rescale"]
    assert "hks_linear_transform_bsgs_ext" in hx.__all__


def test_null_arguments_and_a_bad_rescale_are_refused_and_nothing_is_written(hx):
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
    for rescale in (0, 1):
        assert lib.hexl_hks_bsgs_ext_scratch_bytes(None, 2, 7, rescale) == 0
    fn = lib.hexl_hks_linear_transform_bsgs_ext
    for batch in (1, 0):
        for rescale, l in ((0, 1), (1, 2), (2, 2), (-1, 2), (1, 1)):
            assert fn(None, gs, 2, nulls, gs, 2, pts, None, a, b, batch, l, rescale) == HEXL_E_BADARG
            assert fn(nulls, None, 2, nulls, gs, 2, pts, None, a, b, batch, l, rescale) == HEXL_E_BADARG
            assert fn(nulls, gs, 2, None, gs, 2, pts, None, a, b, batch, l, rescale) == HEXL_E_BADARG
            assert fn(nulls, gs, 2, nulls, None, 2, pts, None, a, b, batch, l, rescale) == HEXL_E_BADARG
            assert fn(nulls, gs, 2, nulls, gs, 2, None, None, a, b, batch, l, rescale) == HEXL_E_BADARG
            assert fn(nulls, gs, 2, nulls, gs, 2, pts, None, None, b, batch, l, rescale) == HEXL_E_BADARG
            assert fn(nulls, gs, 2, nulls, gs, 2, pts, None, a, None, batch, l, rescale) == HEXL_E_BADARG
            assert fn(nulls, gs, 2, nulls, gs, 0, pts, None, a, b, batch, l, rescale) == HEXL_E_BADARG         # no giant step
            assert fn(nulls, gs, 2, nulls, gs, 2, pts, ids, a, b, batch, l, rescale) == HEXL_E_BADARG          # no object at all
            assert fn(nulls, gs, 2, nulls, ones, 2, no_pts, ids, a, b, batch, l, rescale) == HEXL_E_BADARG     # ... even where none would be used
            assert fn(nulls, gs, 0, nulls, ones, 2, no_pts, ids, a, b, batch, l, rescale) == HEXL_E_BADARG
    assert not any(buf), "a refused call wrote"
