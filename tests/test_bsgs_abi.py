"""CPU: hexl_linear_transform_bsgs and hexl_lt_bsgs_scratch_bytes exist in the built library and in the ctypes table, with the
wrappers beside them, and the entry point refuses what needs no GPU to refuse."""
import ctypes

import pytest

HEXL_E_BADARG = -1
NAME, BYTES = "hexl_linear_transform_bsgs", "hexl_lt_bsgs_scratch_bytes"


def test_bsgs_entry_points_and_null_refusals(hx):
    hx.build()
    lib = ctypes.CDLL(str(hx.LIB_PATH))
    vp, u64, sz = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_size_t
    for name in (NAME, BYTES):
        assert name in hx.C_ABI, f"{name} missing from the ctypes table"
        assert hasattr(lib, name), f"{name} not exported by {hx.LIB_PATH.name}"
    P, U = ctypes.POINTER(vp), ctypes.POINTER(u64)
    assert hx.C_ABI[NAME] == [P, U, sz, P, U, sz, P, P, vp, vp, sz]
    assert hx.C_ABI[BYTES] == [vp, sz, sz]
    assert callable(hx.linear_transform_bsgs) and callable(hx.lt_bsgs_scratch_bytes)
    assert "linear_transform_bsgs" in hx.__all__ and "lt_bsgs_scratch_bytes" in hx.__all__
    fn = getattr(lib, NAME)
    fn.argtypes = hx.C_ABI[NAME]
    fn.restype = ctypes.c_int
    buf = (u64 * 32)()
    word = ctypes.addressof(buf)
    plans = (vp * 1)(None)                                             # arrays that hold a null plan
    pts = (vp * 1)(word)
    gs = (u64 * 1)(3)
    out, ct = vp(word + 64), vp(word + 128)
    ok = [plans, gs, 1, plans, gs, 1, pts, None, out, ct, 1]
    for k in (0, 1, 3, 4, 6, 8, 9):                                    # every pointer but d_pt_identity
        args = list(ok)
        args[k] = None
        assert fn(*args) == HEXL_E_BADARG, f"null argument {k}"
    assert fn(*ok) == HEXL_E_BADARG                                    # no plan at all in the two arrays
    args = list(ok)
    args[5] = 0
    assert fn(*args) == HEXL_E_BADARG                                  # n_giant == 0
    size = getattr(lib, BYTES)
    size.argtypes, size.restype = hx.C_ABI[BYTES], sz
    assert size(None, 4, 8) == 0


def test_wrapper_wants_a_full_grid(hx):
    with pytest.raises(ValueError):
        hx.linear_transform_bsgs([None, None], [3, 5], [None], [1], [[None]], None, None, 1)          # a row of one for two babies
    with pytest.raises(ValueError):
        hx.linear_transform_bsgs([None], [3], [None, None], [1, 5], [[None]], None, None, 1)          # one row for two giants
    with pytest.raises(ValueError):
        hx.linear_transform_bsgs([None], [3], [None], [1], [[None]], None, None, 1, pt_identity=[None, None])
