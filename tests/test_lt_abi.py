"""CPU: hexl_linear_transform exists in the built library and in the ctypes table, with the wrapper beside it, and refuses the null
pointers and the empty rotation list that need no GPU to refuse."""
import ctypes

HEXL_E_BADARG = -1
NAME = "hexl_linear_transform"


def test_linear_transform_entry_point_and_null_refusals(hx):
    hx.build()
    lib = ctypes.CDLL(str(hx.LIB_PATH))
    assert NAME in hx.C_ABI, f"{NAME} missing from the ctypes table"
    assert hasattr(lib, NAME), f"{NAME} not exported by {hx.LIB_PATH.name}"
    vp, u64, sz = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_size_t
    assert hx.C_ABI[NAME] == [ctypes.POINTER(vp), ctypes.POINTER(u64), ctypes.POINTER(vp), sz, vp, vp, vp, sz]
    fn = getattr(lib, NAME)
    fn.argtypes = hx.C_ABI[NAME]
    fn.restype = ctypes.c_int
    assert callable(hx.linear_transform) and "linear_transform" in hx.__all__
    buf = (u64 * 32)()
    word = ctypes.addressof(buf)
    plans = (vp * 1)(None)                                             # an array that holds a null plan
    pts = (vp * 1)(word)
    gs = (u64 * 1)(3)
    out, ct = vp(word + 64), vp(word + 128)
    assert fn(None, gs, pts, 1, None, out, ct, 1) == HEXL_E_BADARG    # null plans
    assert fn(plans, None, pts, 1, None, out, ct, 1) == HEXL_E_BADARG # null galois_elts
    assert fn(plans, gs, None, 1, None, out, ct, 1) == HEXL_E_BADARG  # null d_pts
    assert fn(plans, gs, pts, 1, None, None, ct, 1) == HEXL_E_BADARG  # null d_out
    assert fn(plans, gs, pts, 1, None, out, None, 1) == HEXL_E_BADARG # null d_ct
    assert fn(plans, gs, pts, 1, None, out, ct, 1) == HEXL_E_BADARG   # plans[0] is null
    assert fn(plans, gs, pts, 0, None, out, ct, 1) == HEXL_E_BADARG   # n_rot == 0: refused before plans[0] is looked at
    assert fn(None, None, None, 0, None, None, None, 0) == HEXL_E_BADARG


def test_wrapper_wants_one_plaintext_per_rotation(hx):
    import pytest
    with pytest.raises(ValueError):
        hx.linear_transform([None, None], [3, 5], [None], None, None, 1)
