"""CPU: the exact model of hexl_rotate_hoisted (tests/hoist_model.py) against the oracle's keyswitch at g = 1, where the two must
agree word for word; as a rotation (decrypts to sigma_g of the message within the plain keyswitch's noise bound) and as NOT the words
of ckks_model.rotate at g != 1 -- the documented difference in the digit lift; and the entry point's presence in the built library
and its ctypes signature, with the null-pointer refusals that need no GPU."""
import ctypes

import numpy as np
import pytest

from ckks_model import first_mismatch, rotate
from hoist_model import GaloisRlwe, rotate_hoisted
from ks_util import KsCase, RlweCase, extreme_ciphertext, seal_chain

HEXL_E_BADARG = -1


def ct_of(orc, case, b):
    n, L = case.n, case.L
    return np.concatenate([orc.splitmix(n, case.seed * 31 + b * 977 + k * 17 + i, int(case.moduli[i]))
                           for k in range(2) for i in range(L)])


@pytest.mark.parametrize("n,L,K,chain", [(1024, 2, 3, "gen"), (2048, 3, 4, "seal")])
def test_identity_rotation_is_the_oracles_keyswitch(orc, n, L, K, chain):
    """g = 1: sigma is the identity, so steps 3-7 of the model are pinned to the oracle word for word"""
    case = KsCase(orc, n, L, K, seed=81, moduli=seal_chain(orc, K, n) if chain == "seal" else None)
    for ct in (ct_of(orc, case, 0), extreme_ciphertext(case, 1, 2)):
        got, want = rotate_hoisted(orc, case, ct, 1), rotate(orc, case, ct, 1)
        assert np.array_equal(got, want), first_mismatch(got, want, ("component", "limb", "coefficient"), (2, L, n))


@pytest.mark.parametrize("n,L,K,chain", [(1024, 2, 4, "gen"), (2048, 3, 5, "seal")])
def test_identity_rotation_with_more_key_moduli_than_digits_plus_one(orc, n, L, K, chain):
    """K = L + 2: the special prime is modulus K - 1 and modulus L is not used at all; the host keys keep K rows per component. The
    oracle's keyswitch takes rns_modulus_size = L + 1 (ckks_model.rotate), as the GPU tests of such plans do. An L where K - 1 belongs
    anywhere in the model -- slot list, key row, special prime -- would show here"""
    case = KsCase(orc, n, L, K, seed=81, moduli=seal_chain(orc, K, n) if chain == "seal" else None)
    assert int(case.moduli[L]) != int(case.moduli[K - 1]) and case.rns == L + 1
    for ct in (ct_of(orc, case, 0), extreme_ciphertext(case, 1, 2)):
        got, want = rotate_hoisted(orc, case, ct, 1), rotate(orc, case, ct, 1)
        assert np.array_equal(got, want), first_mismatch(got, want, ("component", "limb", "coefficient"), (2, L, n))
    unused = KsCase(orc, n, L, K, seed=81, moduli=case.moduli)
    for key in unused.keys:                                            # rows of the unused modulus L: read by nobody
        key.reshape(2, K, n)[:, L] = 0
    assert np.array_equal(rotate_hoisted(orc, unused, ct, 1), want), "the model read a key row of the unused modulus"


@pytest.fixture(scope="module")
def rlwe(orc):
    return RlweCase(orc, 1024, 2, 3, 50, seed=4)


@pytest.mark.parametrize("which", ["3", "5^3", "2n-1"])
def test_hoisted_rotation_decrypts_and_is_not_rotate(orc, rlwe, which):
    n = rlwe.n
    g = {"3": 3, "5^3": pow(5, 3, 2 * n), "2n-1": 2 * n - 1}[which]
    gr = GaloisRlwe(orc, rlwe, g)
    plain = rotate(orc, gr, gr.ct, g)
    gr.check(plain)                                                    # the yardstick: permute, then keyswitch
    hoisted = rotate_hoisted(orc, gr, gr.ct, g)
    gr.check(hoisted)
    assert not np.array_equal(hoisted, plain), "the hoisted digit lift must differ from rotate's for g != 1"


def test_entry_point_exists_and_refuses_null_pointers(hx):
    hx.build()
    lib = ctypes.CDLL(str(hx.LIB_PATH))
    name = "hexl_rotate_hoisted"
    assert name in hx.C_ABI, f"{name} missing from the ctypes table"
    assert hasattr(lib, name), f"{name} not exported by {hx.LIB_PATH.name}"
    fn = getattr(lib, name)
    fn.argtypes = hx.C_ABI[name]
    fn.restype = ctypes.c_int
    assert callable(hx.rotate_hoisted)
    buf = (ctypes.c_uint64 * 16)()
    word = ctypes.addressof(buf)
    plans = (ctypes.c_void_p * 1)(None)                                # an array that holds a null plan
    outs = (ctypes.c_void_p * 1)(word)
    gs = (ctypes.c_uint64 * 1)(3)
    ct = ctypes.c_void_p(word + 64)
    assert fn(None, gs, 1, outs, ct, 1) == HEXL_E_BADARG              # null plans
    assert fn(plans, gs, 1, None, ct, 1) == HEXL_E_BADARG             # null d_outs
    assert fn(plans, gs, 1, outs, None, 1) == HEXL_E_BADARG           # null d_ct
    assert fn(plans, None, 1, outs, ct, 1) == HEXL_E_BADARG           # null galois_elts
    assert fn(plans, gs, 1, outs, ct, 1) == HEXL_E_BADARG             # plans[0] is null
    assert fn(None, None, 0, None, None, 0) == HEXL_E_BADARG          # n_rot == 0 does not excuse null pointers
