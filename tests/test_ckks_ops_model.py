"""CPU: the two formulas behind hexl_apply_galois / hexl_rotate and hexl_rescale against the oracle, and the argument checks of
the three entry points (no device needed: a null handle or a bad argument is refused before any HIP call)."""
import ctypes

import numpy as np
import pytest

from ckks_model import Limbs, apply_galois, automorphism_coeff, rescale_crt, rescale_input, rescale_poly
from ks_util import big_dropped, primes_below, seal_chain, small_dropped, tier_ladder

HEXL_E_BADARG = -1


def galois_elts(n):
    return [1, 3, 5, pow(5, 7, 2 * n), 2 * n - 1]


@pytest.mark.parametrize("n", [1024, 16384])
def test_galois_permutation_is_the_automorphism_in_ntt_form(orc, n):
    """NTT(a(X^g)) == perm_g(NTT(a)), through the standalone NTT tables and through the keyswitch's transform"""
    q = orc.primes(1, 50, n)[0]
    t = orc.HexlTables(n, q)
    lm = Limbs(orc, n, [q])
    a = orc.splitmix(n, 11, q)
    for g in galois_elts(n):
        rot = automorphism_coeff(a, n, g, q)
        assert np.array_equal(orc.ntt_fwd(rot, t)[0], apply_galois(orc.ntt_fwd(a, t)[0], n, g)), f"standalone NTT, g = {g}"
        assert np.array_equal(lm.ntt(rot, 0), apply_galois(lm.ntt(a, 0), n, g)), f"keyswitch NTT, g = {g}"


def test_galois_permutation_composes(orc):
    n = 2048
    x = orc.splitmix(n, 5)
    g, h = 5, pow(5, 3, 2 * n)
    assert np.array_equal(apply_galois(apply_galois(x, n, g), n, h), apply_galois(x, n, g * h % (2 * n)))
    assert np.array_equal(apply_galois(x, n, 1), x)


@pytest.mark.parametrize("n,moduli", [(1024, "gen"), (1024, "seal"), (2048, "gen")])
def test_rescale_formula_is_rounded_division(orc, n, moduli):
    """out_i = (c_i - NTT_i((s + fix_i) mod q_i)) q_l^-1 equals NTT_i(round(X / q_l) mod q_i) (big-integer CRT)"""
    qs = orc.primes(5, 51, n) if moduli == "gen" else seal_chain(orc, 5, n)
    lm = Limbs(orc, n, qs)
    for n_limbs in (2, 3, 4):
        c = np.stack([orc.splitmix(n, 100 * n_limbs + i, qs[i]) for i in range(n_limbs)])
        assert np.array_equal(rescale_poly(lm, c, n_limbs), rescale_crt(lm, c, n_limbs)), n_limbs


def test_rescale_formula_at_the_ends_of_the_range(orc):
    n = 1024
    qs = orc.primes(4, 50, n)
    lm = Limbs(orc, n, qs)
    for fill in (0, 1, -1):
        c = np.stack([np.full(n, fill % q, dtype=np.uint64) for q in qs])
        assert np.array_equal(rescale_poly(lm, c, 4), rescale_crt(lm, c, 4)), fill


EDGE_CHAINS = {"seal": lambda orc, n: seal_chain(orc, 7, n), "ladder": lambda orc, n: tier_ladder(orc, 8, n),
               "strict": lambda orc, n: primes_below(orc, 5, 1 << 52, n), "period6": lambda orc, n: primes_below(orc, 5, 1 << 50, n),
               "period12": lambda orc, n: primes_below(orc, 5, 1 << 49, n), "big_dropped": big_dropped, "small_dropped": small_dropped}


@pytest.mark.parametrize("kind", list(EDGE_CHAINS))
def test_rescale_formula_on_rounding_edges_and_extreme_words(orc, kind):
    """the model the GPU tests compare with equals big-integer CRT rounding on the very inputs they use: the dropped limb's INTT at 0, 1,
    half - 1 ... half + 2, q_l - 2, q_l - 1 beside extreme kept limbs ("edge"), and every limb extreme in NTT form ("extreme"), for
    every n_limbs the chain admits (2 ... K - 1), three instances (= patterns) each"""
    n = 1024
    qs = EDGE_CHAINS[kind](orc, n)
    lm = Limbs(orc, n, qs)
    for n_limbs in range(2, len(qs)):
        for family in ("edge", "extreme"):
            for b in range(3):
                c = rescale_input(lm, n_limbs, 1, family, b, seed=n_limbs)[0]
                if family == "edge":                              # the dropped limb's coefficients are the edge words themselves
                    half, ql = qs[n_limbs - 1] >> 1, qs[n_limbs - 1]
                    assert set(int(v) for v in lm.intt(c[n_limbs - 1], n_limbs - 1)) <= {0, 1, half - 1, half, half + 1, half + 2, ql - 2, ql - 1}
                assert np.array_equal(rescale_poly(lm, c, n_limbs), rescale_crt(lm, c, n_limbs)), (n_limbs, family, b)


def test_new_entry_points_refuse_a_null_handle(hx):
    """hexl_apply_galois / hexl_rescale / hexl_rotate exist in the library and refuse what they cannot run on"""
    hx.build()
    lib = ctypes.CDLL(str(hx.LIB_PATH))
    for name in ("hexl_apply_galois", "hexl_rescale", "hexl_rotate"):
        assert name in hx.C_ABI
        fn = getattr(lib, name)
        fn.argtypes = hx.C_ABI[name]
        fn.restype = ctypes.c_int
    buf = (ctypes.c_uint64 * 16)()
    a, b = ctypes.addressof(buf), ctypes.addressof(buf) + 8 * 8
    assert lib.hexl_apply_galois(None, a, b, 1, 1024, 3) == HEXL_E_BADARG
    assert lib.hexl_rescale(None, a, b, 1, 2, 2) == HEXL_E_BADARG
    assert lib.hexl_rotate(None, a, b, 1, 3) == HEXL_E_BADARG
    assert lib.hexl_apply_galois(None, None, None, 0, 1024, 3) == HEXL_E_BADARG
