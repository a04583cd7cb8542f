"""CPU: the Python-integer model of hexl_ct_lincomb (tests/lincomb_model.py), pinned on identities: weights (1, q - 1) on (a, a) give zero;
one term of weight 1 with a larger in_limbs is the limb-dropping copy; a weight equal to the constant word of a plaintext gives
rns_model.multiply_plain; and the addends reach component 0 only."""
import numpy as np

from lincomb_model import ct_lincomb
from rns_model import chain, multiply_plain

N, K = 1024, 5


def words(orc, qs, n_components, n_limbs, seed):
    return np.array([[orc.splitmix(N, seed + 16 * k + i, qs[i]) for i in range(n_limbs)] for k in range(n_components)])


def test_a_minus_a_is_zero(orc):
    qs = chain(orc, "seal", K, N)
    a = words(orc, qs, 2, K, 3)
    out = ct_lincomb(qs, N, [a, a], 2, K, weights=[[1] * K, [q - 1 for q in qs]])
    assert not out.any()
    assert np.array_equal(ct_lincomb(qs, N, [a, a], 2, K), (a + a) % np.array(qs, dtype=np.uint64).reshape(1, K, 1))


def test_one_term_of_weight_one_drops_limbs(orc):
    qs = chain(orc, "seal", K, N)
    a = words(orc, qs, 3, K, 5)
    for n_limbs in (1, 3, K):
        for weights in (None, [[1] * n_limbs]):
            out = ct_lincomb(qs, N, [a.reshape(-1)], 3, n_limbs, weights=weights, in_limbs=[K])
            assert np.array_equal(out, a[:, :n_limbs])


def test_constant_weight_is_multiply_plain_by_a_constant_word_plaintext(orc):
    qs = chain(orc, "strict", K, N)
    a, prev = words(orc, qs, 2, K, 7), words(orc, qs, 2, K, 11)
    w = [int(orc.splitmix(1, 100 + i, q)[0]) for i, q in enumerate(qs)]
    pt = np.array([np.full(N, w[i], dtype=np.uint64) for i in range(K)])
    assert np.array_equal(ct_lincomb(qs, N, [a], 2, K, weights=[w]), multiply_plain(qs, N, a, pt, 2, K))
    # with the previous output as a second term of weight 1: the accumulating form
    assert np.array_equal(ct_lincomb(qs, N, [a, prev], 2, K, weights=[w, [1] * K]), multiply_plain(qs, N, a, pt, 2, K, prev=prev))


def test_addends_reach_component_zero_only(orc):
    qs = chain(orc, "period12", K, N)
    n_limbs = 3
    a, b = words(orc, qs, 2, n_limbs + 1, 13), words(orc, qs, 2, n_limbs, 17)
    pt = words(orc, qs, 1, n_limbs, 19)[0]
    const = [q - 1 - i for i, q in enumerate(qs[:n_limbs])]
    w = [[q - 2 for q in qs[:n_limbs]], [3] * n_limbs]
    plain = ct_lincomb(qs, N, [a, b], 2, n_limbs, weights=w, in_limbs=[n_limbs + 1, n_limbs])
    full = ct_lincomb(qs, N, [a, b], 2, n_limbs, weights=w, in_limbs=[n_limbs + 1, n_limbs], pt=pt, const=const)
    assert np.array_equal(full[1], plain[1])
    for i in range(n_limbs):
        want = (plain[0, i].astype(object) + pt[i].astype(object) + const[i]) % qs[i]
        assert np.array_equal(full[0, i], np.array(want, dtype=np.uint64))
        # by hand: -2 a + 3 b
        by_hand = (3 * b[1, i].astype(object) - 2 * a[1, i].astype(object)) % qs[i]
        assert np.array_equal(plain[1, i], np.array(by_hand, dtype=np.uint64))
