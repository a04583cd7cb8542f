"""CPU: the Python-integer model of hexl_ct_tensor_sum / hexl_relinearize / hexl_multiply_sum_relinearize (tests/tensor_model.py), pinned
on what the oracle already has: one term is orc.dyadic(..., exact=True); a sum is its per-term results added modulo q_i; an operand with
more limbs is read through its first n_limbs; and the relinearised sum is the oracle's key switch on the split components."""
import numpy as np

from ks_util import KsCase
from rns_model import chain
from tensor_model import ct_tensor_sum, multiply_sum_relinearize, relinearize

N, K = 1024, 5


def words(orc, qs, n_limbs, seed):
    """one two-component operand [2][n_limbs][N]"""
    return np.array([[orc.splitmix(N, seed + 16 * k + i, qs[i]) for i in range(n_limbs)] for k in range(2)])


def test_one_term_is_the_dyadic_multiply(orc):
    for kind in ("strict", "seal"):
        qs = chain(orc, kind, K, N)
        a, b = words(orc, qs, K, 3), words(orc, qs, K, 7)
        want = orc.dyadic(a.reshape(-1), b.reshape(-1), N, np.array(qs, dtype=np.uint64), exact=True)
        assert np.array_equal(ct_tensor_sum(qs, N, [a], [b], K).reshape(-1), want)
        square = orc.dyadic(a.reshape(-1), a.reshape(-1), N, np.array(qs, dtype=np.uint64), exact=True)
        assert np.array_equal(ct_tensor_sum(qs, N, [a], [a], K).reshape(-1), square)


def test_a_sum_is_its_terms_added(orc):
    qs = chain(orc, "period3_top", K, N)
    a_s = [words(orc, qs, K, 100 + 5 * t) for t in range(8)]
    b_s = [words(orc, qs, K, 900 + 5 * t) for t in range(8)]
    mod = np.array(qs, dtype=object).reshape(1, K, 1)
    for T in (2, 3, 8):
        acc = np.zeros((3, K, N), dtype=object)
        for t in range(T):
            acc = acc + ct_tensor_sum(qs, N, [a_s[t]], [b_s[t]], K).astype(object)
        assert np.array_equal(ct_tensor_sum(qs, N, a_s[:T], b_s[:T], K), np.array(acc % mod, dtype=np.uint64))


def test_operands_with_more_limbs_are_read_through_their_first(orc):
    qs = chain(orc, "seal", K, N)
    n_limbs = 3
    a, b, c = words(orc, qs, K, 11), words(orc, qs, n_limbs + 1, 13), words(orc, qs, n_limbs, 17)
    cut = lambda x: np.ascontiguousarray(x[:, :n_limbs])
    want = ct_tensor_sum(qs, N, [cut(a), cut(b)], [cut(b), c], n_limbs)
    poisoned = [a.copy(), b.copy()]
    for x in poisoned:
        x[:, n_limbs:] = np.uint64(0xFFFFFFFFFFFFFFFF)             # no residue: never read
    got = ct_tensor_sum(qs, N, [poisoned[0].reshape(-1), poisoned[1]], [poisoned[1], c], n_limbs, in_limbs=[[K, n_limbs + 1], [n_limbs + 1, n_limbs]])
    assert np.array_equal(got, want)


def test_relinearised_sum_is_the_keyswitch_on_the_split_components(orc):
    L = 2
    case = KsCase(orc, N, L, L + 1, seed=3)
    qs = [int(q) for q in case.moduli]
    a_s = [words(orc, qs, L, 40 + t) for t in range(2)]
    b_s = [words(orc, qs, L, 60 + t) for t in range(2)]
    ct3 = ct_tensor_sum(qs, N, a_s, b_s, L)
    t, r = ct3[2].reshape(-1).copy(), ct3[:2].reshape(-1).copy()
    want = case.expected(orc, t, r)
    assert np.array_equal(relinearize(orc, case, ct3), want)
    assert np.array_equal(multiply_sum_relinearize(orc, case, a_s, b_s), want)
    assert not np.array_equal(want, r), "the key switch added nothing"
