"""CPU: the host model of hexl_hks_keygen (tests/hks_keygen_model.py) against what its definition claims, at n = 16, L = 3, K = 5
(n_p = 2) with keys of alpha = 2, 1, 3 in one set (a ragged last digit, the per-limb gadget, one digit) and every kind:
  * c0 + a s - P [i in G_d] s' inverse-transforms, at EVERY one of the K limbs, to a polynomial of infinity norm <= 21 (centred) --
  * -- the same integer polynomial at all K limbs, and it is the CBD21 polynomial of the row's index;
  * row (r, d) draws polynomial first + sum_{r' < r} dnum_r' + d of (seed, stream): its mask is that UNIFORM polynomial, word for word,
    and a set split into two calls with `first` advanced gives the same words."""
import numpy as np
import pytest

import hks_keygen_model as km
import sample_model as sm
from ckks_model import Limbs

N, L, K = 16, 3, 5
ALPHAS = [2, 1, 3, 2]
KINDS = [km.FROM_SQUARE, km.FROM_GALOIS, km.FROM_GALOIS, km.FROM_POLY]
ELTS = [4, 5, 2 * N - 1, 0]                                       # the entries of other kinds are ignored
SEED = bytes((37 * k + 11) & 0xFF for k in range(32))
STREAM, FIRST = 0xFEDCBA9876543210, 1000


@pytest.fixture(scope="module")
def setup(orc):
    qs = [int(q) for q in orc.primes(K, 45, N)]
    lm = Limbs(orc, N, qs)
    s = sm.sample(lm, sm.TERNARY, SEED, 1, 0, 1, K)[0]
    poly = sm.sample(lm, sm.UNIFORM, SEED, 9, 0, 1, K)[0]
    keys, models = km.key_set(orc, N, L, K, qs, ALPHAS, KINDS, ELTS, [None, None, None, poly], s, SEED, STREAM, FIRST, lm=lm)
    return qs, lm, s, poly, keys, models


def centred(v, q):
    return np.array([int(x) - q if int(x) > q // 2 else int(x) for x in v], dtype=object)


def test_the_index_of_a_row_is_the_prefix_sum(setup):
    qs, lm, s, poly, keys, models = setup
    dnums = [m.dnum for m in models]
    assert dnums == [2, 3, 1, 2]
    assert [km.first_of(dnums, FIRST, r) for r in range(4)] == [FIRST, FIRST + 2, FIRST + 5, FIRST + 6]
    for r, m in enumerate(models):
        rows = m.key_word_rows(keys[r])
        for d in range(m.dnum):
            c = FIRST + sum(dnums[:r]) + d
            for i in range(K):
                assert np.array_equal(rows[d, 1, i], sm.uniform(SEED, STREAM, c, i, N, qs[i])), (r, d, i)


def test_every_row_is_an_encryption_of_its_plaintext_with_one_small_error(setup):
    qs, lm, s, poly, keys, models = setup
    dnums = [m.dnum for m in models]
    for r, m in enumerate(models):
        s_from = km.from_words(m, s, KINDS[r], ELTS[r], poly if KINDS[r] == km.FROM_POLY else None)
        rows = m.key_word_rows(keys[r])
        digits = m.digits(L)
        assert sorted(i for G in digits for i in G) == list(range(L)) and len(digits) == m.dnum
        for d in range(m.dnum):
            errs = []
            for i in range(K):
                q = qs[i]
                v = rows[d, 0, i].astype(object) + rows[d, 1, i].astype(object) * s[i].astype(object)
                if i in digits[d]:
                    v = v - (m.P % q) * s_from[i].astype(object)
                e = centred(lm.intt(np.array(v % q, dtype=np.uint64), i), q)
                assert max(abs(int(x)) for x in e) <= 21, (r, d, i)
                errs.append(e)
            for i in range(1, K):
                assert np.array_equal(errs[i], errs[0]), f"key {r} row {d}: limb {i} holds another error polynomial than limb 0"
            want = sm.small(SEED, STREAM, sm.CBD21, FIRST + sum(dnums[:r]) + d, N)
            assert np.array_equal(errs[0], want.astype(object)), (r, d)


def test_the_special_limbs_and_the_other_digits_encrypt_zero(setup):
    qs, lm, s, poly, keys, models = setup
    m = models[0]
    for d in range(m.dnum):
        pt = km.plaintext(m, d, km.from_words(m, s, km.FROM_SQUARE))
        for i in range(K):
            assert bool(pt[i].any()) == (i in m.digits(L)[d]), (d, i)


def test_a_set_split_into_two_calls_gives_the_same_words(setup, orc):
    qs, lm, s, poly, keys, models = setup
    dnums = [m.dnum for m in models]
    head, _ = km.key_set(orc, N, L, K, qs, ALPHAS[:2], KINDS[:2], ELTS[:2], None, s, SEED, STREAM, FIRST, lm=lm)
    tail, _ = km.key_set(orc, N, L, K, qs, ALPHAS[2:], KINDS[2:], ELTS[2:], [None, poly], s, SEED, STREAM, FIRST + sum(dnums[:2]), lm=lm)
    for r, k in enumerate(head + tail):
        assert np.array_equal(k, keys[r]), r


def test_the_square_and_the_galois_source_are_what_the_device_routes_make(setup):
    """s' of the two derived kinds: the limb-wise square, and the permutation hexl_apply_galois applies (g = 1: the identity)"""
    qs, lm, s, poly, keys, models = setup
    m = models[0]
    sq = km.from_words(m, s, km.FROM_SQUARE)
    for i in range(K):
        assert all(int(sq[i][j]) == int(s[i][j]) ** 2 % qs[i] for j in range(N))
    assert np.array_equal(km.from_words(m, s, km.FROM_GALOIS, 1), s)
    rot = km.from_words(m, s, km.FROM_GALOIS, 5)
    assert not np.array_equal(rot, s) and all(sorted(rot[i]) == sorted(s[i]) for i in range(K))
