"""CPU: tests/pk_model.py pinned -- the model of hexl_pk_encrypt equals the normative four-call composition built from the models of
hexl_sample, hexl_multiply_plain and hexl_ct_lincomb; decrypt(pk_encrypt(pt)) - pt is exactly the integer polynomial e_pk u + e0 + e1 s
in every limb; instance c consumes TERNARY c and CBD21 2c, 2c + 1; a key kept at K limbs serves a lower level word for word."""
import numpy as np

import pk_model as pm
import sample_model as sm
from ckks_model import Limbs
from ks_util import primes_below
from lincomb_model import ct_lincomb
from rns_model import multiply_plain

N, K = 1024, 3
SEED, PK_SEED = bytes(range(40, 72)), bytes(range(7, 39))


def setup(orc):
    qs = primes_below(orc, 1, 1 << 52, N) + primes_below(orc, 1, 1 << 30, N) + primes_below(orc, 1, 1 << 27, N)
    lm = Limbs(orc, N, qs)
    sv = sm.small(PK_SEED, 1, sm.TERNARY, 0, N)
    s = np.stack([sm.small_words(lm, sv, i) for i in range(K)])
    return lm, sv, s


def test_model_is_the_four_call_composition(orc):
    lm, _, s = setup(orc)
    pk = pm.public_key(lm, PK_SEED, 2, 0, K, s)
    first, count, stream = 5, 2, 9
    for n_limbs in (1, K):
        pts = np.array([[orc.splitmix(N, 60 + 7 * b + i, lm.qs[i]) for i in range(n_limbs)] for b in range(count)])
        U = sm.sample(lm, sm.TERNARY, SEED, stream, first, count, n_limbs)
        E = sm.sample(lm, sm.CBD21, SEED, stream, 2 * first, 2 * count, n_limbs).reshape(count, 2, n_limbs, N)
        for b in range(count):
            T = multiply_plain(lm.qs, N, pk[:, :n_limbs], U[b], 2, n_limbs)
            for pt in (None, pts[b]):
                want = ct_lincomb(lm.qs, N, [T, E[b]], 2, n_limbs, pt=pt)
                assert np.array_equal(pm.pk_encrypt(lm, SEED, stream, first + b, n_limbs, pk, pt), want)


def test_decrypt_leaves_exactly_the_noise_polynomial(orc):
    lm, sv, s = setup(orc)
    pk = pm.public_key(lm, PK_SEED, 2, 3, K, s)
    pt = np.stack([orc.splitmix(N, 77 + i, lm.qs[i]) for i in range(K)])
    c, stream = 12345, 4
    want = pm.noise(PK_SEED, 2, 3, sv, SEED, stream, c, N)
    assert np.abs(want).max() <= (2 * N + 1) * 21 and np.abs(want).max() > 21      # the products are there
    for plain in (pt, None):
        ct = pm.pk_encrypt(lm, SEED, stream, c, K, pk, plain)
        dec = sm.decrypt(lm.qs, N, ct, s, 2, K)
        for i in range(K):
            diff = np.array((dec[i].astype(object) - (0 if plain is None else plain[i].astype(object))) % lm.qs[i], dtype=np.uint64)
            assert np.array_equal(pm.centred(lm.intt(diff, i), lm.qs[i]).astype(np.int64), want), f"limb {i}"


def test_index_map(orc):
    lm, _, s = setup(orc)
    pk = pm.public_key(lm, PK_SEED, 2, 0, 1, s)
    top = (1 << 39) - 1
    assert pm.indices(0) == (0, 0, 1) and pm.indices(5) == (5, 10, 11) and pm.indices(top) == (top, (1 << 40) - 2, (1 << 40) - 1)
    assert pm.indices(top)[2] < sm.MAX_INDEX
    q = lm.qs[0]
    for c in (0, 5, top):
        ct = pm.pk_encrypt(lm, SEED, 3, c, 1, pk)
        u = sm.sample(lm, sm.TERNARY, SEED, 3, c, 1, 1)[0, 0].astype(object)
        e = sm.sample(lm, sm.CBD21, SEED, 3, 2 * c, 2, 1)[:, 0].astype(object)
        assert np.array_equal(ct[0, 0], np.array((pk[0, 0].astype(object) * u + e[0]) % q, dtype=np.uint64))
        assert np.array_equal(ct[1, 0], np.array((pk[1, 0].astype(object) * u + e[1]) % q, dtype=np.uint64))
    # neighbours share nothing: instance c + 1 takes the next mask and the next PAIR of errors
    a, b = pm.small_polys(SEED, 3, 5, N), pm.small_polys(SEED, 3, 6, N)
    assert all(not np.array_equal(x, y) for x in a for y in b)
    assert np.array_equal(b[1], sm.small(SEED, 3, sm.CBD21, 12, N))


def test_a_key_at_K_limbs_serves_every_level(orc):
    lm, _, s = setup(orc)
    full = pm.public_key(lm, PK_SEED, 2, 1, K, s)
    pt = np.stack([orc.splitmix(N, 90 + i, lm.qs[i]) for i in range(K)])
    for n_limbs in (1, 2):
        low = pm.public_key(lm, PK_SEED, 2, 1, n_limbs, s)
        assert np.array_equal(full[:, :n_limbs], low)
        assert np.array_equal(pm.pk_encrypt(lm, SEED, 8, 3, n_limbs, full, pt), pm.pk_encrypt(lm, SEED, 8, 3, n_limbs, low, pt))
        assert np.array_equal(pm.pk_encrypt(lm, SEED, 8, 3, n_limbs, full, pt), pm.pk_encrypt(lm, SEED, 8, 3, K, full, pt)[:, :n_limbs])
