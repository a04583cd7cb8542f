"""Host model of hexl_hks_keygen (include/hexl_mi355x.h) from its definition, in Python integers: the ChaCha streams of
tests/sample_model.py, the digits and P of tests/hks_model.py.

    key r of a call switches from s'_r to s and owns the rows first_r ... first_r + dnum_r - 1, first_r = first + sum_{r' < r} dnum_r'
    row (r, d) = (pt + e - a s, a) modulo all K limbs: a = UNIFORM, e = CBD21 polynomial first_r + d of (seed, stream),
    pt_i = (P mod q_i) s'_(r,i) for i in G_d, 0 at every other limb (the special primes included)

Layouts are the library's: a key is [dnum][2][K][n] (hexl_hks_set_keys_device), the secret and s' are [K][n] in NTT form."""
import numpy as np

import sample_model as sm
from ckks_model import apply_galois
from hks_model import Hks

FROM_POLY, FROM_SQUARE, FROM_GALOIS = 0, 1, 2


def first_of(dnums, first, r):
    """first_r: the polynomial index of row (r, 0)"""
    return first + sum(dnums[:r])


def from_words(hks, s, kind, g=1, poly=None):
    """s'[K][n] for a kind: the caller's polynomial, s_i s_i mod q_i, or the hexl_apply_galois permutation of s"""
    s = np.asarray(s, dtype=np.uint64).reshape(hks.K, hks.n)
    if kind == FROM_POLY:
        return np.asarray(poly, dtype=np.uint64).reshape(hks.K, hks.n)
    if kind == FROM_SQUARE:
        return np.stack([np.array(s[i].astype(object) * s[i].astype(object) % hks.qs[i], dtype=np.uint64) for i in range(hks.K)])
    assert kind == FROM_GALOIS and g & 1 and g < 2 * hks.n
    return apply_galois(s, hks.n, g)


def plaintext(hks, d, s_from):
    """pt[K][n] of row d: (P mod q_i) s'_i for i in G_d, else 0"""
    pt = np.zeros((hks.K, hks.n), dtype=np.uint64)
    for i in hks.digits(hks.L)[d]:
        pt[i] = np.array(np.asarray(s_from[i]).astype(object) * (hks.P % hks.qs[i]) % hks.qs[i], dtype=np.uint64)
    return pt


def key_row(hks, seed, stream, c, d, s, s_from):
    """row d of a key whose polynomial index is c: [2][K][n]"""
    s = np.asarray(s, dtype=np.uint64).reshape(hks.K, hks.n)
    return sm.encrypt(hks.lm, seed, stream, c, hks.K, s, plaintext(hks, d, s_from))


def key(hks, seed, stream, first_r, s, s_from):
    """one key, flat [dnum][2][K][n]"""
    assert first_r + hks.dnum <= sm.MAX_INDEX
    return np.stack([key_row(hks, seed, stream, first_r + d, d, s, s_from) for d in range(hks.dnum)]).reshape(-1)


def key_set(orc, n, L, K, moduli, alphas, kinds, elts, polys, s, seed, stream, first, lm=None):
    """the keys of one hexl_hks_keygen call: a list of flat [dnum_r][2][K][n] arrays, and the models (one Hks per key, sharing the
    transforms)"""
    models = []
    for alpha in alphas:
        models.append(Hks(orc, n, L, K, alpha, moduli, lm=lm or (models[0].lm if models else None)))
    dnums = [m.dnum for m in models]
    keys = [key(m, seed, stream, first_of(dnums, first, r), s, from_words(m, s, kinds[r], elts[r] if elts else 1, polys[r] if polys else None))
            for r, m in enumerate(models)]
    return keys, models
