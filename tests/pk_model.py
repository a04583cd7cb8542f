"""Host model of hexl_pk_encrypt (include/hexl_mi355x.h) in Python integers, from the definition: instance c takes the
TERNARY polynomial c and the CBD21 polynomials 2c and 2c + 1 of (seed, stream), each as NTT_i(v mod q_i) (sample_model.small /
small_words), and out = (pk0 u + e0 + pt, pk1 u + e1) mod q_i word by word. Layouts are the library's."""
import numpy as np

import sample_model as sm

MAX_FIRST_PLUS_COUNT = 1 << 39            # first + count <= 2^39 keeps the CBD21 indices 2c + 1 below sample_model.MAX_INDEX


def indices(c):
    """absolute polynomial indices instance c consumes: (TERNARY, CBD21 of e0, CBD21 of e1)"""
    assert 0 <= c < MAX_FIRST_PLUS_COUNT
    return c, 2 * c, 2 * c + 1


def small_polys(seed, stream, c, n):
    """the three integer polynomials (u, e0, e1) of instance c"""
    t, a, b = indices(c)
    return sm.small(seed, stream, sm.TERNARY, t, n), sm.small(seed, stream, sm.CBD21, a, n), sm.small(seed, stream, sm.CBD21, b, n)


def pk_encrypt(lm, seed, stream, c, n_limbs, pk, pt=None):
    """one instance of hexl_pk_encrypt, absolute index c: pk[2][>= n_limbs][n] (rows beyond n_limbs are not read), pt None or
    [n_limbs][n]; returns [2][n_limbs][n]"""
    u, e0, e1 = small_polys(seed, stream, c, lm.n)
    out = np.empty((2, n_limbs, lm.n), dtype=np.uint64)
    for i in range(n_limbs):
        q = lm.qs[i]
        uw = sm.small_words(lm, u, i).astype(object)
        c0 = np.asarray(pk[0][i]).astype(object) * uw + sm.small_words(lm, e0, i).astype(object)
        if pt is not None:
            c0 = c0 + np.asarray(pt[i]).astype(object)
        c1 = np.asarray(pk[1][i]).astype(object) * uw + sm.small_words(lm, e1, i).astype(object)
        out[0, i] = np.array(c0 % q, dtype=np.uint64)
        out[1, i] = np.array(c1 % q, dtype=np.uint64)
    return out


def public_key(lm, seed, stream, c, n_limbs, s):
    """(e - a s, a) at n_limbs limbs: hexl_rlwe_encrypt(d_pt = NULL, count = 1, first = c)"""
    return sm.encrypt(lm, seed, stream, c, n_limbs, s, None)


def centred(x, q):
    """residues [n] -> the integers of (-q/2, q/2]"""
    x = np.asarray(x).astype(object)
    return np.where(x > q // 2, x - q, x)


def negacyclic_int(a, b):
    """a(X) b(X) mod X^n + 1 over the integers (small coefficients: int64 is ample)"""
    n = len(a)
    full = np.convolve(np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64))
    out = full[:n].copy()
    out[:n - 1] -= full[n:]
    return out


def noise(pk_seed, pk_stream, pk_c, s_int, seed, stream, c, n):
    """the exact noise of decrypt(pk_encrypt(pt)) - pt as integers: e_pk u + e0 + e1 s (negacyclic), with e_pk the CBD21 polynomial pk_c of
    the key's (seed, stream) and s_int the secret's integer coefficients. |.| <= (2n + 1) 21."""
    u, e0, e1 = small_polys(seed, stream, c, n)
    e_pk = sm.small(pk_seed, pk_stream, sm.CBD21, pk_c, n)
    return negacyclic_int(e_pk, u) + e0 + negacyclic_int(e1, s_int)
