"""Host models of hexl_rns_ntt_fwd / hexl_rns_ntt_inv (the oracle's keyswitch transforms, limb by limb) and hexl_multiply_plain
(Python-integer products), plus the moduli chains and input families their tests share. Layouts are the library's."""
import numpy as np

from ks_util import extreme_words, primes_below, primes_from, rounding_edge_coeffs, seal_chain, tier_ladder

BOUNDARY = (1 << 51) + (1 << 44)                                  # f64_arith.hpp LAZY_MAX_MODULUS: period 3 at and below, strict above


def chain(orc, kind, K, n):
    """K moduli of one family: uniformly in one tier (`plan.tiers()` of each is in TIER_OF), or mixed (seal, ladder)"""
    if kind == "strict":
        return primes_below(orc, K, 1 << 52, n)
    if kind == "period3_top":
        return primes_below(orc, K, BOUNDARY, n)
    if kind == "strict_bottom":
        return primes_from(orc, K, BOUNDARY, n)
    if kind == "period6":
        return primes_below(orc, K, 1 << 50, n)
    if kind == "period12":
        return primes_below(orc, K, 1 << 49, n)
    if kind == "seal":
        return seal_chain(orc, K, n)
    if kind == "ladder":
        return tier_ladder(orc, K, n)
    assert kind == "gen", kind
    return orc.primes(K, 51, n)


TIER_OF = {"strict": 0, "period3_top": 3, "strict_bottom": 0, "period6": 6, "period12": 12}


def rns_ntt(lm, x, n_limbs, inverse=False):
    """x[..., n_limbs, n] -> the same shape, polynomial (c, i) through Limbs.ntt / Limbs.intt of limb i"""
    x = np.asarray(x, dtype=np.uint64)
    flat = x.reshape(-1, n_limbs, lm.n)
    f = lm.intt if inverse else lm.ntt
    return np.stack([np.stack([f(c[i], i) for i in range(n_limbs)]) for c in flat]).reshape(x.shape)


def ntt_input(lm, n_limbs, family, c, seed=1, inverse=False):
    """polynomial set c of a transform input [n_limbs][n], every word below its modulus:
    uniform   splitmix words
    extreme   ks_util.extreme_words (q - 1, beside q / 2, 0, 1) in every limb
    zero      the all-zero polynomial
    edge      (inverse only) NTT_i(rounding_edge_coeffs): the inverse's output is exactly 0, 1, half - 1 ... half + 2, q - 2, q - 1"""
    out = np.empty((n_limbs, lm.n), dtype=np.uint64)
    for i in range(n_limbs):
        q = lm.qs[i]
        if family == "uniform":
            out[i] = lm.orc.splitmix(lm.n, seed * 1013 + c * 101 + i, q)
        elif family == "extreme":
            out[i] = extreme_words(lm.n, q, c * 5 + i + seed)
        elif family == "zero":
            out[i] = 0
        else:
            assert family == "edge" and inverse, family
            out[i] = lm.ntt(rounding_edge_coeffs(lm.n, q, c * 3 + i + seed), i)
    return out


def multiply_plain(qs, n, ct, pt, n_components, n_limbs, prev=None):
    """ct[n_components][n_limbs][n] * pt[n_limbs][n] mod q_i (+ prev of ct's shape), in Python integers"""
    ct = np.asarray(ct, dtype=np.uint64).reshape(n_components, n_limbs, n).astype(object)
    pt = np.asarray(pt, dtype=np.uint64).reshape(n_limbs, n).astype(object)
    out = np.empty((n_components, n_limbs, n), dtype=np.uint64)
    acc = None if prev is None else np.asarray(prev, dtype=np.uint64).reshape(n_components, n_limbs, n).astype(object)
    for k in range(n_components):
        for i in range(n_limbs):
            v = ct[k, i] * pt[i]
            if acc is not None:
                v = v + acc[k, i]
            out[k, i] = np.array(v % int(qs[i]), dtype=np.uint64)
    return out


def negacyclic_product(a, b, q):
    """a(X) b(X) mod (X^n + 1, q) for two coefficient vectors, in Python integers (schoolbook by rows of a)"""
    n = len(a)
    a = [int(v) for v in a]
    bo = np.asarray(b, dtype=np.uint64).astype(object)
    acc = np.zeros(2 * n, dtype=object)
    for j, aj in enumerate(a):
        if aj:
            acc[j:j + n] += aj * bo
    return np.array((acc[:n] - acc[n:]) % q, dtype=np.uint64)


def assert_instances(got, want, count, shape_names, shape, label):
    """got[count][...] against want[c % len(want)], every instance; the first wrong word is named (ckks_model.first_mismatch)"""
    from ckks_model import first_mismatch
    got = np.asarray(got).reshape(count, -1)
    for c in range(count):
        w = np.asarray(want[c % len(want)]).reshape(-1)
        if not np.array_equal(got[c], w):
            raise AssertionError(f"{label}: instance {c}, {first_mismatch(got[c], w, shape_names, shape)}")
