"""CPU: the hybrid multiply's host model (tests/hks_mul_model.py) against what its definition claims, at the smallest ring the oracle's
transforms take (n = 2) and at n = 16, L = 3, K = 5, alpha = 2 (n_p = 2), levels 2 and 3:
  * out_k = round(X_k / R) - e with e in {0 ... n_p} for EVERY coefficient, X_k rebuilt by CRT over Q_l P from acc', R = P q_(l-1),
    round(x) = floor(x + 1/2) = floor((X + (R - 1) / 2) / R); random words and the extreme ones (0 everywhere, q - 1 everywhere);
  * with a real key (Hks.gen_key from a ternary s to s^2) and a product of two encryptions of small messages, out_0 + out_1 s equals
    D(s) / q_(l-1) within 21 n sum_d |G_d| D_d / (P q_(l-1)) + (n_p + 1/2)(n + 1);
  * the three-call route of the model (relinearize, then an exact rounding division by q_(l-1)) differs from the fused output by at
    most n_p + 1 per coefficient: the two are not word-identical and decrypt alike."""
import math

import numpy as np
import pytest

from hks_mul_model import HksMul, negacyclic

L, K, ALPHA = 3, 5, 2
N_P = K - L


def model(orc, n):
    return HksMul(orc, n, L, K, ALPHA, orc.primes(K, 45, n))


def words(orc, hks, family, comps, l, salt):
    rows = []
    for k in range(comps):
        for i in range(l):
            q = hks.qs[i]
            rows.append({"random": lambda: orc.splitmix(hks.n, 401 + salt * 53 + k * 7 + i, q), "zeros": lambda: np.zeros(hks.n, dtype=np.uint64),
                         "tops": lambda: np.full(hks.n, q - 1, dtype=np.uint64)}[family]())
    return np.concatenate(rows)


def key_words(orc, hks, family):
    return np.concatenate([np.full(hks.n, hks.qs[i] - 1, dtype=np.uint64) if family == "tops" else
                           orc.splitmix(hks.n, 9001 + d * 131 + k * 17 + i, hks.qs[i])
                           for d in range(hks.dnum) for k in range(2) for i in range(K)])


def centred_out(hks, out, l):
    """the fused output [2][l - 1][n] -> per component the coefficients CRT-lifted centred over Q_(l-1), and Q_(l-1)"""
    out = np.asarray(out, dtype=np.uint64).reshape(2, l - 1, hks.n)
    lifted = [hks.crt_coeffs(out[k], list(range(l - 1)), centred=True) for k in range(2)]
    return [v for v, _ in lifted], lifted[0][1]


@pytest.mark.parametrize("n", [2, 16])
@pytest.mark.parametrize("l", [2, 3])
@pytest.mark.parametrize("family", ["random", "zeros", "tops"])
def test_one_rounding_with_a_bounded_overshoot(orc, n, l, family):
    hks = model(orc, n)
    keys = key_words(orc, hks, family)
    ct3 = words(orc, hks, family, 3, l, l)
    acc = hks.acc_prime(keys, ct3, l)
    out, Qlow = centred_out(hks, hks.relinearize_rescale(keys, ct3, l), l)
    R = hks.P * hks.qs[l - 1]
    seen = set()
    for k in range(2):
        X, QP = hks.crt_coeffs(acc[k], hks.basis(l))
        assert QP == Qlow * R
        for j in range(n):
            e = ((int(X[j]) + (R - 1) // 2) // R - int(out[k][j])) % Qlow
            assert 0 <= e <= N_P, f"component {k}, coefficient {j}: round(X / R) - out = {e if e <= Qlow // 2 else e - Qlow}"
            seen.add(e)
    print(f"[hks mul model] n = {n}, level {l}, {family}: overshoots seen {sorted(seen)}")


def encrypt(hks, rng, m, s, l):
    """(m + e - a s, a) at level l in NTT form, [2][l][n]; e uniform in [-21, 21], a uniform below Q_l; returns the ciphertext and m + e"""
    n = hks.n
    Q = math.prod(hks.qs[:l])
    a = np.array([int.from_bytes(rng.bytes(32), "little") % Q for _ in range(n)], dtype=object)
    me = np.array([int(v) for v in m], dtype=object) + np.array([int(v) for v in rng.integers(-21, 22, n)], dtype=object)
    c0 = me - negacyclic(a, s)
    return np.stack([np.stack([np.array(hks.ntt_signed(c, i), dtype=np.uint64) for i in range(l)]) for c in (c0, a)]), me


@pytest.mark.parametrize("n", [2, 16])
@pytest.mark.parametrize("l", [2, 3])
def test_a_real_product_decrypts_within_the_noise_bound(orc, n, l):
    hks = model(orc, n)
    rng = np.random.default_rng(29 + n + l)
    s = rng.integers(-1, 2, n)
    keys = hks.gen_key(s, negacyclic(s, s), rng)
    cta, mea = encrypt(hks, rng, rng.integers(-2**28, 2**28, n), s, l)
    ctb, meb = encrypt(hks, rng, rng.integers(-2**28, 2**28, n), s, l)
    out = np.asarray(hks.multiply_sum_rescale(keys, [cta], [ctb], l), dtype=np.uint64).reshape(2, l - 1, n)
    D = negacyclic(mea, meb)                                      # D(s) = (m_a + e_a)(m_b + e_b), far below Q_l / 2: its centred lift
    dec = [(out[0, i].astype(object) + out[1, i].astype(object) * hks.ntt_signed(s, i)) % hks.qs[i] for i in range(l - 1)]
    V, Qlow = hks.crt_coeffs(dec, list(range(l - 1)), centred=True)
    q, Ql = hks.qs[l - 1], Qlow * hks.qs[l - 1]
    B = hks.rescale_noise_bound(l)
    worst = 0
    for j in range(n):
        E = (q * int(V[j]) - int(D[j])) % Ql                      # q (out_0 + out_1 s) - D(s), centred modulo Q_l
        worst = max(worst, min(E, Ql - E))
    print(f"[hks mul model] n = {n}, level {l}: |out_0 + out_1 s - D(s) / q| = {worst / q:.3f}, bound {B:.4g}, |D / q| up to {max(abs(int(v)) for v in D) / q:.4g}")
    assert worst <= q * B, f"level {l}: {worst / q} > {B}"


@pytest.mark.parametrize("n", [2, 16])
@pytest.mark.parametrize("l", [2, 3])
@pytest.mark.parametrize("family", ["random", "tops"])
def test_the_three_call_route_differs_by_at_most_np_plus_one(orc, n, l, family):
    hks = model(orc, n)
    keys = key_words(orc, hks, family)
    ct3 = words(orc, hks, family, 3, l, 7 + l)
    fused, Qlow = centred_out(hks, hks.relinearize_rescale(keys, ct3, l), l)
    rel = np.asarray(hks.relinearize(keys, ct3, l), dtype=np.uint64).reshape(2, l, n)
    q = hks.qs[l - 1]
    worst = 0
    for k in range(2):
        X, _ = hks.crt_coeffs(rel[k], list(range(l)))
        for j in range(n):
            d = ((int(X[j]) + q // 2) // q - int(fused[k][j])) % Qlow
            worst = max(worst, min(d, Qlow - d))
    print(f"[hks mul model] n = {n}, level {l}, {family}: the routes differ by up to {worst}")
    assert worst <= N_P + 1


def test_multiply_sum_relinearize_is_the_composition(orc):
    import tensor_model
    hks = model(orc, 2)
    keys = key_words(orc, hks, "random")
    a, b = words(orc, hks, "random", 2, 3, 1), words(orc, hks, "random", 2, 3, 2)
    ct3 = tensor_model.ct_tensor_sum(hks.qs, 2, [a, a], [b, a], 3)
    assert np.array_equal(hks.multiply_sum_relinearize(keys, [a, a], [b, a], 3), hks.relinearize(keys, ct3, 3))
    assert np.array_equal(hks.multiply_sum_rescale(keys, [a, a], [b, a], 3), hks.relinearize_rescale(keys, ct3, 3))
