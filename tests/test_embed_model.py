"""CPU: the host model of encode / decode (tests/embed_model.py) -- its FFT against the example's formulas evaluated directly, encode
then decode, the encode of an integer polynomial's slots, and the slot order against the Galois permutation the library already
models (ckks_model.apply_galois): g = 5 rotates the slots by one."""
import numpy as np

from ckks_model import Limbs, apply_galois
from embed_model import (LD, as_double_slots, crt_lift, embed, embed_direct, embed_inverse, embed_inverse_direct, from_f64,
                         ints_to_ld, ints_to_words)
from rns_model import chain

EPS = float(np.finfo(LD).eps)


def rand_slots(rng, n, count=None):
    shape = (n // 2,) if count is None else (count, n // 2)
    return rng.uniform(-1, 1, shape) + 1j * rng.uniform(-1, 1, shape)


def test_fft_is_the_formula():
    n = 64
    rng = np.random.default_rng(1)
    m = rng.integers(-1000, 1000, n)
    z = rand_slots(rng, n)
    assert np.abs(embed(m, n) - embed_direct(m, n)).max() < 1e5 * EPS
    assert np.abs(embed_inverse(z, n) - embed_inverse_direct(z, n)).max() < 1e3 * EPS
    # the inverse formula gives a REAL polynomial that takes the slot values at zeta^(5^k) and their conjugates at zeta^(-5^k)
    assert np.abs(embed_direct(embed_inverse_direct(z, n), n) - z).max() < 1e3 * EPS


def test_encode_then_decode_returns_the_slots():
    rng = np.random.default_rng(2)
    for n in (1024, 4096):
        z = rand_slots(rng, n, 2)
        back = embed(embed_inverse(z, n), n)
        assert np.abs(back - z).max() < n * 64 * EPS


def test_encode_of_an_integer_polynomials_slots_is_the_polynomial():
    rng = np.random.default_rng(3)
    for n in (1024, 8192):
        m = rng.integers(-(1 << 20), (1 << 20) + 1, n)
        x = embed_inverse(embed(m, n), n)
        assert np.abs(x - m.astype(LD)).max() < 2.0 ** -20
        # through slots rounded to double, the scaled coefficients still round to 2^10 m
        z = as_double_slots(embed(m, n))
        x = embed_inverse(z[..., 0].astype(LD) + 1j * z[..., 1].astype(LD), n) * LD(1024)
        assert np.abs(x - 1024 * m.astype(LD)).max() < 2.0 ** -6


def test_galois_five_rotates_the_slots_by_one(orc):
    n, K = 1024, 2
    qs = chain(orc, "gen", K, n)
    lm = Limbs(orc, n, qs)
    rng = np.random.default_rng(4)
    z = rand_slots(rng, n)
    scale = 2.0 ** 40
    r = np.array([int(v) for v in np.rint(embed_inverse(z, n) * LD(scale))], dtype=object)
    words = ints_to_words(lm, r, K)
    assert np.array_equal(words, from_f64(lm, np.array([float(v) for v in r]), K))
    rot = np.stack([apply_galois(words[i], n, 5) for i in range(K)])
    back = embed(ints_to_ld(crt_lift(lm, rot, K)), n) / LD(scale)
    assert np.abs(back - np.roll(z, -1)).max() < (n / 2 + 1) / scale
    # and the lift of the unrotated words is the polynomial
    assert list(crt_lift(lm, words, K)) == list(r)
