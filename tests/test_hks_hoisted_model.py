"""CPU: the host model of the hybrid gadget's hoisted rotations and linear transform (tests/hks_hoisted_model.py) against what it must
reduce to and what it must achieve, at n = 1024, L = 4, alpha = 2, K = 6 on 45-bit primes, at l = 4 and l = 3 (a ragged last digit):
  * hoisted at g = 1 is Hks.rotate(g = 1) word for word; for g != 1 it is not;
  * the linear transform with one all-ones plaintext is the hoisted rotation word for word;
  * alpha = 1, K = L + 1 (L = 2): both are the per-limb models (hoist_model.rotate_hoisted, lt_model.linear_transform) word for word;
  * with keys built as gen_hybrid_key defines them for g in {5, 2n - 1}: the hoisted output decrypts to the rotated message within
    Hks.noise_bound(l), and the transform -- dense plaintexts with |coefficient| <= 8 and an identity term -- within
    B_lt = (sum_r ||pt_r||_1) 21 n sum_d |G_d| D_d / P + (n_p + 1/2)(n + 1) (derivation: hks_hoisted_model.py)."""
import numpy as np
import pytest

import hoist_model
import lt_model
from hks_hoisted_model import (encode_small, linear_transform, lt_noise, lt_noise_bound, ones_plaintext, rotate_hoisted, sigma_signed)
from hks_model import Hks
from ks_util import KsCase

N, L, ALPHA, K = 1024, 4, 2, 6
LEVELS = [4, 3]


@pytest.fixture(scope="module")
def hks(orc):
    return Hks(orc, N, L, K, ALPHA, orc.primes(K, 45, N))


def uniform_keys(orc, h, salt):
    return np.concatenate([orc.splitmix(N, 9001 + salt * 7919 + d * 131 + k * 17 + i, h.qs[i])
                           for d in range(h.dnum) for k in range(2) for i in range(h.K)])


def uniform_ct(orc, h, l, salt):
    return np.concatenate([orc.splitmix(N, 5003 + salt * 1009 + k * 17 + i, h.qs[i]) for k in range(2) for i in range(l)])


@pytest.mark.parametrize("l", LEVELS)
def test_hoisted_at_g1_is_rotate_and_ones_transform_is_hoisted(orc, hks, l):
    keys, ct = uniform_keys(orc, hks, 0), uniform_ct(orc, hks, l, l)
    ext = hks.mod_up(ct.reshape(2, l, N)[1], l)
    assert np.array_equal(rotate_hoisted(hks, keys, ct, l, 1, ext), hks.rotate(keys, ct, l, 1)), "g = 1 must be Hks.rotate word for word"
    for g in (5, 2 * N - 1):
        hoisted = rotate_hoisted(hks, keys, ct, l, g, ext)
        assert not np.array_equal(hoisted, hks.rotate(keys, ct, l, g)), f"g = {g}: lifting before permuting changes words"
        assert np.array_equal(linear_transform(hks, [keys], [g], [ones_plaintext(hks)], None, ct, l, ext), hoisted), \
            f"g = {g}: one all-ones plaintext must give the hoisted words"


def test_alpha_one_is_the_per_limb_models(orc):
    l = 2
    cases = [KsCase(orc, N, l, l + 1, seed=3 + r) for r in range(2)]
    h = Hks(orc, N, l, l + 1, 1, cases[0].moduli)
    ct = uniform_ct(orc, h, l, 7)
    gs = [5, 2 * N - 1]
    keys = [np.concatenate(c.keys) for c in cases]
    for r, g in enumerate(gs):
        assert np.array_equal(rotate_hoisted(h, keys[r], ct, l, g), hoist_model.rotate_hoisted(orc, cases[r], ct, g)), f"hoisted, g = {g}"
    pts = [lt_model.uniform_plaintext(orc, cases[0], r) for r in range(2)]
    pt_id = lt_model.uniform_plaintext(orc, cases[0], 9, rows=l)
    for pid in (None, pt_id):
        assert np.array_equal(linear_transform(h, keys, gs, pts, pid, ct, l), lt_model.linear_transform(orc, cases, gs, pts, pid, ct)), \
            f"linear transform, identity term {pid is not None}"


def test_real_keys_decrypt_within_the_bounds(orc, hks):
    rng = np.random.default_rng(23)
    s = rng.integers(-1, 2, N)
    gs = [5, 2 * N - 1]
    keys = [hks.gen_key(s, sigma_signed(s, N, g), rng) for g in gs]
    polys = [rng.integers(-8, 9, N) for _ in gs]
    pts = [encode_small(hks, p) for p in polys]
    norms = [int(np.abs(p).sum()) for p in polys]
    pt_id = encode_small(hks, rng.integers(-8, 9, N))
    for l in LEVELS:
        ct = uniform_ct(orc, hks, l, 40 + l)
        ext = hks.mod_up(ct.reshape(2, l, N)[1], l)
        for r, g in enumerate(gs):
            out = rotate_hoisted(hks, keys[r], ct, l, g, ext)
            worst = max(abs(int(v)) for v in lt_noise(hks, out, ct, s, [g], [ones_plaintext(hks)], None, l))
            B = hks.noise_bound(l)
            print(f"[hks hoisted model] g = {g} level {l}: |noise| = {worst}, bound {B:.4g}")
            assert worst <= B, f"hoisted g = {g} level {l}: {worst} > {B}"
        assert lt_noise_bound(hks, l, [1]) == hks.noise_bound(l)
        out = linear_transform(hks, keys, gs, pts, pt_id, ct, l, ext)
        worst = max(abs(int(v)) for v in lt_noise(hks, out, ct, s, gs, pts, pt_id, l))
        B = lt_noise_bound(hks, l, norms)
        print(f"[hks hoisted model] linear transform level {l}: |noise| = {worst}, bound {B:.4g}")
        assert worst <= B, f"linear transform level {l}: {worst} > {B}"
