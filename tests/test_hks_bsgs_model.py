"""CPU: the host model of hexl_hks_linear_transform_bsgs (tests/hks_bsgs_model.py) against what it must reduce to and what it must
achieve, at n = 1024, L = 4, alpha = 2, K = 6 on 45-bit primes, at l = 4 and l = 3 (a ragged last digit):
  * one giant step with G = 1 is hks_hoisted_model.linear_transform word for word;
  * an all-ones baby plaintext and one giant step is two chained hks_hoisted_model.rotate_hoisted calls;
  * alpha = 1, K = L + 1 (L = 2) is the per-limb bsgs_model.linear_transform_bsgs word for word;
  * with keys from Hks.gen_key under one secret a 2 x 2 grid and a 3-baby x 2-giant grid (a NULL entry, an unused column without keys, a
    row of identity only, G = 1 not first, g = 25 as a baby and as a giant step) decrypt to the baby-step/giant-step sum within
    B_bsgs = sum_j B_lt(row j) + #{j : G_j != 1} . B (derivation: hks_bsgs_model.py)."""
import numpy as np
import pytest

import bsgs_model
import lt_model
from hks_bsgs_model import bsgs_noise, bsgs_noise_bound, linear_transform_bsgs
from hks_hoisted_model import encode_small, linear_transform, ones_plaintext, rotate_hoisted, sigma_signed
from hks_model import Hks
from ks_util import KsCase

N, L, ALPHA, K = 1024, 4, 2, 6
LEVELS = [4, 3]

# The two grids of real keys (tests/test_gpu_hks_bsgs.py runs the same two shapes on the device): (baby elements, giant elements,
# which (j, i) hold a plaintext, which rows hold an identity plaintext). "3x2": column 1 is used by no row (its object may be NULL), entry (0, 1) is NULL, row 1 is
# identity only, G = 1 is the SECOND giant step, and 25 is a baby step and a giant step.
GRIDS = {
    "2x2": ([5, 25], [1, 125], [[1, 1], [1, 1]], [0, 0]),
    "3x2": ([25, 5, 2 * N - 1], [25, 1], [[1, 0, 1], [0, 0, 0]], [1, 1]),
}


@pytest.fixture(scope="module")
def hks(orc):
    return Hks(orc, N, L, K, ALPHA, orc.primes(K, 45, N))


def uniform_keys(orc, h, salt):
    return np.concatenate([orc.splitmix(N, 9001 + salt * 7919 + d * 131 + k * 17 + i, h.qs[i])
                           for d in range(h.dnum) for k in range(2) for i in range(h.K)])


def uniform_ct(orc, h, l, salt):
    return np.concatenate([orc.splitmix(N, 5003 + salt * 1009 + k * 17 + i, h.qs[i]) for k in range(2) for i in range(l)])


def uniform_pt(orc, h, salt, rows=None):
    return np.stack([orc.splitmix(N, 7000 + salt * 131 + i, h.qs[i]) for i in range(h.K if rows is None else rows)])


def real_grid(h, name, rng, s):
    """keys, plaintexts and 1-norms of a grid of GRIDS under the secret s: (baby_keys, giant_keys, pts, pt_ids, row_norms)"""
    bgs, ggs, has, ids = GRIDS[name]
    used = [any(row[i] for row in has) for i in range(len(bgs))]
    baby_keys = [h.gen_key(s, sigma_signed(s, h.n, g), rng) if u else None for g, u in zip(bgs, used)]
    giant_keys = [None if G == 1 else h.gen_key(s, sigma_signed(s, h.n, G), rng) for G in ggs]
    pts, norms = [], []
    for row in has:
        polys = [rng.integers(-8, 9, h.n) if x else None for x in row]
        pts.append([None if p is None else encode_small(h, p) for p in polys])
        norms.append([int(np.abs(p).sum()) for p in polys if p is not None])
    pt_ids = [encode_small(h, rng.integers(-8, 9, h.n)) if x else None for x in ids]
    return baby_keys, giant_keys, pts, (pt_ids if any(ids) else None), norms


@pytest.mark.parametrize("l", LEVELS)
def test_one_giant_step_without_rotation_is_the_linear_transform(orc, hks, l):
    gs = [3, 5, 2 * N - 1]
    keys = [uniform_keys(orc, hks, r) for r in range(3)]
    ct = uniform_ct(orc, hks, l, l)
    pts = [uniform_pt(orc, hks, r) for r in range(3)]
    for pt_id in (None, uniform_pt(orc, hks, 9, rows=l)):
        got = linear_transform_bsgs(hks, keys, gs, [None], [1], [pts], None if pt_id is None else [pt_id], ct, l)
        assert np.array_equal(got, linear_transform(hks, keys, gs, pts, pt_id, ct, l)), f"level {l}, identity {pt_id is not None}"


@pytest.mark.parametrize("l", LEVELS)
def test_all_ones_baby_and_one_giant_is_two_chained_hoisted_rotations(orc, hks, l):
    keys = [uniform_keys(orc, hks, 3), uniform_keys(orc, hks, 4)]
    ct = uniform_ct(orc, hks, l, 10 + l)
    g, G = 3, 2 * N - 1
    got = linear_transform_bsgs(hks, keys[:1], [g], keys[1:], [G], [[ones_plaintext(hks)]], None, ct, l)
    assert np.array_equal(got, rotate_hoisted(hks, keys[1], rotate_hoisted(hks, keys[0], ct, l, g), l, G))


def test_alpha_one_is_the_per_limb_model(orc):
    l = 2
    cases = [KsCase(orc, N, l, l + 1, seed=3 + r) for r in range(3)]
    h = Hks(orc, N, l, l + 1, 1, cases[0].moduli)
    keys = [np.concatenate(c.keys) for c in cases]
    ct = uniform_ct(orc, h, l, 7)
    bgs, ggs = [5, 2 * N - 1], [3, 1]
    pts = [[lt_model.uniform_plaintext(orc, cases[0], 0), None], [lt_model.uniform_plaintext(orc, cases[0], 1), lt_model.uniform_plaintext(orc, cases[0], 2)]]
    ids = [lt_model.uniform_plaintext(orc, cases[0], 9, rows=l), None]
    got = linear_transform_bsgs(h, keys[:2], bgs, [keys[2], None], ggs, pts, ids, ct, l)
    want = bsgs_model.linear_transform_bsgs(orc, cases[:2], bgs, [cases[2], None], ggs, pts, ids, ct)
    assert np.array_equal(got, want), "alpha = 1, K = L + 1 must be the per-limb model word for word"


@pytest.mark.parametrize("name", sorted(GRIDS))
def test_real_keys_decrypt_within_the_bound(orc, hks, name):
    rng = np.random.default_rng(31)
    s = rng.integers(-1, 2, N)
    bgs, ggs, _, _ = GRIDS[name]
    baby_keys, giant_keys, pts, pt_ids, norms = real_grid(hks, name, rng, s)
    for l in LEVELS:
        ct = uniform_ct(orc, hks, l, 60 + l)
        out = linear_transform_bsgs(hks, baby_keys, bgs, giant_keys, ggs, pts, pt_ids, ct, l)
        worst = max(abs(int(v)) for v in bsgs_noise(hks, out, ct, s, bgs, ggs, pts, pt_ids, l))
        B = bsgs_noise_bound(hks, l, norms, ggs)
        print(f"[hks bsgs model] {name} level {l}: |noise| = {worst}, bound {B:.4g}")
        assert worst <= B, f"{name} level {l}: {worst} > {B}"
    assert bsgs_noise_bound(hks, L, [[], []], [1, 1]) == 0, "identity-only rows without a rotation are exact"
