"""CPU: the host model of hexl_hks_linear_transform_bsgs_ext (tests/hks_bsgs_ext_model.py) against what the header says it reduces to and
what it must achieve, at n = 16 and n = 1024, L = 4, alpha = 2, K = 6 on 45-bit primes, at l = 4 and l = 3 (T_l not a prefix):
  * n_giant = 1, G = 1, rescale = 0 is hks_hoisted_model.linear_transform on row 0 word for word; a grid whose giant elements are all 1
    is the flat linear_transform over the concatenated non-NULL terms;
  * u_j is component 1 of linear_transform(row j);
  * rescale = 1: out_k = round(X_k / R) - e with e in {0 .. n_p} on every coefficient, X_k rebuilt by CRT over Q_l P, on random words and
    on 0 / q - 1 everywhere;
  * with keys from Hks.gen_key under one secret the two grids of test_hks_bsgs_model decrypt within the bound DESIGN.md 4.6.14 proves, for
    both rescale values, and the difference from hks_bsgs_model.linear_transform_bsgs decrypts to less than the sum of the two bounds."""
import numpy as np
import pytest

from hks_bsgs_ext_model import as_ext, bsgs_ext_noise, bsgs_ext_noise_bound, linear_transform_bsgs_ext
from hks_bsgs_model import bsgs_noise_bound, linear_transform_bsgs
from hks_hoisted_model import linear_transform, mod_down
from hks_model import Hks
from test_hks_bsgs_model import GRIDS, real_grid

L, ALPHA, K = 4, 2, 6
LEVELS = [4, 3]
SIZES = [16, 1024]


@pytest.fixture(scope="module", params=SIZES)
def hks(orc, request):
    n = request.param
    return Hks(orc, n, L, K, ALPHA, orc.primes(K, 45, n))


def words(orc, h, rows, salt, family="uniform"):
    """rows: plan limbs, one row of n words each"""
    if family == "zero":
        return np.zeros((len(rows), h.n), dtype=np.uint64)
    if family == "top":
        return np.stack([np.full(h.n, h.qs[i] - 1, dtype=np.uint64) for i in rows])
    return np.stack([orc.splitmix(h.n, 4000 + salt * 977 + r * 31 + i, h.qs[i]) for r, i in enumerate(rows)])


def keys_of(orc, h, salt, family="uniform"):
    return words(orc, h, [i for _ in range(h.dnum) for _ in range(2) for i in range(h.K)], 100 + salt, family).reshape(-1)


def ct_of(orc, h, l, salt, family="uniform"):
    return words(orc, h, [i for _ in range(2) for i in range(l)], 200 + salt, family).reshape(-1)


def pt_of(orc, h, salt, rows=None, family="uniform"):
    return words(orc, h, list(range(h.K if rows is None else rows)), 300 + salt, family)


@pytest.mark.parametrize("l", LEVELS)
def test_one_row_without_rotation_is_the_linear_transform(orc, hks, l):
    n = hks.n
    gs = [3, 5, 2 * n - 1]
    keys = [keys_of(orc, hks, r) for r in range(3)]
    ct = ct_of(orc, hks, l, l)
    pts = [pt_of(orc, hks, r) for r in range(3)]
    for pt_id in (None, pt_of(orc, hks, 9, rows=l)):
        got = linear_transform_bsgs_ext(hks, keys, gs, [None], [1], [pts], None if pt_id is None else [pt_id], ct, l, 0)
        assert np.array_equal(got, linear_transform(hks, keys, gs, pts, pt_id, ct, l)), f"level {l}, identity {pt_id is not None}"


@pytest.mark.parametrize("l", LEVELS)
def test_all_giant_elements_one_is_the_flat_linear_transform(orc, hks, l):
    """three rows, G = 1 each, a NULL entry, the identity term on the middle row: the flat call over the concatenated terms, objects and
    elements repeated per row"""
    n = hks.n
    gs = [3, 2 * n - 1]
    keys = [keys_of(orc, hks, 5 + r) for r in range(2)]
    ct = ct_of(orc, hks, l, 20 + l)
    grid = [[pt_of(orc, hks, 10), pt_of(orc, hks, 11)], [None, pt_of(orc, hks, 12)], [pt_of(orc, hks, 13), None]]
    pid = pt_of(orc, hks, 14, rows=l)
    got = linear_transform_bsgs_ext(hks, keys, gs, [None] * 3, [1, 1, 1], grid, [None, pid, None], ct, l, 0)
    flat = [(keys[i], gs[i], row[i]) for row in grid for i in range(2) if row[i] is not None]
    want = linear_transform(hks, [f[0] for f in flat], [f[1] for f in flat], [f[2] for f in flat], pid, ct, l)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("l", LEVELS)
def test_u_is_component_one_of_the_rows_linear_transform(orc, hks, l):
    n = hks.n
    bgs, ggs = [5, 3], [2 * n - 1, 1, 3]
    bkeys = [keys_of(orc, hks, 20 + r) for r in range(2)]
    gkeys = [keys_of(orc, hks, 30), None, keys_of(orc, hks, 31)]
    ct = ct_of(orc, hks, l, 40 + l)
    grid = [[pt_of(orc, hks, 20), pt_of(orc, hks, 21)], [pt_of(orc, hks, 22), None], [None, None]]
    ids = [pt_of(orc, hks, 23, rows=l), None, pt_of(orc, hks, 24, rows=l)]
    parts = {}
    linear_transform_bsgs_ext(hks, bkeys, bgs, gkeys, ggs, grid, ids, ct, l, 0, parts)
    assert sorted(parts["u"]) == [0, 2]
    row0 = linear_transform(hks, bkeys, bgs, grid[0], ids[0], ct, l).reshape(2, l, n)
    assert np.array_equal(parts["u"][0], row0[1])
    # the identity-only row that rotates: u = pt_id c1 + down_P(0), the mod-down's overshoot on a zero accumulator included
    zero = [[np.zeros(n, dtype=object)] * (l + K - L)] * 2
    c1 = ct.reshape(2, l, n)[1].astype(object)
    base = [(ids[2][i].astype(object) * c1[i]) % hks.qs[i] for i in range(l)]
    assert np.array_equal(parts["u"][2], mod_down(hks, zero, [base, base], l)[1])


@pytest.mark.parametrize("family", ["uniform", "zero", "top"])
@pytest.mark.parametrize("l", LEVELS)
def test_the_rescaled_output_is_the_rounded_quotient_less_a_small_overshoot(orc, hks, l, family):
    n, n_p = hks.n, K - L
    bgs, ggs = [5, 3], [2 * n - 1, 1]
    bkeys = [keys_of(orc, hks, 50 + r, family) for r in range(2)]
    gkeys = [keys_of(orc, hks, 60, family), None]
    ct = ct_of(orc, hks, l, 70 + l, family)
    grid = [[pt_of(orc, hks, 50, family=family), None], [pt_of(orc, hks, 51, family=family), pt_of(orc, hks, 52, family=family)]]
    ids = [pt_of(orc, hks, 53, rows=l, family=family), None]
    parts = {}
    out = linear_transform_bsgs_ext(hks, bkeys, bgs, gkeys, ggs, grid, ids, ct, l, 1, parts).reshape(2, l - 1, n)
    m = as_ext(hks)
    R = hks.P * hks.qs[l - 1]
    worst = 0
    for k in range(2):
        X, QP = m.crt_coeffs(parts["X"][k], hks.basis(l))
        got, Q1 = m.crt_coeffs(out[k], list(range(l - 1)))
        assert QP == Q1 * R
        for x, o in zip(X, got):
            e = ((int(x) + R // 2) // R - int(o)) % Q1                # round(X / R) = floor((X + (R - 1) / 2) / R), R odd
            assert 0 <= e <= n_p, f"component {k}: overshoot {e}"
            worst = max(worst, e)
    print(f"[hks bsgs ext model] n = {n} level {l} {family}: largest overshoot {worst} of at most {n_p}")


@pytest.mark.parametrize("name", sorted(GRIDS))
def test_real_keys_decrypt_within_the_bound(orc, name):
    n = 1024
    h = Hks(orc, n, L, K, ALPHA, orc.primes(K, 45, n))
    rng = np.random.default_rng(31)
    s = rng.integers(-1, 2, n)
    bgs, ggs, _, _ = GRIDS[name]
    baby_keys, giant_keys, pts, pt_ids, norms = real_grid(h, name, rng, s)
    for l in LEVELS:
        ct = ct_of(orc, h, l, 80 + l)
        outs = {}
        for rescale in (0, 1):
            out = outs[rescale] = linear_transform_bsgs_ext(h, baby_keys, bgs, giant_keys, ggs, pts, pt_ids, ct, l, rescale)
            worst = max(abs(int(v)) for v in bsgs_ext_noise(h, out, ct, s, bgs, ggs, pts, pt_ids, l, rescale))
            B = bsgs_ext_noise_bound(h, l, norms, ggs, rescale) * (h.qs[l - 1] if rescale else 1)
            print(f"[hks bsgs ext model] {name} level {l} rescale {rescale}: |noise| = {worst}, bound {float(B):.4g}")
            assert worst <= B, f"{name} level {l} rescale {rescale}: {worst} > {float(B)}"
        # against the composition of hexl_hks_linear_transform_bsgs: other words, the same plaintext up to both bounds
        old = linear_transform_bsgs(h, baby_keys, bgs, giant_keys, ggs, pts, pt_ids, ct, l)
        q = np.array(h.qs[:l], dtype=object).reshape(1, l, 1)
        diff = np.array((outs[0].reshape(2, l, n).astype(object) - old.reshape(2, l, n).astype(object)) % q, dtype=np.uint64)
        gap = max(abs(int(v)) for v in h.noise(diff, np.zeros((l, n), dtype=np.uint64), s, s, l))
        both = bsgs_ext_noise_bound(h, l, norms, ggs, 0) + bsgs_noise_bound(h, l, norms, ggs)
        print(f"[hks bsgs ext model] {name} level {l}: |ext - bsgs| decrypts to {gap}, the two bounds sum to {float(both):.4g}")
        assert gap < both
        if any(G != 1 for G in ggs):
            assert not np.array_equal(outs[0], old), "with a rotated giant step the two calls differ in words"
