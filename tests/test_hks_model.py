"""CPU: the hybrid key switch's host model (tests/hks_model.py) against what it must reduce to and what it must achieve.
  * alpha = 1, K = L + 1: the oracle's key switch (ks_util.KsCase.expected) word for word -- the anchor of the definition;
  * a key built as KeySwitchPlan.gen_hybrid_key defines it, from a ternary s and an arbitrary s': c0' + c1' s - t s' is small at EVERY
    level l = 1 ... L with the ONE key, after a centred CRT lift over the l limbs, within
        B = 21 n sum_d |G_d| D_d / P + (n_p + 1/2)(n + 1)
    (n coefficients of an extended digit below |G_d| D_d times a key error of magnitude <= 21, divided by P; a rounding-plus-overshoot
    error below n_p + 1/2 per component times 1 + ||s||_1) on the shapes tests/test_gpu_hks.py runs."""
import numpy as np
import pytest

from hks_model import Hks
from ks_util import KsCase, seal_chain

N = 1024


def chain_for(orc, shape):
    """(L, alpha, K, moduli) of a named shape"""
    if shape == "L4_a2_K6":
        return 4, 2, 6, orc.primes(6, 45, N)
    if shape == "L5_a2_K7_ragged":
        return 5, 2, 7, orc.primes(7, 40, N)
    if shape == "one_digit":
        return 3, 3, 6, orc.primes(6, 36, N)
    if shape == "per_limb":
        return 3, 1, 4, orc.primes(4, 51, N)
    if shape == "np1_a2":
        return 4, 2, 5, orc.primes(5, 50, N)
    assert shape == "mixed_tier", shape
    return 4, 2, 6, seal_chain(orc, 6, N)                         # 52, 30, 30, 40 | 27, 27 bits


SHAPES = ["L4_a2_K6", "L5_a2_K7_ragged", "one_digit", "per_limb", "np1_a2", "mixed_tier"]


@pytest.mark.parametrize("L", [2, 3])
def test_alpha_one_is_the_oracle_keyswitch(orc, L):
    case = KsCase(orc, N, L, L + 1, seed=3)
    hks = Hks(orc, N, L, L + 1, 1, case.moduli)
    assert hks.dnum == L and hks.P == int(case.moduli[L])
    for b in range(2):
        t, r = case.inputs(orc, b) if b == 0 else case.extreme_inputs(orc, b)
        assert np.array_equal(hks.keyswitch(np.concatenate(case.keys), t, r, L), case.expected(orc, t, r)), f"instance {b}"


@pytest.mark.parametrize("shape", SHAPES)
def test_one_key_switches_every_level_within_the_bound(orc, shape):
    L, alpha, K, moduli = chain_for(orc, shape)
    hks = Hks(orc, N, L, K, alpha, moduli)
    rng = np.random.default_rng(11)
    s = rng.integers(-1, 2, N)
    s_from = rng.integers(-2**30, 2**30, N)
    keys = hks.gen_key(s, s_from, rng)
    for l in range(1, L + 1):
        t = np.stack([orc.splitmix(N, 77 + 13 * l + i, hks.qs[i]) for i in range(l)])
        out = hks.keyswitch(keys, t, np.zeros((2, l, N), dtype=np.uint64), l)
        worst = max(abs(int(v)) for v in hks.noise(out, t, s, s_from, l))
        B = hks.noise_bound(l)
        print(f"[hks model] {shape} level {l}: |noise| = {worst}, bound {B:.4g}")
        assert worst <= B, f"{shape} level {l}: {worst} > {B}"


def test_digits_and_basis():
    class NoTransforms:
        pass
    h = Hks(None, N, 5, 7, 2, [3, 5, 7, 11, 13, 17, 19], lm=NoTransforms())
    assert h.dnum == 3 and h.P == 17 * 19
    assert h.digits(5) == [[0, 1], [2, 3], [4]] and h.digits(3) == [[0, 1], [2]] and h.digits(2) == [[0, 1]]
    assert h.basis(3) == [0, 1, 2, 5, 6]
