"""CPU: the exact model of hexl_linear_transform (tests/lt_model.py), pinned three ways -- (a) with one rotation and an all-ones
plaintext it is hoist_model.rotate_hoisted word for word; (b) with real Galois keys it decrypts to the plaintext-weighted sum of the
rotated messages within the bound one rotation is granted, carried through the products and the sum; (c) its words are NOT those of the
composition rotate_hoisted -> multiply -> add, as the header documents -- and the host replay of the multiply-accumulate's scalar chain
(f64_arith.hpp lt_mac / lt_mac_acc) against 128-bit integers (tests/cpp/lt_mac_selftest.cpp, compiled here)."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from ckks_model import first_mismatch
from hoist_model import GaloisRlwe, limbs_of, mod_up, rotate_hoisted
from ks_util import KsCase, RlweCase, extreme_ciphertext
from lt_model import (check_decrypts, composition, linear_transform, ones_plaintext, sparse_plaintext, uniform_plaintext)
from test_rns_ops_abi import selftest_moduli

ROOT = Path(__file__).resolve().parent.parent

# the decryption case, shared with tests/test_gpu_linear_transform.py: sparse signed plaintexts, sum of ||.||_1 = 60 (< 2^18)
LT_GS = lambda n: [5, 25, 2 * n - 1]
LT_COEFFS = [{0: 3, 7: -2, 500: 5}, {1: -4, 1023: 6}, {0: 1, 64: -7, 65: 8, 900: -9}]
LT_ID_COEFFS = {0: 2, 3: -11, 512: 2}


def ct_of(orc, case, b):
    n, L = case.n, case.L
    return np.concatenate([orc.splitmix(n, case.seed * 31 + b * 977 + k * 17 + i, int(case.moduli[i]))
                           for k in range(2) for i in range(L)])


def rlwe_rotations(orc, rc):
    """three Galois key sets over one RlweCase (one secret); they share the ciphertext and the message, which follow the seed alone"""
    grs = [GaloisRlwe(orc, rc, g) for g in LT_GS(rc.n)]
    assert all(np.array_equal(g.ct, grs[0].ct) and np.array_equal(g.m, grs[0].m) for g in grs)
    return grs


@pytest.mark.parametrize("g", ["1", "3", "2n-1"])
def test_all_ones_plaintext_is_the_hoisted_rotation(orc, g):
    n, L, K = 1024, 2, 3
    g = {"1": 1, "3": 3, "2n-1": 2 * n - 1}[g]
    case = KsCase(orc, n, L, K, seed=83)
    for ct in (ct_of(orc, case, 0), extreme_ciphertext(case, 1, 2)):
        got, want = linear_transform(orc, [case], [g], [ones_plaintext(case)], None, ct), rotate_hoisted(orc, case, ct, g)
        assert np.array_equal(got, want), first_mismatch(got, want, ("component", "limb", "coefficient"), (2, L, n))


@pytest.mark.parametrize("g", ["1", "3"])
def test_all_ones_plaintext_is_the_hoisted_rotation_with_more_key_moduli_than_digits_plus_one(orc, g):
    """K = L + 2: row L of a plaintext is modulo the special prime moduli[K - 1]; hoist_model is pinned to the oracle at this K in
    test_hoist_model.py. A plaintext of ones in every row but row L shows that row L is read"""
    n, L, K = 1024, 2, 4
    g = int(g)
    case = KsCase(orc, n, L, K, seed=83)
    assert int(case.moduli[L]) != int(case.moduli[K - 1])
    for ct in (ct_of(orc, case, 0), extreme_ciphertext(case, 1, 2)):
        got, want = linear_transform(orc, [case], [g], [ones_plaintext(case)], None, ct), rotate_hoisted(orc, case, ct, g)
        assert np.array_equal(got, want), first_mismatch(got, want, ("component", "limb", "coefficient"), (2, L, n))
    twos = ones_plaintext(case)
    twos[L * n:] = 2
    assert not np.array_equal(linear_transform(orc, [case], [g], [twos], None, ct), want), "row L of the plaintext is not read"


@pytest.mark.parametrize("identity", [False, True])
def test_decrypts_to_the_weighted_sum_of_rotations(orc, identity):
    rc = RlweCase(orc, 1024, 2, 3, 50, seed=4)
    grs = rlwe_rotations(orc, rc)
    pts = [sparse_plaintext(rc, c) for c in LT_COEFFS]
    pt_id = sparse_plaintext(rc, LT_ID_COEFFS, rows=rc.L) if identity else None
    out = linear_transform(orc, grs, LT_GS(rc.n), pts, pt_id, grs[0].ct)
    noise, bound = check_decrypts(grs, LT_COEFFS, LT_ID_COEFFS if identity else None, out)
    print(f"largest noise coefficient {noise} (2^{np.log2(max(noise, 1)):.1f}), bound 2^{np.log2(bound):.1f}")
    # the composition decrypts to the same plaintext, with other words
    comp = composition(orc, grs, LT_GS(rc.n), pts, pt_id, grs[0].ct)
    check_decrypts(grs, LT_COEFFS, LT_ID_COEFFS if identity else None, comp)
    assert not np.array_equal(out, comp)


@pytest.mark.parametrize("R", [2, 3])
def test_words_differ_from_the_three_call_composition(orc, R):
    """uniform data: one rounding by q_sp against R"""
    n, L, K = 1024, 2, 3
    gs = [3, 5, 2 * n - 1][:R]
    cases = [KsCase(orc, n, L, K, seed=83 + r) for r in range(R)]
    ct = ct_of(orc, cases[0], 0)
    lm = limbs_of(orc, cases[0])
    u = mod_up(lm, cases[0], ct)
    pts = [uniform_plaintext(orc, cases[0], r) for r in range(R)]
    got, comp = linear_transform(orc, cases, gs, pts, None, ct, lm, u), composition(orc, cases, gs, pts, None, ct, lm, u)
    differ = int((got != comp).sum())
    print(f"R = {R}: {differ} of {got.size} words differ from the composition")
    assert differ > got.size // 2


def test_lt_mac_host_replay(orc, tmp_path):
    exe = tmp_path / "lt_mac_selftest"
    subprocess.run(["g++", "-O2", "-std=c++17", "-mfma", "-ffp-contract=off", "-Wall", "-o", str(exe),
                    str(ROOT / "tests" / "cpp" / "lt_mac_selftest.cpp")], check=True)
    out = subprocess.run([str(exe), "4000"] + [str(q) for q in selftest_moduli(orc)], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:])
    assert out.returncode == 0 and "ALL PASSED" in out.stdout
