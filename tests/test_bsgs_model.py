"""CPU: the exact model of hexl_linear_transform_bsgs (tests/bsgs_model.py) is the composition lt_model.linear_transform ->
hoist_model.rotate_hoisted -> modular sum. Pinned two ways: (a) one giant step with G = 1 is lt_model.linear_transform word for word;
(b) with real Galois keys under one secret a 2 x 2 and a 3 x 2 grid with a NULL entry and identity terms decrypt to
sum_j sigma_{G_j}( sum_i p_{j,i} . sigma_{g_i}(m) + p_id_j . m ) within the bound derived in bsgs_model.check_decrypts_bsgs."""
import numpy as np
import pytest

from bsgs_model import check_decrypts_bsgs, linear_transform_bsgs
from ckks_model import first_mismatch
from hoist_model import GaloisRlwe
from ks_util import KsCase, RlweCase
from lt_model import linear_transform, sparse_plaintext, uniform_plaintext
from test_lt_model import ct_of

# the decryption cases, shared with tests/test_gpu_linear_transform_bsgs.py: sparse signed plaintexts {exponent: coefficient}.
# grid = (baby elements, giant elements, coeffs[j][i] or None, identity coeffs[j] or None); n = 1024
BSGS_GRIDS = {
    "2x2": ([5, 25], [1, 125],
            [[{0: 3, 7: -2}, {1: -4, 1023: 6}], [{64: -7, 65: 8}, {500: 5}]],
            None),
    # three baby steps, two giant steps: a NULL entry, a baby column no row uses, a row of identity only, G = 1 not first, the same
    # element (25) as a baby and as a giant step, identity terms
    "3x2": ([5, 25, 2047], [25, 1],
            [[{0: 1, 900: -9}, None, {3: 2, 511: -4}], [None, None, None]],
            [{0: 2, 3: -11}, {512: 2, 1: 1}]),
}


def bsgs_rlwe(orc, rc, name):
    """Galois key sets over one RlweCase (one secret, one message, one ciphertext): (baby, giant); no giant set where G = 1"""
    baby_gs, giant_gs, _, _ = BSGS_GRIDS[name]
    baby = [GaloisRlwe(orc, rc, g) for g in baby_gs]
    giant = [None if G == 1 else GaloisRlwe(orc, rc, G) for G in giant_gs]
    return baby, giant


def bsgs_plaintexts(rc, name):
    _, _, coeffs, ids = BSGS_GRIDS[name]
    pts = [[None if c is None else sparse_plaintext(rc, c) for c in row] for row in coeffs]
    pt_ids = None if ids is None else [None if c is None else sparse_plaintext(rc, c, rows=rc.L) for c in ids]
    return pts, pt_ids


@pytest.mark.parametrize("identity", [False, True])
def test_one_giant_step_without_rotation_is_the_linear_transform(orc, identity):
    n, L, K = 1024, 2, 3
    gs = [3, 5, 2 * n - 1]
    cases = [KsCase(orc, n, L, K, seed=83 + r) for r in range(3)]
    ct = ct_of(orc, cases[0], 0)
    pts = [uniform_plaintext(orc, cases[0], r) for r in range(3)]
    pt_id = uniform_plaintext(orc, cases[0], 9, rows=L) if identity else None
    got = linear_transform_bsgs(orc, cases, gs, [None], [1], [pts], None if pt_id is None else [pt_id], ct)
    want = linear_transform(orc, cases, gs, pts, pt_id, ct)
    assert np.array_equal(got, want), first_mismatch(got, want, ("component", "limb", "coefficient"), (2, L, n))


@pytest.mark.parametrize("name", sorted(BSGS_GRIDS))
def test_decrypts_to_the_baby_step_giant_step_sum(orc, name):
    rc = RlweCase(orc, 1024, 2, 3, 50, seed=4)
    baby, giant = bsgs_rlwe(orc, rc, name)
    baby_gs, giant_gs, coeffs, ids = BSGS_GRIDS[name]
    pts, pt_ids = bsgs_plaintexts(rc, name)
    out = linear_transform_bsgs(orc, baby, baby_gs, giant, giant_gs, pts, pt_ids, baby[0].ct)
    noise, bound = check_decrypts_bsgs(baby, giant, giant_gs, coeffs, ids, out)
    print(f"{name}: largest noise coefficient {noise} (2^{np.log2(max(noise, 1)):.1f}), bound 2^{np.log2(bound):.1f}")
