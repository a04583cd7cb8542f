"""Host model of hexl_hks_linear_transform_bsgs (include/hexl_mi355x.h) in exact integers. It is literally the composition
the header fixes the output by, on the models of the two parent calls (tests/hks_hoisted_model.py):

    t_j = hks_hoisted_model.linear_transform(row j's non-NULL baby steps in the order of i, pt_identity = pt_ids[j], ct, l)
          (a row with only an identity term: t_j = pt_id_j . (c0, c1) mod q_i)
    r_j = t_j                                                        if G_j == 1
          hks_hoisted_model.rotate_hoisted(giant_keys[j], t_j, l, G_j)    otherwise
    out = sum_j r_j  mod q_i

so it adds no arithmetic of its own beside the modular sum and the identity-only row.

Noise (bsgs_noise_bound). Row j's inner result t_j decrypts to its exact value plus a noise of infinity norm at most B_lt(row j)
(hks_hoisted_model.lt_noise_bound over the 1-norms of row j's plaintexts; an identity-only row is exact: no key, no mod-down). sigma_G maps
X^k to +-X^(kG mod n): a signed permutation of the coefficients, so the infinity norm of that noise is unchanged by the giant rotation. The
giant rotation's own key switch adds a noise that depends on the digits of t_j's component 1 and the key's errors only, at most
B = Hks.noise_bound(l); G_j = 1 runs no key switch and adds nothing. Hence
    B_bsgs = sum_j B_lt(row j) + #{j : G_j != 1} . B."""
import math

import numpy as np

from ckks_model import apply_galois
from hks_hoisted_model import linear_transform, lt_noise_bound, rotate_hoisted


def identity_row(hks, pt_id, ct, l):
    """pt_id[>= l][n] . (c0, c1) mod q_i, flat uint64 [2][l][n]"""
    n = hks.n
    c = np.asarray(ct, dtype=np.uint64).reshape(2, l, n).astype(object)
    p = np.asarray(pt_id, dtype=np.uint64).reshape(-1, n)[:l].astype(object)
    q = np.array([hks.qs[i] for i in range(l)], dtype=object).reshape(1, l, 1)
    return np.array(c * p[None] % q, dtype=np.uint64).reshape(-1)


def linear_transform_bsgs(hks, baby_keys, baby_gs, giant_keys, giant_gs, pts, pt_ids, ct, l, ext=None):
    """ct[2][l][n] -> flat uint64 [2][l][n], the words hexl_hks_linear_transform_bsgs writes. baby_keys[i] / giant_keys[j]: key words
    [dnum][2][K][n] (None where the object may be NULL); pts[j][i]: None or [K][n]; pt_ids: None or n_giant entries, each None or
    [>= l][n]; ext: hks.mod_up of ct's component 1, shared between calls on one ciphertext"""
    n = hks.n
    q = np.array([hks.qs[i] for i in range(l)], dtype=object).reshape(1, l, 1)
    total = np.zeros((2, l, n), dtype=object)
    for j, G in enumerate(giant_gs):
        pt_id = None if pt_ids is None else pt_ids[j]
        used = [i for i, p in enumerate(pts[j]) if p is not None]
        if used:
            ext = ext or hks.mod_up(np.asarray(ct, dtype=np.uint64).reshape(2, l, n)[1], l)
            t = linear_transform(hks, [baby_keys[i] for i in used], [baby_gs[i] for i in used], [pts[j][i] for i in used], pt_id, ct, l, ext)
        else:
            assert pt_id is not None, "a giant row with no term at all"
            t = identity_row(hks, pt_id, ct, l)
        r = t if G == 1 else rotate_hoisted(hks, giant_keys[j], t, l, G)
        total = total + r.reshape(2, l, n).astype(object)
    return np.array(total % q, dtype=np.uint64).reshape(-1)


def bsgs_noise(hks, out, ct, s, baby_gs, giant_gs, pts, pt_ids, l):
    """the centred CRT lift over the l limbs of
        out0 + out1 s - sum_j sigma_{G_j}( sum_i pt_{j,i} sigma_{g_i}(c0 + c1 s) + pt_id_j (c0 + c1 s) ),
    coefficient by coefficient: what the call leaves beside the exact baby-step/giant-step sum under keys from s(X^g) to s"""
    lm, qs, n, K = hks.lm, hks.qs, hks.n, hks.K
    out = np.asarray(out, dtype=np.uint64).reshape(2, l, n).astype(object)
    c = np.asarray(ct, dtype=np.uint64).reshape(2, l, n).astype(object)
    Q = math.prod(qs[:l])
    acc = np.zeros(n, dtype=object)
    for i in range(l):
        q = qs[i]
        si = hks.ntt_signed(s, i)
        dec = (c[0, i] + c[1, i] * si) % q
        v = out[0, i] + out[1, i] * si
        for j, G in enumerate(giant_gs):
            inner = np.zeros(n, dtype=object)
            for b, pt in enumerate(pts[j]):
                if pt is not None:
                    w = np.asarray(pt, dtype=np.uint64).reshape(K, n)[i].astype(object)
                    inner = inner + w * apply_galois(np.array(dec, dtype=np.uint64), n, baby_gs[b]).astype(object)
            if pt_ids is not None and pt_ids[j] is not None:
                inner = inner + np.asarray(pt_ids[j], dtype=np.uint64).reshape(-1, n)[i].astype(object) * dec
            v = v - apply_galois(np.array(inner % q, dtype=np.uint64), n, G).astype(object)
        coeffs = lm.intt(np.array(v % q, dtype=np.uint64), i).astype(object)
        acc = acc + coeffs * ((Q // q) * pow(Q // q, -1, q))
    acc = acc % Q
    return np.array([int(v) - Q if int(v) > Q // 2 else int(v) for v in acc], dtype=object)


def bsgs_noise_bound(hks, l, row_norms, giant_gs, err=21):
    """B_bsgs = sum_j B_lt(row j) + #{j : G_j != 1} . B; row_norms[j]: the 1-norms of row j's baby plaintexts, empty for a row of
    identity only (which is exact). The identity plaintexts add nothing."""
    rows = sum(lt_noise_bound(hks, l, norms, err) for norms in row_norms if len(norms))
    return rows + sum(1 for G in giant_gs if G != 1) * hks.noise_bound(l, err)
