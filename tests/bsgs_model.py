"""Host model of hexl_linear_transform_bsgs in exact integers. It is literally the composition the header fixes the output by:

    t_j = lt_model.linear_transform(row j's non-NULL baby steps, pt_identity = pt_ids[j], ct)
          (a row with only an identity term: t_j = pt_id_j . (c0, c1) mod q_i)
    r_j = t_j                                            if G_j == 1
          hoist_model.rotate_hoisted(giant_cases[j], t_j, G_j)     otherwise
    out = sum_j r_j  mod q_i

so it adds no arithmetic of its own beside the modular sum and the identity-only row."""
import numpy as np

from hoist_model import limbs_of, mod_up, rotate_hoisted
from lt_model import linear_transform, negacyclic_sparse


def reference_case(baby_cases, giant_cases):
    """the first case there is: n, L, K and the moduli are the same for all of them"""
    return next(c for c in list(baby_cases) + list(giant_cases) if c is not None)


def identity_row(case, pt_id, ct):
    """pt_id[L][n] . (c0, c1) mod q_i, flat uint64"""
    n, L = case.n, case.L
    c = np.asarray(ct, dtype=np.uint64).reshape(2, L, n).astype(object)
    p = np.asarray(pt_id, dtype=np.uint64).reshape(L, n).astype(object)
    q = np.array([int(v) for v in case.moduli[:L]], dtype=object).reshape(1, L, 1)
    return np.array(c * p[None] % q, dtype=np.uint64).reshape(-1)


def linear_transform_bsgs(orc, baby_cases, baby_gs, giant_cases, giant_gs, pts, pt_ids, ct, lm=None, u=None):
    """ct[2][L][n] -> out[2][L][n] (flat uint64), the words hexl_linear_transform_bsgs writes. pts[j][i]: None or [L + 1][n];
    pt_ids: None or a list of n_giant entries, each None or [L][n]; giant_cases[j] may be None when giant_gs[j] == 1.
    `lm` and `u` (mod_up of the same ct) may be shared between calls on the same ciphertext."""
    ref = reference_case(baby_cases, giant_cases)
    n, L = ref.n, ref.L
    lm = lm or limbs_of(orc, ref)
    q = np.array([lm.qs[i] for i in range(L)], dtype=object).reshape(1, L, 1)
    total = np.zeros((2, L, n), dtype=object)
    for j, G in enumerate(giant_gs):
        pt_id = None if pt_ids is None else pt_ids[j]
        used = [i for i, p in enumerate(pts[j]) if p is not None]
        if used:
            u = u or mod_up(lm, ref, ct)
            t = linear_transform(orc, [baby_cases[i] for i in used], [baby_gs[i] for i in used], [pts[j][i] for i in used], pt_id, ct, lm, u)
        else:
            assert pt_id is not None, "a giant row with no term at all"
            t = identity_row(ref, pt_id, ct)
        r = t if G == 1 else rotate_hoisted(orc, giant_cases[j], t, G, lm)
        total = total + r.reshape(2, L, n).astype(object)
    return np.array(total % q, dtype=np.uint64).reshape(-1)


def check_decrypts_bsgs(baby_grs, giant_grs, giant_gs, coeffs, id_coeffs, out, noise_bits=24):
    """out[2][L][n] decrypts under s to sum_j sigma_{G_j}( sum_i p_{j,i} . sigma_{g_i}(m) + p_id_j . m ) + noise, the same noise
    polynomial in every limb. baby_grs / giant_grs: hoist_model.GaloisRlwe objects over ONE RlweCase (one secret, one message);
    giant_grs[j] may be None when giant_gs[j] == 1. coeffs[j][i]: {exponent: coefficient} or None; id_coeffs[j] likewise.
    The bound (derived, not fitted):
      * lt_model.check_decrypts grants the inner layer t_j the noise ||p||_1-sum of row j times 2^noise_bits: one hoisted rotation's
        granted noise (GaloisRlwe.check: |sigma_g(e) + e_ks| < 2^noise_bits, e the encryption noise, |e| <= 3) carried through a
        negacyclic product with a plaintext (factor ||p||_1) and the sum;
      * sigma_{G_j} permutes coefficients up to sign: the infinity norm of that noise is unchanged by the giant rotation;
      * the giant rotation's own keyswitch adds e_ks', which depends on the digits of t_j's component 1 (any words below q_d) and
        the key's noise only, not on what t_j encrypts: from the same granted bound, |e_ks'| < 2^noise_bits + 3;
      * G_j == 1 runs no keyswitch and adds nothing.
    Returns (largest noise coefficient, bound)."""
    gr0 = next(g for g in list(baby_grs) + list(giant_grs) if g is not None)
    rc, n, L = gr0.rc, gr0.n, gr0.L
    out = np.asarray(out, dtype=np.uint64).reshape(2, L, n)
    m = np.array([int(v) for v in gr0.m], dtype=object)
    want = np.zeros(n, dtype=object)
    bound, l1_all = 0, 0
    for j, G in enumerate(giant_gs):
        inner = np.zeros(n, dtype=object)
        l1 = 0
        for i, c in enumerate(coeffs[j]):
            if c is not None:
                inner = inner + negacyclic_sparse(c, baby_grs[i].sigma_signed(m), n)
                l1 += sum(abs(v) for v in c.values())
        if id_coeffs is not None and id_coeffs[j] is not None:
            inner = inner + negacyclic_sparse(id_coeffs[j], m, n)
            l1 += sum(abs(v) for v in id_coeffs[j].values())
        want = want + (inner if G == 1 else giant_grs[j].sigma_signed(inner))
        bound += (l1 << noise_bits) + (0 if G == 1 else (1 << noise_bits) + 3)
        l1_all += l1
    assert l1_all << 30 < min(rc.qs[:L]) // 4, "the plaintexts leave no room for the message below q / 4"
    noises = []
    for i in range(L):
        q = rc.qs[i]
        dec = rc.intt((out[0, i].astype(object) + out[1, i].astype(object) * gr0.s_ntt[i]) % q, i)
        centred = np.array([int(v) if v <= q // 2 else int(v) - q for v in dec], dtype=object)
        noise = centred - want
        assert max(abs(int(v)) for v in noise) < bound, f"limb {i}: does not decrypt to the baby-step/giant-step sum"
        noises.append(noise)
    for i in range(1, L):
        assert (noises[i] == noises[0]).all(), "limbs disagree on the noise polynomial"
    return max(abs(int(v)) for v in noises[0]), bound
