"""Host model of hexl_hks_rotate_hoisted and hexl_hks_linear_transform (include/hexl_mi355x.h) in Python integers, built
on hks_model.Hks (mod_up, digits, basis, key_word_rows) and ckks_model.apply_galois:

    ext[d][jT]   = Hks.mod_up(c1, l): steps 1-2 of the hybrid key switch on component 1, ONCE per ciphertext; jT indexes basis(l)
    hoisted      acc_r[k][j] = sum_d sigma_{g_r}(ext_d[j]) key_r[d][k][j];   out_r = (sigma_{g_r}(c0), 0) + down(acc_r)
    transform    acc[k][j]   = sum_r pt_r[j] (sum_d sigma_{g_r}(ext_d[j]) key_r[d][k][j])
                 out[0][i]   = sum_r pt_r[i] sigma_{g_r}(c0[i]) + pt_id[i] c0[i] + down(acc[0])[i]
                 out[1][i]   =                                   pt_id[i] c1[i] + down(acc[1])[i]
    down(acc)[i] = (acc[i] - NTT_i((w_i + fix_i) mod q_i)) P^-1, step 4 of the key switch (mod_down below)

pt_r is [K][n], the plaintext modulo every plan limb; pt_id [>= l][n]. For g = 1 the hoisted rotation is Hks.rotate word for word; for
g != 1 it is not: the digits are lifted and then permuted, Hks.rotate permutes and then lifts.

Noise of the linear transform (lt_noise_bound), derived as Hks.noise_bound is. With key_r[d] = (P [j in G_d] s(X^g_r) + e_rd - a_rd s, a_rd)
and x_d the lift of digit d in [0, |G_d| D_d) whose transform ext_d is,
    acc[0] + acc[1] s = P sum_r pt_r sigma_r(c1) sigma_r(s) + sum_r pt_r sum_d sigma_r(x_d) e_rd
over the integers modulo Q_l P, as long as every pt_r is ONE small integer polynomial reduced modulo every limb of T_l. A product of
polynomials modulo X^n + 1 has infinity norm at most ||a||_1 ||b||_inf, so the second sum is at most
sum_r ||pt_r||_1 . n . sum_d |G_d| D_d . 21 in magnitude; the mod-down divides it by P and adds its rounding-plus-overshoot error, below
n_p + 1/2 per component, times 1 + ||s||_1 <= n + 1 -- ONCE, because there is one mod-down. The identity term pt_id (c0 + c1 s) and the
terms pt_r sigma_r(c0) are exact. Hence
    B_lt = (sum_r ||pt_r||_1) 21 n sum_d |G_d| D_d / P + (n_p + 1/2)(n + 1)."""
import math

import numpy as np

from ckks_model import apply_galois, automorphism_coeff


def mod_down(hks, acc, base, l):
    """step 4: acc[2][T_l] (object rows below their moduli) added into base[2][l][n] -> uint64 [2][l][n]"""
    lm, qs, n, L, K, P = hks.lm, hks.qs, hks.n, hks.L, hks.K, hks.P
    half = P // 2
    out = np.empty((2, l, n), dtype=np.uint64)
    for k in range(2):
        z = {}
        for si, s in enumerate(range(L, K)):
            b = (lm.intt(np.array(acc[k][l + si], dtype=np.uint64), s).astype(object) + half % qs[s]) % qs[s]
            z[s] = (b * pow(P // qs[s], -1, qs[s])) % qs[s]
        for i in range(l):
            qi = qs[i]
            w = sum(z[s] * ((P // qs[s]) % qi) for s in range(L, K)) % qi
            wn = lm.ntt(np.array((w + qi - half % qi) % qi, dtype=np.uint64), i).astype(object)
            out[k, i] = np.array((base[k][i] + (acc[k][i] - wn) * pow(P, -1, qi)) % qi, dtype=np.uint64)
    return out


def inner(hks, keys, ext, l, g):
    """[k][jT] = sum_d sigma_g(ext_d[jT]) key[d][k][j] mod q_j, object rows"""
    kw = hks.key_word_rows(keys)
    n = hks.n
    rows = [[apply_galois(ext[d][jT], n, g).astype(object) for jT in range(len(ext[d]))] for d in range(len(ext))]
    return [[sum(rows[d][jT] * kw[d, k, j].astype(object) for d in range(len(ext))) % hks.qs[j] for jT, j in enumerate(hks.basis(l))]
            for k in range(2)]


def rotate_hoisted(hks, keys, ct, l, g, ext=None):
    """ct[2][l][n] -> flat uint64 [2][l][n], the words hexl_hks_rotate_hoisted writes for Galois element g and `keys`; ext = the shared
    hks.mod_up(c1, l)"""
    n = hks.n
    c = np.asarray(ct, dtype=np.uint64).reshape(2, l, n)
    ext = ext or hks.mod_up(c[1], l)
    base = [[apply_galois(c[0, i], n, g).astype(object) for i in range(l)], [0] * l]
    return mod_down(hks, inner(hks, keys, ext, l, g), base, l).reshape(-1)


def linear_transform(hks, keys_list, gs, pts, pt_id, ct, l, ext=None):
    """ct[2][l][n] -> flat uint64 [2][l][n], the words hexl_hks_linear_transform writes; pts[r]: [K][n], pt_id: [>= l][n] or None"""
    n, K = hks.n, hks.K
    c = np.asarray(ct, dtype=np.uint64).reshape(2, l, n)
    ext = ext or hks.mod_up(c[1], l)
    basis = hks.basis(l)
    pts = [np.asarray(p, dtype=np.uint64).reshape(K, n).astype(object) for p in pts]
    pid = None if pt_id is None else np.asarray(pt_id, dtype=np.uint64).reshape(-1, n)[:l].astype(object)
    acc = [[np.zeros(n, dtype=object) for _ in basis] for _ in range(2)]
    base = [[np.zeros(n, dtype=object) for _ in range(l)] for _ in range(2)]
    for keys, g, pt in zip(keys_list, gs, pts):
        part = inner(hks, keys, ext, l, g)
        for k in range(2):
            for jT, j in enumerate(basis):
                acc[k][jT] = (acc[k][jT] + pt[j] * part[k][jT]) % hks.qs[j]
        for i in range(l):
            base[0][i] = base[0][i] + pt[i] * apply_galois(c[0, i], n, g).astype(object)
    if pid is not None:
        for k in range(2):
            for i in range(l):
                base[k][i] = base[k][i] + pid[i] * c[k, i].astype(object)
    return mod_down(hks, acc, base, l).reshape(-1)


# ---- real keys and the noise of a transform ----
def sigma_signed(poly, n, g):
    """coefficient domain, signed integers: poly(X) -> poly(X^g) mod X^n + 1"""
    big = 1 << 62
    img = automorphism_coeff(np.array([int(v) % big for v in poly], dtype=np.uint64), n, g, big)
    return np.array([int(v) - big if int(v) >= big >> 1 else int(v) for v in img], dtype=object)


def encode_small(hks, poly):
    """a signed integer polynomial -> [K][n] uint64: NTT form modulo every plan limb, special primes included"""
    return np.stack([np.array(hks.ntt_signed(poly, i), dtype=np.uint64) for i in range(hks.K)])


def ones_plaintext(hks):
    return np.ones((hks.K, hks.n), dtype=np.uint64)


def lt_noise(hks, out, ct, s, gs, pts, pt_id, l):
    """the centred CRT lift over the l limbs of  out0 + out1 s - sum_r pt_r sigma_r(c0 + c1 s) - pt_id (c0 + c1 s),  coefficient by
    coefficient: what a transform with keys from s(X^g_r) to s leaves beside the exact result. A hoisted rotation is the transform with
    one all-ones plaintext."""
    lm, qs, n, K = hks.lm, hks.qs, hks.n, hks.K
    out = np.asarray(out, dtype=np.uint64).reshape(2, l, n).astype(object)
    c = np.asarray(ct, dtype=np.uint64).reshape(2, l, n).astype(object)
    pts = [np.asarray(p, dtype=np.uint64).reshape(K, n).astype(object) for p in pts]
    Q = math.prod(qs[:l])
    acc = np.zeros(n, dtype=object)
    for i in range(l):
        q = qs[i]
        si = hks.ntt_signed(s, i)
        dec = c[0, i] + c[1, i] * si
        v = out[0, i] + out[1, i] * si
        for g, pt in zip(gs, pts):
            v = v - pt[i] * apply_galois(np.array(dec % q, dtype=np.uint64), n, g).astype(object)
        if pt_id is not None:
            v = v - np.asarray(pt_id, dtype=np.uint64).reshape(-1, n)[i].astype(object) * dec
        coeffs = lm.intt(np.array(v % q, dtype=np.uint64), i).astype(object)
        acc = acc + coeffs * ((Q // q) * pow(Q // q, -1, q))
    acc = acc % Q
    return np.array([int(v) - Q if int(v) > Q // 2 else int(v) for v in acc], dtype=object)


def lt_noise_bound(hks, l, pt_norms, err=21):
    """B_lt = (sum_r ||pt_r||_1) err n sum_d |G_d| D_d / P + (n_p + 1/2)(n + 1); pt_norms: the 1-norms of the rotations' plaintexts (the
    identity plaintext adds nothing). One all-ones plaintext (norm 1) gives Hks.noise_bound."""
    n, n_p = hks.n, hks.K - hks.L
    first = sum(len(G) * math.prod(hks.qs[i] for i in G) for G in hks.digits(l))
    return sum(pt_norms) * err * n * first / hks.P + (n_p + 0.5) * (n + 1)
