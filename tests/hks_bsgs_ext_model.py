"""Host model of hexl_hks_linear_transform_bsgs_ext (include/hexl_mi355x.h) in exact integers: the header's definition
line by line, on the pieces the earlier models pin -- Hks.mod_up and Hks.basis (hks_model), inner and mod_down (hks_hoisted_model), the
rescaling division of HksMul.relinearize_rescale and HksMul.crt_coeffs (hks_mul_model), bsgs_noise (hks_bsgs_model).

    1  ext = mod_up(c1)
    2  inner_j[k][r] = sum_i pt_{j,i}[r] inner(key_i, ext, g_i)[k][r];  kf_j = the key-free part of row j
    3  G_j = 1:  A += inner_j, F += kf_j
       G_j != 1: u_j = kf_j[1] + down_P(inner_j[1]);  W_j = inner(key_G, mod_up(u_j), G_j)
                 A[0] += sigma_G(inner_j[0]) + W_j[0];  A[1] += W_j[1];  F[0] += sigma_G(kf_j[0])
    4  rescale = 0: out = F + down_P(A);   rescale = 1: X_k = P F_k + A_k divided by R = P q_(l-1)

Noise (bsgs_ext_noise_bound; the proof is DESIGN.md 4.6.14). With E = 21 n sum_d |G_d| D_d and S_j the sum of the 1-norms of row j's
plaintexts, P F + A decrypts modulo Q_l P to P times the exact sum plus at most
    pre = sum_j S_j E + #{G != 1} (E + P (n_p + 1/2) n)
(row j's baby switches; per rotated row the giant switch's own error and the rounding of u_j, at most (n_p + 1/2) P per coefficient,
times s). The one division adds (n_p + 1/2)(n + 1):  B = pre / P + (n_p + 1/2)(n + 1), and with rescale = 1 pre / (P q_(l-1)) + the same,
against the exact sum divided by q_(l-1)."""
import math
from fractions import Fraction

import numpy as np

from ckks_model import apply_galois
from hks_bsgs_model import bsgs_noise
from hks_hoisted_model import inner, mod_down
from hks_mul_model import HksMul


class HksExt(HksMul):
    """HksMul whose step 3' is handed in: relinearize_rescale then runs its steps 4' on the residues of X_k = P F_k + A_k"""
    given = None

    def acc_prime(self, keys, ct3, l):
        return self.given

    def divide_by_R(self, X, l):
        """X[k][jT]: the residues of X_k on T_l (object rows) -> flat uint64 [2][l - 1][n], HksMul.relinearize_rescale's division"""
        self.given = X
        return self.relinearize_rescale(None, None, l)


def as_ext(hks):
    return HksExt(None, hks.n, hks.L, hks.K, hks.alpha, hks.qs, lm=hks.lm)     # the transforms are hks's own: no oracle handle needed


def linear_transform_bsgs_ext(hks, baby_keys, baby_gs, giant_keys, giant_gs, pts, pt_ids, ct, l, rescale, parts=None):
    """ct[2][l][n] -> flat uint64 [2][l - rescale][n], the words hexl_hks_linear_transform_bsgs_ext writes. Arguments as
    hks_bsgs_model.linear_transform_bsgs. parts: a dict that receives u (row -> uint64 [l][n]) and X (the residues of P F + A on T_l,
    [2][T] object rows)"""
    n, K, qs = hks.n, hks.K, hks.qs
    basis = hks.basis(l)
    c = np.asarray(ct, dtype=np.uint64).reshape(2, l, n)
    co = c.astype(object)
    ext = hks.mod_up(c[1], l)
    baby = {}
    A = [[np.zeros(n, dtype=object) for _ in basis] for _ in range(2)]
    F = [[np.zeros(n, dtype=object) for _ in range(l)] for _ in range(2)]
    sig = lambda row, g: apply_galois(np.array(row, dtype=np.uint64), n, g).astype(object)
    for j, G in enumerate(giant_gs):
        inn = [[np.zeros(n, dtype=object) for _ in basis] for _ in range(2)]
        kf = [[np.zeros(n, dtype=object) for _ in range(l)] for _ in range(2)]
        for i, p in enumerate(pts[j]):
            if p is None:
                continue
            if i not in baby:
                baby[i] = inner(hks, baby_keys[i], ext, l, baby_gs[i])
            pt = np.asarray(p, dtype=np.uint64).reshape(K, n).astype(object)
            for k in range(2):
                for jT, r in enumerate(basis):
                    inn[k][jT] = (inn[k][jT] + pt[r] * baby[i][k][jT]) % qs[r]
            for i_ in range(l):
                kf[0][i_] = (kf[0][i_] + pt[i_] * sig(c[0, i_], baby_gs[i])) % qs[i_]
        if pt_ids is not None and pt_ids[j] is not None:
            pid = np.asarray(pt_ids[j], dtype=np.uint64).reshape(-1, n)[:l].astype(object)
            for k in range(2):
                for i_ in range(l):
                    kf[k][i_] = (kf[k][i_] + pid[i_] * co[k, i_]) % qs[i_]
        if G == 1:
            for k in range(2):
                for jT, r in enumerate(basis):
                    A[k][jT] = (A[k][jT] + inn[k][jT]) % qs[r]
                for i_ in range(l):
                    F[k][i_] = (F[k][i_] + kf[k][i_]) % qs[i_]
            continue
        u = mod_down(hks, [inn[1], inn[1]], [kf[1], kf[1]], l)[1]          # step 4 on component 1 only
        if parts is not None:
            parts.setdefault("u", {})[j] = u
        W = inner(hks, giant_keys[j], hks.mod_up(u, l), l, G)
        for jT, r in enumerate(basis):
            A[0][jT] = (A[0][jT] + sig(inn[0][jT], G) + W[0][jT]) % qs[r]
            A[1][jT] = (A[1][jT] + W[1][jT]) % qs[r]
        for i_ in range(l):
            F[0][i_] = (F[0][i_] + sig(kf[0][i_], G)) % qs[i_]
    X = [[(A[k][jT] + ((hks.P % qs[r]) * F[k][jT] if jT < l else 0)) % qs[r] for jT, r in enumerate(basis)] for k in range(2)]
    if parts is not None:
        parts["X"] = X
    if not rescale:
        return mod_down(hks, A, F, l).reshape(-1)
    return as_ext(hks).divide_by_R(X, l)


def lift_rescaled(hks, out, l):
    """out[2][l - 1][n] of a rescale = 1 call -> uint64 [2][l][n] holding q_(l-1) out modulo Q_l: limb i < l - 1 times q_(l-1), limb
    l - 1 zero. bsgs_noise of it is q_(l-1) dec(out) - M, M the exact sum: what the bound times q_(l-1) limits."""
    n, qs = hks.n, hks.qs
    o = np.asarray(out, dtype=np.uint64).reshape(2, l - 1, n).astype(object)
    up = np.zeros((2, l, n), dtype=np.uint64)
    for i in range(l - 1):
        up[:, i] = np.array(o[:, i] * qs[l - 1] % qs[i], dtype=np.uint64)
    return up.reshape(-1)


def bsgs_ext_noise(hks, out, ct, s, baby_gs, giant_gs, pts, pt_ids, l, rescale):
    """rescale = 0: hks_bsgs_model.bsgs_noise. rescale = 1: the centred lift over Q_l of q_(l-1) dec(out) - M (compare with
    q_(l-1) times the bound)"""
    return bsgs_noise(hks, lift_rescaled(hks, out, l) if rescale else out, ct, s, baby_gs, giant_gs, pts, pt_ids, l)


def bsgs_ext_noise_bound(hks, l, row_norms, giant_gs, rescale, err=21):
    """B = (sum_j S_j E + #{G != 1} (E + P (n_p + 1/2) n)) / (P, or P q_(l-1)) + (n_p + 1/2)(n + 1), exact as a Fraction.
    row_norms[j]: the 1-norms of row j's baby plaintexts"""
    n, n_p, P = hks.n, hks.K - hks.L, hks.P
    E = err * n * sum(len(G) * math.prod(hks.qs[i] for i in G) for G in hks.digits(l))
    half = Fraction(2 * n_p + 1, 2)
    rotated = sum(1 for G in giant_gs if G != 1)
    pre = sum(sum(norms) for norms in row_norms) * E + rotated * (E + P * half * n)
    return pre / (P * (hks.qs[l - 1] if rescale else 1)) + half * (n + 1)
