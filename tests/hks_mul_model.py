"""Host model of the hybrid multiply (include/hexl_mi355x.h hexl_hks_multiply_sum_relinearize, hexl_hks_relinearize_rescale,
hexl_hks_multiply_sum_rescale) in Python integers, on hks_model.Hks and its transforms.

    1-3  steps 1-3 of the key switch on t = d2 at level l: acc[k][j], j in T_l = {0 .. l-1} + S
    3'   acc'[k][i] = acc[k][i] + (P mod q_i) d_k[i] for i < l; acc'[k][s] = acc[k][s] for s in S
    4'   R = P q_(l-1), h = (R - 1) / 2, B = S + {l - 1}:
         b_s = INTT_s(acc'[k][s]) + h mod q_s;  z_s = b_s (R/q_s)^-1 mod q_s;  w_i = sum_{s in B} z_s (R/q_s mod q_i)
         out[k][i] = (acc'[k][i] - NTT_i(w_i + fix_i)) R^-1 mod q_i,  fix_i = q_i - h mod q_i,  i < l - 1"""
import math

import numpy as np

import tensor_model
from hks_model import Hks


class HksMul(Hks):
    def accumulate(self, keys, t, l):
        """steps 1-3: acc[k][jT] (object rows, NTT form, canonical) for t[l][n]; jT indexes basis(l)"""
        kw = self.key_word_rows(keys)
        ext = self.mod_up(t, l)
        acc = []
        for k in range(2):
            rows = []
            for jT, j in enumerate(self.basis(l)):
                s = np.zeros(self.n, dtype=object)
                for d in range(len(ext)):
                    s = s + ext[d][jT].astype(object) * kw[d, k, j].astype(object)
                rows.append(s % self.qs[j])
            acc.append(rows)
        return acc

    def acc_prime(self, keys, ct3, l):
        """step 3': acc'[k][jT], the residue vector of X_k = P d_k + KSacc_k modulo Q_l P"""
        c = np.asarray(ct3, dtype=np.uint64).reshape(3, l, self.n)
        acc = self.accumulate(keys, c[2], l)
        for k in range(2):
            for i in range(l):
                acc[k][i] = (acc[k][i] + (self.P % self.qs[i]) * c[k, i].astype(object)) % self.qs[i]
        return acc

    def rescale_sources(self, l):
        """B as (plan limb, row of T_l) pairs: the special primes, then the data limb l - 1"""
        return [(s, l + si) for si, s in enumerate(range(self.L, self.K))] + [(l - 1, l - 1)]

    def relinearize_rescale(self, keys, ct3, l):
        """ct3[3][l][n] -> flat uint64 [2][l - 1][n], the words hexl_hks_relinearize_rescale writes"""
        assert 2 <= l <= self.L
        lm, qs, n = self.lm, self.qs, self.n
        acc = self.acc_prime(keys, ct3, l)
        R = self.P * qs[l - 1]
        h = (R - 1) // 2
        out = np.empty((2, l - 1, n), dtype=np.uint64)
        for k in range(2):
            z = {}
            for s, jT in self.rescale_sources(l):
                b = (lm.intt(np.array(acc[k][jT], dtype=np.uint64), s).astype(object) + h % qs[s]) % qs[s]
                z[s] = (b * pow(R // qs[s], -1, qs[s])) % qs[s]
            for i in range(l - 1):
                qi = qs[i]
                w = sum(z[s] * ((R // qs[s]) % qi) for s in z) % qi
                fix = qi - h % qi
                wn = lm.ntt(np.array((w + fix) % qi, dtype=np.uint64), i).astype(object)
                out[k, i] = np.array((acc[k][i] - wn) * pow(R, -1, qi) % qi, dtype=np.uint64)
        return out.reshape(-1)

    def multiply_sum_relinearize(self, keys, a_s, b_s, l, in_limbs=None):
        """the normative composition: ct_tensor_sum at level l, then relinearize"""
        return self.relinearize(keys, tensor_model.ct_tensor_sum(self.qs, self.n, a_s, b_s, l, in_limbs), l)

    def multiply_sum_rescale(self, keys, a_s, b_s, l, in_limbs=None):
        """the normative composition: ct_tensor_sum at level l, then relinearize_rescale"""
        return self.relinearize_rescale(keys, tensor_model.ct_tensor_sum(self.qs, self.n, a_s, b_s, l, in_limbs), l)

    # ---- what the tests measure the definition against ----
    def crt_coeffs(self, rows, limbs, centred=False):
        """the CRT value of every coefficient of NTT-form rows (one per limb of `limbs`) over the product of those moduli"""
        qs = [self.qs[j] for j in limbs]
        Q = math.prod(qs)
        X = np.zeros(self.n, dtype=object)
        for row, j, q in zip(rows, limbs, qs):
            c = self.lm.intt(np.array(row, dtype=np.uint64), j).astype(object)
            X = (X + c * ((Q // q) * pow(Q // q, -1, q))) % Q
        if centred:
            X = np.array([int(v) - Q if int(v) > Q // 2 else int(v) for v in X], dtype=object)
        return X, Q

    def rescale_noise_bound(self, l, err=21):
        """21 n sum_d |G_d| D_d / (P q_(l-1)) + (n_p + 1/2)(n + 1): the key switch's first term divided by q_(l-1) as well, and one rounding
        plus at most n_p multiples of overshoot per component times 1 + ||s||_1"""
        n, n_p = self.n, self.K - self.L
        first = sum(len(G) * math.prod(self.qs[i] for i in G) for G in self.digits(l))
        return err * n * first / (self.P * self.qs[l - 1]) + (n_p + 0.5) * (n + 1)


def negacyclic(a, b):
    """a b mod X^n + 1 for signed coefficient vectors (Python integers)"""
    n = len(a)
    out = [0] * n
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            if i + j < n:
                out[i + j] += int(x) * int(y)
            else:
                out[i + j - n] -= int(x) * int(y)
    return np.array(out, dtype=object)
