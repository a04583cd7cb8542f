"""Host model of the hybrid key switch (include/hexl_mi355x.h hexl_hks_*) in Python integers, on the exact transforms
rns_model.py's models run on (ckks_model.Limbs: the oracle's keyswitch NTT / INTT under each modulus of the plan).

    L data limbs, S = {L .. K-1} special primes, P their product, alpha limbs per digit, dnum = ceil(L / alpha)
    level l: digits G_d = {d alpha .. min((d+1) alpha, l) - 1}, d < ceil(l / alpha); basis T_l = {0 .. l-1} + S
    1  a_i = INTT_i(t[i])
    2  y_i = a_i (D/q_i)^-1 mod q_i;  x_d[j] = sum_i y_i (D/q_i mod q_j) mod q_j;  ext_d[j] = NTT_j(x_d[j]) outside the digit, t[j] inside
    3  acc[k][j] = sum_d ext_d[j] key[d][k][j]
    4  b_s = INTT_s(acc[k][s]) + floor(P/2);  z_s = b_s (P/q_s)^-1;  w_i = sum_s z_s (P/q_s mod q_i)
       out[k][i] = result[k][i] + (acc[k][i] - NTT_i(w_i + fix_i)) P^-1,  fix_i = q_i - floor(P/2) mod q_i

Keys: hks keys are [dnum][2][K][n] (key d at d 2 K n, word (k K + i) n + j), as one flat uint64 array or a list of dnum arrays."""
import math

import numpy as np

from ckks_model import Limbs, apply_galois


class Hks:
    def __init__(self, orc, n, L, K, alpha, moduli, lm=None):
        assert 1 <= alpha <= L < K
        self.n, self.L, self.K, self.alpha = n, L, K, alpha
        self.qs = [int(q) for q in moduli[:K]]
        self.lm = lm or Limbs(orc, n, self.qs)
        self.dnum = -(-L // alpha)
        self.P = math.prod(self.qs[L:K])

    def digits(self, l):
        return [list(range(d * self.alpha, min((d + 1) * self.alpha, l))) for d in range(-(-l // self.alpha))]

    def basis(self, l):
        return list(range(l)) + list(range(self.L, self.K))

    def key_word_rows(self, keys):
        return np.asarray(keys, dtype=np.uint64).reshape(self.dnum, 2, self.K, self.n)

    def mod_up(self, t, l):
        """ext[d][jT] (uint64 rows, NTT form) for t[l][n]; jT indexes basis(l)"""
        lm, qs, n = self.lm, self.qs, self.n
        t = np.asarray(t, dtype=np.uint64).reshape(l, n)
        a = [lm.intt(t[i], i).astype(object) for i in range(l)]
        ext = []
        for G in self.digits(l):
            D = math.prod(qs[i] for i in G)
            y = {i: (a[i] * pow(D // qs[i], -1, qs[i])) % qs[i] for i in G}
            rows = []
            for j in self.basis(l):
                if j in G:
                    rows.append(t[j])
                    continue
                x = sum(y[i] * ((D // qs[i]) % qs[j]) for i in G) % qs[j]
                rows.append(lm.ntt(np.array(x, dtype=np.uint64), j))
            ext.append(rows)
        return ext

    def keyswitch(self, keys, t, result, l):
        """result[2][l][n] + KS(t[l][n]) -> flat uint64 [2][l][n], the words hexl_hks_keyswitch leaves in d_result"""
        lm, qs, n, L, K, P = self.lm, self.qs, self.n, self.L, self.K, self.P
        kw = self.key_word_rows(keys)
        res = np.asarray(result, dtype=np.uint64).reshape(2, l, n)
        ext = self.mod_up(t, l)
        basis = self.basis(l)
        half = P // 2
        out = np.empty((2, l, n), dtype=np.uint64)
        for k in range(2):
            acc = []
            for jT, j in enumerate(basis):
                s = np.zeros(n, dtype=object)
                for d in range(len(ext)):
                    s = s + ext[d][jT].astype(object) * kw[d, k, j].astype(object)
                acc.append(s % qs[j])
            z = {}
            for si, s in enumerate(range(L, K)):
                b = (lm.intt(np.array(acc[l + si], dtype=np.uint64), s).astype(object) + half % qs[s]) % qs[s]
                z[s] = (b * pow(P // qs[s], -1, qs[s])) % qs[s]
            for i in range(l):
                qi = qs[i]
                w = sum(z[s] * ((P // qs[s]) % qi) for s in range(L, K)) % qi
                fix = qi - half % qi
                wn = lm.ntt(np.array((w + fix) % qi, dtype=np.uint64), i).astype(object)
                out[k, i] = np.array((res[k, i].astype(object) + (acc[i] - wn) * pow(P, -1, qi)) % qi, dtype=np.uint64)
        return out.reshape(-1)

    def relinearize(self, keys, ct3, l):
        c = np.asarray(ct3, dtype=np.uint64).reshape(3, l, self.n)
        return self.keyswitch(keys, c[2], c[:2], l)

    def rotate(self, keys, ct, l, g):
        n = self.n
        c = np.asarray(ct, dtype=np.uint64).reshape(2, l, n)
        base = np.concatenate([apply_galois(c[0], n, g), np.zeros((l, n), dtype=np.uint64)])
        return self.keyswitch(keys, apply_galois(c[1], n, g), base, l)

    # ---- real keys, as KeySwitchPlan.gen_hybrid_key defines them, and the noise of a switch ----
    def ntt_signed(self, poly, i):
        q = self.qs[i]
        return self.lm.ntt(np.array([int(v) % q for v in poly], dtype=np.uint64), i).astype(object)

    def gen_key(self, s, s_from, rng, err=21):
        """keys [dnum][2][K][n] from the signed coefficient vectors s (the secret switched TO) and s_from: key d, limb i =
        (P [i in G_d] s_from + e_d - a_d s, a_d), e_d uniform in [-err, err], a_d uniform"""
        n, K, qs = self.n, self.K, self.qs
        keys = np.zeros((self.dnum, 2, K, n), dtype=np.uint64)
        for d, G in enumerate(self.digits(self.L)):
            e = rng.integers(-err, err + 1, n)
            for i in range(K):
                a = np.array([int(v) % qs[i] for v in rng.integers(0, 2**62, n)], dtype=object)
                pt = (self.P % qs[i]) * self.ntt_signed(s_from, i) if i in G else 0
                keys[d, 0, i] = np.array((pt + self.ntt_signed(e, i) - a * self.ntt_signed(s, i)) % qs[i], dtype=np.uint64)
                keys[d, 1, i] = np.array(a, dtype=np.uint64)
        return keys.reshape(-1)

    def noise(self, out, t, s, s_from, l):
        """the centred CRT lift over the l limbs of c0' + c1' s - t s_from, coefficient by coefficient (Python integers), for the key
        switch output `out`[2][l][n] of t[l][n] into a zero result"""
        lm, qs, n = self.lm, self.qs, self.n
        out = np.asarray(out, dtype=np.uint64).reshape(2, l, n)
        t = np.asarray(t, dtype=np.uint64).reshape(l, n)
        Q = math.prod(qs[:l])
        acc = np.zeros(n, dtype=object)
        for i in range(l):
            q = qs[i]
            v = (out[0, i].astype(object) + out[1, i].astype(object) * self.ntt_signed(s, i) - t[i].astype(object) * self.ntt_signed(s_from, i)) % q
            c = lm.intt(np.array(v, dtype=np.uint64), i).astype(object)
            acc = acc + c * ((Q // q) * pow(Q // q, -1, q))
        acc = acc % Q
        return np.array([int(v) - Q if int(v) > Q // 2 else int(v) for v in acc], dtype=object)

    def noise_bound(self, l, err=21):
        """B = err n sum_d |G_d| D_d / P + (n_p + 1/2)(n + 1): n coefficients of an extended digit below |G_d| D_d times a key error of
        magnitude <= err, divided by P; plus a rounding-plus-overshoot error below n_p + 1/2 per component times 1 + ||s||_1"""
        n, n_p = self.n, self.K - self.L
        first = sum(len(G) * math.prod(self.qs[i] for i in G) for G in self.digits(l))
        return err * n * first / self.P + (n_p + 0.5) * (n + 1)
