"""Host model of hexl_rotate_hoisted in exact integers (Python integers in numpy object arrays) on ckks_model.Limbs' transforms:

    c_d        = INTT_d(c1[d])                                             the keyswitch's step 1
    u[d][slot] = NTT_slot(c_d mod q_slot), slot = the L data limbs and the special prime     step 2 -- ONCE per ciphertext (mod_up)
    prod[k][slot] = sum_d sigma_g(u[d][slot]) . key[d][k][slot]  mod q_slot          sigma_g = ckks_model.apply_galois, the word permutation
    s'_k       = (INTT_sp(prod[k][sp]) + floor(q_sp / 2)) mod q_sp
    out[k][i]  = [k = 0] sigma_g(c0)[i] + (prod[k][i] - NTT_i((s'_k + fix_i) mod q_i)) . msf_i  mod q_i
                 fix_i = q_i - (floor(q_sp / 2) mod q_i), msf_i = the case's modswitch factor

At g = 1 this is the oracle's keyswitch word for word (test_hoist_model.py); for g != 1 it is NOT ckks_model.rotate: the digits of c1
are lifted and then permuted, rotate permutes and then lifts (include/hexl_mi355x.h)."""
import numpy as np

from ckks_model import Limbs, apply_galois, automorphism_coeff


def limbs_of(orc, case):
    return Limbs(orc, case.n, case.moduli)


def mod_up(lm, case, ct):
    """u[d][si] (object arrays below q_slot) for ct[2][L][n]; si = 0 ... L - 1 are the data limbs, si = L the special prime"""
    n, L, K = case.n, case.L, case.K
    c1 = np.asarray(ct, dtype=np.uint64).reshape(2, L, n)[1]
    slots = list(range(L)) + [K - 1]
    u = []
    for d in range(L):
        c_d = lm.intt(c1[d], d)
        u.append([lm.ntt(c_d % np.uint64(lm.qs[i]), i).astype(object) for i in slots])
    return u


def rotate_hoisted(orc, case, ct, g, lm=None, u=None):
    """ct[2][L][n] -> out[2][L][n] (flat uint64), the words hexl_rotate_hoisted writes for Galois element g and the case's keys.
    `lm` (limbs_of) and `u` (mod_up of the same ct) may be passed in to share them between rotations, as the launcher does."""
    n, L, K = case.n, case.L, case.K
    lm = lm or limbs_of(orc, case)
    u = u or mod_up(lm, case, ct)
    c0 = np.asarray(ct, dtype=np.uint64).reshape(2, L, n)[0]
    slots = list(range(L)) + [K - 1]
    q_sp, half = lm.qs[K - 1], lm.qs[K - 1] >> 1
    out = np.empty((2, L, n), dtype=np.uint64)
    for k in range(2):
        prod = []
        for si, i in enumerate(slots):
            acc = np.zeros(n, dtype=object)
            for d in range(L):
                key = case.keys[d][(k * K + i) * n:(k * K + i + 1) * n].astype(object)
                acc = acc + apply_galois(u[d][si], n, g) * key
            prod.append(acc % lm.qs[i])
        s = (lm.intt(np.array(prod[L], dtype=np.uint64), K - 1).astype(object) + half) % q_sp
        for i in range(L):
            qi = lm.qs[i]
            fix = qi - half % qi
            w = lm.ntt(np.array((s + fix) % qi, dtype=np.uint64), i).astype(object)
            first = apply_galois(c0[i], n, g).astype(object) if k == 0 else 0
            out[k, i] = np.array((first + (prod[i] - w) * int(case.modswitch[i])) % qi, dtype=np.uint64)
    return out.reshape(-1)


class GaloisRlwe:
    """A real Galois key in ks_util.RlweCase's construction (s_old = s, s_new = sigma_g(s)) and an encryption (c0, c1) of a message m
    under s: a rotation by g, hoisted or not, must decrypt under s to sigma_g(m) up to key-switch noise. Has the fields of a KsCase
    that the models read (n, L, K, moduli, modswitch, keys)."""

    def __init__(self, orc, rc, g, seed=9):
        """rc: an RlweCase, for its moduli, its transforms and its secret s_old"""
        self.rc, self.g = rc, g
        self.n, self.L, self.K = rc.n, rc.L, rc.K
        self.moduli, self.modswitch = rc.moduli, rc.modswitch
        n, L, K, qs = rc.n, rc.L, rc.K, rc.qs
        P = qs[K - 1]
        rng = np.random.default_rng(seed)
        s = rc.s_old
        self.s_ntt = [rc.ntt(s, i) for i in range(K)]
        s_rot = self.sigma_signed(s)
        self.keys = []
        for d in range(L):
            e = rng.integers(-3, 4, n)
            key = np.zeros(2 * K * n, dtype=np.uint64)
            for i in range(K):
                a = rc.ntt(rng.integers(0, 2**62, n).astype(object) % qs[i], i)
                b = (-a * self.s_ntt[i] + rc.ntt(e, i) + (P % qs[i] if i == d else 0) * rc.ntt(s_rot, i)) % qs[i]
                key[i * n:(i + 1) * n] = np.array(b, dtype=np.uint64)
                key[(K + i) * n:(K + i + 1) * n] = np.array(a, dtype=np.uint64)
            self.keys.append(key)
        self.m = rng.integers(-2**30, 2**30, n)
        e = rng.integers(-3, 4, n)
        a_int = rng.integers(0, 2**62, n).astype(object)
        c0, c1 = [], []
        for i in range(L):
            a = rc.ntt(a_int % qs[i], i)
            c1.append(np.array(a, dtype=np.uint64))
            c0.append(np.array((-a * self.s_ntt[i] + rc.ntt(e, i) + rc.ntt(self.m, i)) % qs[i], dtype=np.uint64))
        self.ct = np.concatenate(c0 + c1)

    def sigma_signed(self, poly):
        """coefficient domain, signed integers: poly(X) -> poly(X^g) mod X^n + 1"""
        n = self.n
        big = 1 << 62
        img = automorphism_coeff(np.array([int(v) % big for v in poly], dtype=np.uint64), n, self.g, big)
        return np.array([int(v) - big if int(v) >= big >> 1 else int(v) for v in img], dtype=object)

    def check(self, out, noise_bits=24):
        """out[2][L][n] decrypts under s to sigma_g(m) + noise, |noise| < 2^noise_bits (RlweCase.check's bound for the plain keyswitch),
        the same noise polynomial in every limb"""
        rc, n, L = self.rc, self.n, self.L
        out = np.asarray(out, dtype=np.uint64).reshape(2, L, n)
        m_rot = self.sigma_signed(self.m)
        noises = []
        for i in range(L):
            q = rc.qs[i]
            dec = rc.intt((out[0, i].astype(object) + out[1, i].astype(object) * self.s_ntt[i]) % q, i)
            centred = np.array([int(v) if v <= q // 2 else int(v) - q for v in dec], dtype=object)
            noise = centred - m_rot
            assert max(abs(int(v)) for v in noise) < 1 << noise_bits, f"limb {i}: does not decrypt to sigma_g(m)"
            noises.append(noise)
        for i in range(1, L):
            assert (noises[i] == noises[0]).all(), "limbs disagree on the noise polynomial"
