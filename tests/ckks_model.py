"""Host models of the CKKS level operations (hexl_apply_galois, hexl_rescale, hexl_rotate) built from the oracle's transforms.

Layouts are the library's: a polynomial in NTT form is n words in the transforms' bit-reversed output order, moduli are the plan's
(NTT tables from MinimalPrimitiveRoot(2n, q), as hexl_ks_plan_create derives them without caller twiddles)."""
import numpy as np

from ks_util import extreme_words, rounding_edge_coeffs


def bitrev(j, logn):
    j = np.asarray(j, dtype=np.int64)
    out = np.zeros_like(j)
    for b in range(logn):
        out |= ((j >> b) & 1) << (logn - 1 - b)
    return out


def galois_src(n, g):
    """src[j]: NTT-form X -> X^g moves word src[j] of the input to word j of the output"""
    logn = n.bit_length() - 1
    e = ((2 * bitrev(np.arange(n), logn) + 1) * g) % (2 * n)
    return bitrev((e - 1) // 2, logn)


def apply_galois(x, n, g):
    """x[..., n] (any 64-bit words) -> the permuted copy"""
    x = np.asarray(x)
    return x.reshape(-1, n)[:, galois_src(n, g)].reshape(x.shape)


def automorphism_coeff(a, n, g, q):
    """coefficient domain: a(X) -> a(X^g) mod (X^n + 1, q)"""
    k = np.arange(n, dtype=np.int64)
    e = (k * g) % (2 * n)
    out = np.zeros(n, dtype=np.uint64)
    neg = e >= n
    vals = np.asarray(a, dtype=np.uint64)
    out[e % n] = np.where(neg, (np.uint64(q) - vals) % np.uint64(q), vals)
    return out


class Limbs:
    """NTT / INTT under each modulus of a chain, the keyswitch's transforms (orc_ks_ntt / orc_ks_intt)"""

    def __init__(self, orc, n, moduli):
        self.orc, self.n = orc, n
        self.qs = [int(q) for q in moduli]
        self.blks = []
        for q in self.qs:
            b = np.zeros(4 * n, dtype=np.uint64)
            orc.orc().orc_tables_keyswitch(n, q, orc.orc().orc_minimal_primitive_root(2 * n, q), orc.p(b))
            self.blks.append(b)

    def ntt(self, x, i):
        y = np.ascontiguousarray(x, dtype=np.uint64).copy()
        self.orc.orc().orc_ks_ntt(self.orc.p(y), self.n, self.qs[i], self.orc.p(self.blks[i][2 * self.n:3 * self.n]))
        return y

    def intt(self, x, i):
        y = np.ascontiguousarray(x, dtype=np.uint64).copy()
        self.orc.orc().orc_ks_intt(self.orc.p(y), self.n, self.qs[i], self.orc.p(self.blks[i][0:self.n]))
        return y


def rescale_poly(lm, c, n_limbs):
    """c[n_limbs][n] (NTT form, words < q_i) -> [n_limbs - 1][n]: the formula the kernels compute --
    s = (INTT_l(c_l) + half) mod q_l, out_i = (c_i - NTT_i((s + fix_i) mod q_i)) * q_l^-1 mod q_i"""
    n, l = lm.n, n_limbs - 1
    c = np.asarray(c, dtype=np.uint64).reshape(n_limbs, n)
    ql = lm.qs[l]
    half = ql >> 1
    s = (lm.intt(c[l], l).astype(object) + half) % ql
    out = np.empty((l, n), dtype=np.uint64)
    for i in range(l):
        qi = lm.qs[i]
        fix = qi - half % qi
        w = lm.ntt(np.array((s + fix) % qi, dtype=np.uint64), i).astype(object)
        out[i] = np.array((c[i].astype(object) - w) * pow(ql, -1, qi) % qi, dtype=np.uint64)
    return out


def rescale_crt(lm, c, n_limbs):
    """the same from the definition: NTT_i(round(X / q_l) mod q_i), X the CRT value of each coefficient (big integers)"""
    n, l = lm.n, n_limbs - 1
    c = np.asarray(c, dtype=np.uint64).reshape(n_limbs, n)
    qs = lm.qs[:n_limbs]
    Q = 1
    for q in qs:
        Q *= q
    X = np.zeros(n, dtype=object)
    for i, q in enumerate(qs):
        Qi = Q // q
        X = (X + lm.intt(c[i], i).astype(object) * (Qi * pow(Qi, -1, q))) % Q
    r = (X + qs[l] // 2) // qs[l]
    return np.stack([lm.ntt(np.array(r % qs[i], dtype=np.uint64), i) for i in range(l)])


def rescale_input(lm, n_limbs, n_components, family, b, seed=1):
    """instance b of a rescale input [n_components][n_limbs][n] (NTT form) from one of three families:
    uniform   every word uniform below its modulus
    extreme   every word of every limb from ks_util.extreme_words (q - 1, beside q / 2, 0, 1), in NTT form as it stands
    edge      kept limbs as in `extreme`; the dropped limb is NTT_l(rounding_edge_coeffs), so INTT_l(c_l) is exactly those words and
              s = (INTT_l(c_l) + half) mod q_l lands on 0, 1, q_l - 1 and both sides of the wrap"""
    n, l = lm.n, n_limbs - 1
    out = np.empty((n_components, n_limbs, n), dtype=np.uint64)
    for k in range(n_components):
        for i in range(n_limbs):
            w = b * 7 + k * 3 + i
            if family == "uniform":
                out[k, i] = lm.orc.splitmix(n, seed * 1009 + b * 101 + k * 13 + i, lm.qs[i])
            elif family == "edge" and i == l:
                out[k, i] = lm.ntt(rounding_edge_coeffs(n, lm.qs[l], w + seed), l)
            else:
                assert family in ("extreme", "edge"), family
                out[k, i] = extreme_words(n, lm.qs[i], w + seed)
    return out


def first_mismatch(got, want, shape_names, shape):
    """'instance 3, limb 1, coefficient 77: got ..., want ...' for the first differing word of two flat arrays of `shape`"""
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    bad = np.flatnonzero(got != want)
    if not len(bad):
        return "equal"
    idx = np.unravel_index(bad[0], shape)
    where = ", ".join(f"{nm} {int(v)}" for nm, v in zip(shape_names, idx))
    return f"{where}: got {int(got[bad[0]])}, want {int(want[bad[0]])} ({len(bad)} of {len(got)} words differ)"


def rescale(lm, x, batch, n_limbs, n_components):
    """x[batch][n_components][n_limbs][n] -> [batch][n_components][n_limbs - 1][n]"""
    x = np.asarray(x, dtype=np.uint64).reshape(batch, n_components, n_limbs, lm.n)
    return np.stack([np.stack([rescale_poly(lm, x[b, k], n_limbs) for k in range(n_components)]) for b in range(batch)])


def rotate(orc, case, ct, g):
    """ct[2][L][n] -> (sigma_g(c0), 0) + KeySwitch(sigma_g(c1)) with the case's keys"""
    n, L = case.n, case.L
    ct = np.asarray(ct, dtype=np.uint64).reshape(2, L * n)
    out = np.concatenate([apply_galois(ct[0], n, g), np.zeros(L * n, dtype=np.uint64)])
    orc.keyswitch(out, np.ascontiguousarray(apply_galois(ct[1], n, g)), n, L, case.K, L + 1, case.moduli, case.keys,
                  case.modswitch)
    return out
