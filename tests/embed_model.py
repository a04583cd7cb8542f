"""Host model of the device-side encode / decode (hexl_rns_from_f64, hexl_rns_to_f64, hexl_ckks_encode, hexl_ckks_decode) on top of
ckks_model.Limbs. The canonical embedding is the example's two formulas (examples/ckks_flow_example.cpp embed / embed_inverse),
  z_k = m(zeta^(5^k)),   m_j = (2/n) Re(sum_k z_k zeta^(-j 5^k)),   zeta = exp(i pi / n), k < n/2,
vectorised in np.longdouble: np.fft computes in double, so the transform is a hand radix-2 FFT (embed_direct is the formula itself,
O(n^2), for pinning the FFT at small n). from_f64 and the CRT centre-lift are Python integers."""
import numpy as np

LD, CLD = np.longdouble, np.clongdouble
PI = LD(4) * np.arctan(LD(1))


def zeta_pow(n, e):
    """zeta^e for integer exponents e (any shape), reduced mod 2n first"""
    ang = PI * (np.asarray(e, dtype=np.int64) % (2 * n)).astype(LD) / LD(n)
    return np.cos(ang) + 1j * np.sin(ang).astype(CLD)


def slot_exponents(n):
    """5^k mod 2n, k < n/2"""
    out, e = np.empty(n // 2, dtype=np.int64), 1
    for k in range(n // 2):
        out[k] = e
        e = e * 5 % (2 * n)
    return out


def fft(x, sign):
    """X_s = sum_j x_j exp(sign 2 pi i j s / N) over the last axis, N a power of two, in long double"""
    x = np.asarray(x, dtype=CLD)
    N = x.shape[-1]
    if N == 1:
        return x
    ev, od = fft(x[..., 0::2], sign), fft(x[..., 1::2], sign)
    ang = LD(sign) * 2 * PI * np.arange(N // 2).astype(LD) / LD(N)
    t = (np.cos(ang) + 1j * np.sin(ang).astype(CLD)) * od
    return np.concatenate([ev + t, ev - t], axis=-1)


def embed(m, n):
    """coefficients m[..., n] (real) -> slots z[..., n/2], z_k = m(zeta^(5^k)): with u_j = m_j + i m_(j + n/2) (zeta^(n/2 . e) = i for
    e = 1 mod 4) and 5^k = 4 s + 1, z_k = sum_(j < n/2) u_j zeta^j exp(2 pi i j s / (n/2))"""
    m = np.asarray(m, dtype=LD)
    h = n // 2
    u = (m[..., :h] + 1j * m[..., h:].astype(CLD)) * zeta_pow(n, np.arange(h))
    return fft(u, +1)[..., (slot_exponents(n) - 1) // 4]


def embed_inverse(z, n):
    """slots z[..., n/2] -> the real coefficients m[..., n] (long double, unrounded) of the polynomial with m(zeta^(5^k)) = z_k"""
    z = np.asarray(z, dtype=CLD)
    h = n // 2
    w = np.zeros(z.shape, dtype=CLD)
    w[..., (slot_exponents(n) - 1) // 4] = z
    u = fft(w, -1) * np.conj(zeta_pow(n, np.arange(h))) / LD(h)
    return np.concatenate([u.real, u.imag], axis=-1)


def embed_direct(m, n):
    """the formula itself: z_k = sum_j m_j zeta^(j 5^k)"""
    m = np.asarray(m, dtype=LD)
    e = slot_exponents(n)
    return (zeta_pow(n, np.outer(e, np.arange(n))) * m).sum(axis=-1)


def embed_inverse_direct(z, n):
    """the formula itself: m_j = (2/n) Re(sum_k z_k zeta^(-j 5^k))"""
    z = np.asarray(z, dtype=CLD)
    e = slot_exponents(n)
    return (np.conj(zeta_pow(n, np.outer(np.arange(n), e))) * z).sum(axis=-1).real * LD(2) / LD(n)


def as_double_slots(z):
    """complex long-double slots -> float64 [..., n/2, 2] (re, im), each part rounded once"""
    z = np.asarray(z)
    return np.stack([z.real.astype(np.float64), z.imag.astype(np.float64)], axis=-1)


def rint_ints(c):
    """float64 coefficients -> Python integers, round to nearest, ties to even (exact: np.rint of a double is a double integer)"""
    return np.array([int(v) for v in np.rint(np.asarray(c, dtype=np.float64)).reshape(-1)], dtype=object)


def ints_to_words(lm, r, n_limbs):
    """integer coefficients r[n] (Python integers, any sign) -> [n_limbs][n] NTT-form words, limb i = NTT_i(r mod q_i)"""
    r = np.asarray(r, dtype=object)
    return np.stack([lm.ntt(np.array(r % lm.qs[i], dtype=np.uint64), i) for i in range(n_limbs)])


def from_f64(lm, c, n_limbs):
    """hexl_rns_from_f64 of one instance c[n]"""
    return ints_to_words(lm, rint_ints(c), n_limbs)


def crt_lift(lm, words, n_limbs):
    """[n_limbs][n] NTT-form words -> the centred CRT value of every coefficient in (-Q/2, Q/2), Python integers"""
    words = np.asarray(words, dtype=np.uint64).reshape(n_limbs, lm.n)
    qs = lm.qs[:n_limbs]
    Q = 1
    for q in qs:
        Q *= q
    X = np.zeros(lm.n, dtype=object)
    for i, q in enumerate(qs):
        Qi = Q // q
        X = (X + lm.intt(words[i], i).astype(object) * (Qi * pow(Qi, -1, q))) % Q
    return np.array([int(v) - Q if int(v) > Q // 2 else int(v) for v in X], dtype=object)


def ints_to_ld(x):
    """Python integers of any size -> long double, correctly rounded up to the two-piece split (error below 2^-100 relative)"""
    out = np.empty(len(x), dtype=LD)
    for j, v in enumerate(x):
        v = int(v)
        hi = float(v)                       # correctly rounded
        out[j] = LD(hi) + LD(float(v - int(hi)))
    return out
