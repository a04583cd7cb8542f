"""Host model of the random streams of hexl_sample / hexl_rlwe_encrypt (include/hexl_mi355x.h): a numpy ChaCha20 block
function, the three kinds with their block addressing, and Python-integer encrypt / decrypt on the oracle's transforms
(ckks_model.Limbs). Layouts are the library's. Everything here follows the definition, not the kernels: 128-bit values and the small
maps are Python integers."""
import numpy as np

UNIFORM, TERNARY, CBD21 = 1, 2, 3
CONSTANTS = (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574)
MAX_INDEX = 1 << 40


def seed_of(raw):
    """32 bytes (or eight u32) -> eight little-endian u32 words"""
    if isinstance(raw, (bytes, bytearray)):
        assert len(raw) == 32
        return np.frombuffer(bytes(raw), dtype="<u4").astype(np.uint32)
    w = np.asarray(raw, dtype=np.uint32)
    assert w.shape == (8,)
    return w


def _rotl(x, k):
    return (x << np.uint32(k)) | (x >> np.uint32(32 - k))


def _quarter(x, a, b, c, d):
    x[a] += x[b]; x[d] = _rotl(x[d] ^ x[a], 16)
    x[c] += x[d]; x[b] = _rotl(x[b] ^ x[c], 12)
    x[a] += x[b]; x[d] = _rotl(x[d] ^ x[a], 8)
    x[c] += x[d]; x[b] = _rotl(x[b] ^ x[c], 7)


def chacha_blocks(seed, ctrs, stream):
    """[len(ctrs)][16] u32: the RFC 8439 block function on (constants, seed, ctr lo, ctr hi, stream lo, stream hi), one block per ctr"""
    seed = seed_of(seed)
    ctrs = np.asarray(ctrs, dtype=np.uint64).reshape(-1)
    m = len(ctrs)
    state = [np.full(m, v, dtype=np.uint32) for v in CONSTANTS] + [np.full(m, v, dtype=np.uint32) for v in seed]
    state += [(ctrs & np.uint64(0xFFFFFFFF)).astype(np.uint32), (ctrs >> np.uint64(32)).astype(np.uint32),
              np.full(m, stream & 0xFFFFFFFF, dtype=np.uint32), np.full(m, (stream >> 32) & 0xFFFFFFFF, dtype=np.uint32)]
    x = [s.copy() for s in state]
    with np.errstate(over="ignore"):
        for _ in range(10):
            _quarter(x, 0, 4, 8, 12); _quarter(x, 1, 5, 9, 13); _quarter(x, 2, 6, 10, 14); _quarter(x, 3, 7, 11, 15)
            _quarter(x, 0, 5, 10, 15); _quarter(x, 1, 6, 11, 12); _quarter(x, 2, 7, 8, 13); _quarter(x, 3, 4, 9, 14)
        out = [a + b for a, b in zip(x, state)]
    return np.stack(out, axis=1)


def lanes(blocks):
    """[m][16] u32 -> [m][8] u64: lane t = w[2t] | w[2t+1] << 32"""
    b = blocks.astype(np.uint64)
    return b[:, 0::2] | (b[:, 1::2] << np.uint64(32))


def _ctrs(kind, first_block, count):
    assert first_block + count <= 1 << 60
    return np.array([(kind << 60) | (first_block + k) for k in range(count)], dtype=np.uint64)


def ternary_of(r):
    return ((int(r) * 3) >> 64) - 1


def cbd21_of(r):
    r = int(r)
    return bin(r & 0x1FFFFF).count("1") - bin((r >> 21) & 0x1FFFFF).count("1")


def mod128(hi, lo, q):
    return ((int(hi) << 64) + int(lo)) % q


_cache = {}


def uniform(seed, stream, c, i, n, q):
    """the n words of polynomial (c, limb i) modulo q: word j from block ((c 16 + i) n + j) >> 2, lanes 2 (j & 3) (low) and + 1 (high)"""
    key = (UNIFORM, bytes(seed_of(seed).tobytes()), stream, c, i, n, q)
    if key not in _cache:
        base = (c * 16 + i) * n
        assert base % 4 == 0
        ln = lanes(chacha_blocks(seed, _ctrs(UNIFORM, base >> 2, n // 4), stream)).reshape(n, 2).astype(object)
        _cache[key] = np.array((ln[:, 0] + (ln[:, 1] << 64)) % q, dtype=np.uint64)
    return _cache[key]


def small(seed, stream, kind, c, n):
    """the n integer coefficients of polynomial c: coefficient j from block (c n + j) >> 3, lane j & 7"""
    assert kind in (TERNARY, CBD21)
    key = (kind, bytes(seed_of(seed).tobytes()), stream, c, n)
    if key not in _cache:
        ln = lanes(chacha_blocks(seed, _ctrs(kind, (c * n) >> 3, n // 8), stream)).reshape(n)
        f = ternary_of if kind == TERNARY else cbd21_of
        _cache[key] = np.array([f(r) for r in ln], dtype=np.int64)
    return _cache[key]


def small_words(lm, v, i):
    """NTT_i(v mod q_i): negative v as q_i - |v|"""
    q = lm.qs[i]
    return lm.ntt(np.array([int(x) % q for x in v], dtype=np.uint64), i)


def sample(lm, kind, seed, stream, first, count, n_limbs):
    """hexl_sample: [count][n_limbs][n]"""
    assert first + count <= MAX_INDEX
    out = np.empty((count, n_limbs, lm.n), dtype=np.uint64)
    for b in range(count):
        v = None if kind == UNIFORM else small(seed, stream, kind, first + b, lm.n)
        for i in range(n_limbs):
            out[b, i] = uniform(seed, stream, first + b, i, lm.n, lm.qs[i]) if kind == UNIFORM else small_words(lm, v, i)
    return out


def encrypt_with(qs, n, a, e, s, pt=None):
    """(pt + e - a s, a) for given a, e, s (and pt) [n_limbs][n] in NTT form, Python integers: [2][n_limbs][n]"""
    n_limbs = len(a)
    out = np.empty((2, n_limbs, n), dtype=np.uint64)
    for i in range(n_limbs):
        c0 = np.asarray(e[i]).astype(object) - np.asarray(a[i]).astype(object) * np.asarray(s[i]).astype(object)
        if pt is not None:
            c0 = c0 + np.asarray(pt[i]).astype(object)
        out[0, i] = np.array(c0 % int(qs[i]), dtype=np.uint64)
        out[1, i] = a[i]
    return out


def encrypt(lm, seed, stream, c, n_limbs, s, pt=None):
    """one instance of hexl_rlwe_encrypt, absolute index c: a = UNIFORM, e = CBD21 of (seed, stream, c)"""
    a = [uniform(seed, stream, c, i, lm.n, lm.qs[i]) for i in range(n_limbs)]
    ev = small(seed, stream, CBD21, c, lm.n)
    e = [small_words(lm, ev, i) for i in range(n_limbs)]
    return encrypt_with(lm.qs, lm.n, a, e, s, pt)


def decrypt(qs, n, ct, s, n_components, n_limbs):
    """c0 + c1 s (+ c2 s^2) mod q_i from the definition: [n_limbs][n]"""
    ct = np.asarray(ct, dtype=np.uint64).reshape(n_components, n_limbs, n).astype(object)
    out = np.empty((n_limbs, n), dtype=np.uint64)
    for i in range(n_limbs):
        si = np.asarray(s[i]).astype(object)
        v = ct[0, i] + ct[1, i] * si
        if n_components == 3:
            v = v + ct[2, i] * si * si
        out[i] = np.array(v % int(qs[i]), dtype=np.uint64)
    return out


def switching_key_plaintext(qs, n, L, K, s_from):
    """pt[d][i] = [i == d] (P mod q_i) s'_i, P = qs[K - 1]: [L][K][n] from s_from[K][n] (NTT form)"""
    P = int(qs[K - 1])
    pt = np.zeros((L, K, n), dtype=np.uint64)
    for d in range(L):
        pt[d, d] = np.array(np.asarray(s_from[d]).astype(object) * (P % int(qs[d])) % int(qs[d]), dtype=np.uint64)
    return pt
