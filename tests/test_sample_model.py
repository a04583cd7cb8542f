"""CPU: tests/sample_model.py pinned -- the block function against RFC 8439 section 2.3.2 (and against openssl's chacha20 where the
program exists), the two small maps at their boundaries, r mod q against Python, the block addressing, the distributions (properties of
the model, checked here and nowhere on the GPU), decrypt(encrypt(pt)) - pt == NTT(e), and the key-shaped output against the formula of
ks_util.RlweCase."""
import shutil
import subprocess

import numpy as np

import sample_model as sm
from ckks_model import Limbs
from ks_util import RlweCase, primes_below

RFC_KEY = bytes(range(32))
RFC_CTR = 1 | (0x09000000 << 32)
RFC_STREAM = 0x4A000000
RFC_HEAD = bytes.fromhex("10f1e7e4d13b5915500fdd1fa32071c4")
RFC_TAIL = bytes.fromhex("a2503c4e")
# RFC 8439 2.3.2, the whole serialized block
RFC_BLOCK = bytes.fromhex("10f1e7e4d13b5915500fdd1fa32071c4c7d1f4c733c068030422aa9ac3d46c4e"
                          "d2826446079faa0914c2d705d98b02a2b5129cd1de164eb9cbd083e8a2503c4e")


def test_block_function_is_rfc8439():
    blk = sm.chacha_blocks(RFC_KEY, [RFC_CTR], RFC_STREAM)
    raw = blk.astype("<u4").tobytes()
    assert raw[:16] == RFC_HEAD and raw[-4:] == RFC_TAIL
    assert raw == RFC_BLOCK
    ln = sm.lanes(blk)[0]
    assert int(ln[0]) == int.from_bytes(raw[:8], "little") and int(ln[7]) == int.from_bytes(raw[56:], "little")
    # vectorised over counters: block k of a batch is the block of its own counter
    many = sm.chacha_blocks(RFC_KEY, [RFC_CTR + k for k in range(5)], RFC_STREAM)
    assert np.array_equal(many[0], blk[0])
    assert np.array_equal(many[3], sm.chacha_blocks(RFC_KEY, [RFC_CTR + 3], RFC_STREAM)[0])
    assert len({m.tobytes() for m in many}) == 5


def test_keystream_matches_openssl_where_it_exists():
    """openssl's 16-byte IV is counter || nonce, little-endian: exactly state words 12 ... 15"""
    exe = shutil.which("openssl")
    if exe is None:
        print("openssl not installed: the RFC vector alone pins the block function")
        return
    seed = bytes((7 * k + 3) & 0xFF for k in range(32))
    ctr, stream = (sm.UNIFORM << 60) | 0x123456789, 0xFEDCBA9876543210
    iv = ctr.to_bytes(8, "little") + stream.to_bytes(8, "little")
    r = subprocess.run([exe, "enc", "-chacha20", "-K", seed.hex(), "-iv", iv.hex()], input=bytes(192), capture_output=True, timeout=60)
    if r.returncode != 0 or len(r.stdout) != 192:
        print("this openssl has no raw chacha20:", r.stderr[-200:])
        return
    want = sm.chacha_blocks(seed, [ctr, ctr + 1, ctr + 2], stream).astype("<u4").tobytes()
    assert r.stdout == want


def test_ternary_boundaries():
    t1, t2 = -(-(1 << 64) // 3), -(-(1 << 65) // 3)                # ceil(2^64 / 3), ceil(2^65 / 3)
    for r, v in ((0, -1), (1, -1), (t1 - 1, -1), (t1, 0), (t1 + 1, 0), (t2 - 1, 0), (t2, 1), (t2 + 1, 1), ((1 << 64) - 1, 1),
                 (1 << 63, 0), ((1 << 63) - 1, 0)):
        assert sm.ternary_of(r) == v, hex(r)
    assert t1 * 3 >= 1 << 64 > (t1 - 1) * 3 and t2 * 3 >= 1 << 65 > (t2 - 1) * 3


def test_cbd21_halves():
    ones = 0x1FFFFF
    for r, v in ((0, 0), (ones, 21), (ones << 21, -21), (ones | (ones << 21), 0), ((1 << 64) - 1, 0), (~(ones << 21) & ((1 << 64) - 1), 21),
                 (1, 1), (1 << 20, 1), (1 << 21, -1), (1 << 41, -1), (1 << 42, 0), (0xFFFFFC0000000000, 0), (0x155555, 11), (0x0AAAAA, 10)):
        assert sm.cbd21_of(r) == v, hex(r)


def test_mod128_extremes(orc):
    top = (1 << 64) - 1
    for bits in (27, 30, 40, 49, 50, 51, 52):
        q = primes_below(orc, 1, 1 << bits, 1024)[0]
        for hi in (0, 1, q - 1, q, top - 1, top, 1 << 63):
            for lo in (0, 1, q - 1, q, top - 1, top, 1 << 63):
                want = (hi * (1 << 64) + lo) % q
                assert sm.mod128(hi, lo, q) == want
                assert ((hi % q) * ((1 << 64) % q) + lo % q) % q == want          # the two-step route through 2^64 mod q


def test_addressing_and_limb_prefix(orc):
    n = 1024
    qs = primes_below(orc, 3, 1 << 40, n)
    seed, stream = bytes(range(1, 33)), 5
    c, i = (1 << 40) - 1, 2
    a = sm.uniform(seed, stream, c, i, n, qs[i])
    for j in (0, 1, 3, 4, 517, n - 1):
        blk = sm.lanes(sm.chacha_blocks(seed, [(1 << 60) | (((c * 16 + i) * n + j) >> 2)], stream))[0]
        t = 2 * (j & 3)
        assert int(a[j]) == (int(blk[t]) + (int(blk[t + 1]) << 64)) % qs[i]
    assert (((c * 16 + 15) * 32768 + 32767) >> 2) < 1 << 60
    v = sm.small(seed, stream, sm.CBD21, c, n)
    for j in (0, 7, 8, 1023):
        blk = sm.lanes(sm.chacha_blocks(seed, [(3 << 60) | ((c * n + j) >> 3)], stream))[0]
        assert int(v[j]) == sm.cbd21_of(blk[j & 7])
    lm = Limbs(orc, n, qs)
    hi, lo = sm.sample(lm, sm.UNIFORM, seed, stream, 7, 2, 3), sm.sample(lm, sm.UNIFORM, seed, stream, 7, 2, 2)
    assert np.array_equal(hi[:, :2], lo)
    # kinds, streams, seeds and indices are separate streams
    t = sm.small(seed, stream, sm.TERNARY, c, n)
    assert not np.array_equal(t, np.clip(v, -1, 1))
    assert not np.array_equal(a, sm.uniform(seed, stream + 1, c, i, n, qs[i]))
    assert not np.array_equal(a, sm.uniform(bytes(32), stream, c, i, n, qs[i]))
    assert not np.array_equal(a, sm.uniform(seed, stream, c - 1, i, n, qs[i]))


def test_distributions():
    """8 x 4096 coefficients of each small kind, 4096 uniform words: means and variances within six standard errors"""
    seed, n = bytes(range(64, 96)), 4096
    t = np.concatenate([sm.small(seed, 1, sm.TERNARY, c, n) for c in range(8)]).astype(float)
    e = np.concatenate([sm.small(seed, 1, sm.CBD21, c, n) for c in range(8)]).astype(float)
    m = len(t)
    assert set(np.unique(t)) == {-1.0, 0.0, 1.0} and np.abs(e).max() <= 21
    assert abs(t.mean()) < 6 * np.sqrt(2 / 3 / m) and abs(t.var() - 2 / 3) < 6 * np.sqrt(2 / 9 / m)     # var of t^2: 2/3 - 4/9
    assert abs(e.mean()) < 6 * np.sqrt(10.5 / m)
    assert abs(e.var() - 10.5) < 6 * np.sqrt(2 * 10.5 ** 2 / m) * 1.1                                     # near-normal fourth moment
    q = (1 << 40) - 87
    u = sm.uniform(seed, 1, 0, 0, n, q).astype(float) / q
    assert abs(u.mean() - 0.5) < 6 * np.sqrt(1 / 12 / n) and 0.0 <= u.min() and u.max() < 1.0


def test_decrypt_of_encrypt_is_plaintext_plus_error(orc):
    n, K = 1024, 3
    qs = primes_below(orc, 1, 1 << 52, n) + primes_below(orc, 1, 1 << 30, n) + primes_below(orc, 1, 1 << 27, n)
    lm = Limbs(orc, n, qs)
    seed, stream, c = bytes(range(100, 132)), 9, 12345
    sv = sm.small(seed, stream, sm.TERNARY, 0, n)
    s = [sm.small_words(lm, sv, i) for i in range(K)]
    pt = [orc.splitmix(n, 77 + i, qs[i]) for i in range(K)]
    ev = sm.small(seed, stream, sm.CBD21, c, n)
    for plain in (pt, None):
        ct = sm.encrypt(lm, seed, stream, c, K, s, plain)
        assert all(np.array_equal(ct[1, i], sm.uniform(seed, stream, c, i, n, qs[i])) for i in range(K))
        dec = sm.decrypt(qs, n, ct, s, 2, K)
        for i in range(K):
            diff = (dec[i].astype(object) - (0 if plain is None else plain[i].astype(object))) % qs[i]
            assert np.array_equal(np.array(diff, dtype=np.uint64), sm.small_words(lm, ev, i))
            back = lm.intt(np.array(diff, dtype=np.uint64), i).astype(object)
            assert np.array_equal(np.where(back > qs[i] // 2, back - qs[i], back).astype(np.int64), ev)
    # three components: c0 + c1 s + c2 s^2 against Horner in Python integers
    ct3 = np.array([[orc.splitmix(n, 900 + 10 * k + i, qs[i]) for i in range(K)] for k in range(3)])
    dec = sm.decrypt(qs, n, ct3, s, 3, K)
    for i in range(K):
        so = s[i].astype(object)
        assert np.array_equal(dec[i], np.array(((ct3[2, i].astype(object) * so + ct3[1, i].astype(object)) * so + ct3[0, i].astype(object)) % qs[i],
                                               dtype=np.uint64))


def test_key_shaped_output_is_rlwecase_formula(orc):
    """RlweCase builds key d, limb i as b = -a s_old + e + [i == d] P s_new, (b, a) at ((k K + i) n): feed its formula the model's a and e"""
    n, L, K = 1024, 2, 3
    case = RlweCase(orc, n, L, K, 40)
    qs = case.qs
    lm = Limbs(orc, n, qs)
    seed, stream = bytes(range(32)), 3
    s_old = [np.array(case.ntt(case.s_old, i), dtype=np.uint64) for i in range(K)]
    s_new = [np.array(case.ntt(case.s_new, i), dtype=np.uint64) for i in range(K)]
    pt = sm.switching_key_plaintext(qs, n, L, K, s_new)
    P = qs[K - 1]
    for d in range(L):
        key = sm.encrypt(lm, seed, stream, d, K, s_old, pt[d]).reshape(-1)
        ev = sm.small(seed, stream, sm.CBD21, d, n)
        for i in range(K):
            a = sm.uniform(seed, stream, d, i, n, qs[i]).astype(object)
            b = (-a * case.ntt(case.s_old, i) + case.ntt(ev, i) + (P % qs[i] if i == d else 0) * case.ntt(case.s_new, i)) % qs[i]
            assert np.array_equal(key[(0 * K + i) * n:(0 * K + i + 1) * n], np.array(b, dtype=np.uint64))
            assert np.array_equal(key[(1 * K + i) * n:(1 * K + i + 1) * n], np.array(a, dtype=np.uint64))
