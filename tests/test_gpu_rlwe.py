"""GPU: hexl_sample / hexl_rlwe_encrypt / hexl_rlwe_decrypt bit-exact against the host model (tests/sample_model.py: a numpy ChaCha20 and
Python integers on the oracle's transforms), every word of every instance; the first wrong word is named. Ring sizes 1024 (one chunk
per polynomial), 2048 (two: block addressing across the seam) and one case at 16384; the chains strict / period3_top / period12 / seal
at K = 5 (seal: moduli from 27 to 52 bits). Outputs are pre-filled with -1. No statistical thresholds here: the distributions are
properties of the model (tests/test_sample_model.py)."""
import math

import numpy as np
import pytest

import sample_model as sm
from ckks_model import Limbs
from ks_util import KsCase, extreme_ciphertext
from rns_model import assert_instances, chain
from test_gpu_streams import Op, assert_every, closing, dev_pair, fill, first_then_warm, side_context  # noqa: F401  (closing, fill: fixtures)

pytestmark = pytest.mark.gpu

K, COUNT = 5, 3
KINDS = ["strict", "period3_top", "period12", "seal"]
SEEDS = [bytes(range(32)), bytes((251 * k + 17) & 0xFF for k in range(32))]
STREAMS = [0, 0xFEDCBA9876543210]
FIRSTS = [0, 5, (1 << 40) - 3]
NAMES = ("limb", "coefficient")


def make_plan(hx, ctx, orc, n, qs, L=1):
    k = len(qs)
    case = KsCase(orc, n, L, k, moduli=qs)
    return hx.KeySwitchPlan(ctx, n, L, k, k, 2, case.moduli, case.modswitch)       # no keys: nothing here needs them


_lm = {}


def limbs(orc, kind, n):
    if (kind, n) not in _lm:
        _lm[kind, n] = Limbs(orc, n, chain(orc, kind, K, n))
    return _lm[kind, n]


def minus_one(dev, words):
    import torch
    return torch.full((words,), -1, dtype=torch.int64, device=dev)


def up(hx, dev, a):
    return hx.as_i64(np.ascontiguousarray(a, dtype=np.uint64).reshape(-1)).to(dev)


def secret_of(lm, seed, rows):
    """NTT_i of one ternary polynomial (index 0 of stream 77), `rows` limbs"""
    v = sm.small(seed, 77, sm.TERNARY, 0, lm.n)
    return np.stack([sm.small_words(lm, v, i) for i in range(rows)])


def check_sample(hx, ctx, dev, plan, lm, kind, seed, stream, first, count, n_limbs, label):
    n = lm.n
    out = minus_one(dev, count * n_limbs * n + n)                  # n words behind the output stay -1
    plan.sample(out, kind, count, n_limbs, seed=seed, stream=stream, first=first)
    ctx.sync()
    got = hx.to_u64(out)
    want = sm.sample(lm, kind, seed, stream, first, count, n_limbs)
    assert_instances(got[:count * n_limbs * n], want, count, NAMES, (n_limbs, n), f"{label} kind={kind} stream={stream:#x} first={first} n_limbs={n_limbs}")
    assert (got[count * n_limbs * n:] == np.uint64(0xFFFFFFFFFFFFFFFF)).all(), f"{label}: wrote behind the output"
    assert all(int(got.reshape(-1)[:count * n_limbs * n].reshape(count, n_limbs, n)[:, i].max()) < lm.qs[i] for i in range(n_limbs))


@pytest.mark.parametrize("kind", KINDS)
def test_sample_matrix(hx, ctx, dev, orc, kind):
    """n = 1024: n_limbs {1, 3, K} x each kind x first {0, 5, 2^40 - 3} x two seeds x two streams, count 3"""
    n = 1024
    lm = limbs(orc, kind, n)
    plan = make_plan(hx, ctx, orc, n, lm.qs)
    for n_limbs in (1, 3, K):
        for what in (sm.UNIFORM, sm.TERNARY, sm.CBD21):
            for first in FIRSTS:
                for seed in SEEDS:
                    for stream in STREAMS:
                        check_sample(hx, ctx, dev, plan, lm, what, seed, stream, first, COUNT, n_limbs, kind)
    plan.close()


@pytest.mark.parametrize("kind", ["strict", "seal"])
def test_sample_two_chunks_per_polynomial(hx, ctx, dev, orc, kind):
    """n = 2048: two 1024-word chunks per polynomial, the block index runs across the seam"""
    n = 2048
    lm = limbs(orc, kind, n)
    plan = make_plan(hx, ctx, orc, n, lm.qs)
    for what in (sm.UNIFORM, sm.TERNARY, sm.CBD21):
        check_sample(hx, ctx, dev, plan, lm, what, SEEDS[1], STREAMS[1], 5, COUNT, 3, kind)
    check_sample(hx, ctx, dev, plan, lm, sm.UNIFORM, SEEDS[0], 1, (1 << 40) - 3, COUNT, K, kind)
    plan.close()


def test_sample_and_encrypt_at_16384(hx, ctx, dev, orc):
    n, kind, n_limbs = 16384, "seal", 2
    lm = limbs(orc, kind, n)
    plan = make_plan(hx, ctx, orc, n, lm.qs)
    for what in (sm.UNIFORM, sm.CBD21):
        check_sample(hx, ctx, dev, plan, lm, what, SEEDS[0], 3, (1 << 40) - 2, 2, n_limbs, kind)
    s = secret_of(lm, SEEDS[0], n_limbs)
    pt = np.stack([orc.splitmix(n, 41 + i, lm.qs[i]) for i in range(n_limbs)])
    out = minus_one(dev, 2 * 2 * n_limbs * n)
    plan.rlwe_encrypt(out, up(hx, dev, s), 2, n_limbs, pt=up(hx, dev, pt), pt_batch=1, seed=SEEDS[1], stream=9, first=6)
    ctx.sync()
    want = [sm.encrypt(lm, SEEDS[1], 9, 6 + b, n_limbs, s, pt) for b in range(2)]
    assert_instances(hx.to_u64(out), want, 2, ("component",) + NAMES, (2, n_limbs, n), "encrypt at 16384")
    plan.close()


def test_addressing_is_independent_of_the_split(hx, ctx, dev, orc):
    """count 7 in one call = 3 + 4 with `first` advanced; UNIFORM at two limbs = the first two of K"""
    import torch
    n, kind, n_limbs = 1024, "seal", 3
    lm = limbs(orc, kind, n)
    plan = make_plan(hx, ctx, orc, n, lm.qs)
    s = up(hx, dev, secret_of(lm, SEEDS[0], K))
    per = n_limbs * n
    for what in (sm.UNIFORM, sm.TERNARY, sm.CBD21):
        whole, parts = minus_one(dev, 7 * per), minus_one(dev, 7 * per)
        plan.sample(whole, what, 7, n_limbs, seed=SEEDS[0], stream=4, first=11)
        plan.sample(parts[:3 * per], what, 3, n_limbs, seed=SEEDS[0], stream=4, first=11)
        plan.sample(parts[3 * per:], what, 4, n_limbs, seed=SEEDS[0], stream=4, first=14)
        ctx.sync()
        assert torch.equal(whole, parts), f"kind {what}: 7 != 3 + 4"
    whole, parts = minus_one(dev, 7 * 2 * per), minus_one(dev, 7 * 2 * per)
    plan.rlwe_encrypt(whole, s, 7, n_limbs, seed=SEEDS[0], stream=4, first=11)
    plan.rlwe_encrypt(parts[:3 * 2 * per], s, 3, n_limbs, seed=SEEDS[0], stream=4, first=11)
    plan.rlwe_encrypt(parts[3 * 2 * per:], s, 4, n_limbs, seed=SEEDS[0], stream=4, first=14)
    two, full = minus_one(dev, COUNT * 2 * n), minus_one(dev, COUNT * K * n)
    plan.sample(two, sm.UNIFORM, COUNT, 2, seed=SEEDS[1], stream=1, first=2)
    plan.sample(full, sm.UNIFORM, COUNT, K, seed=SEEDS[1], stream=1, first=2)
    ctx.sync()
    assert torch.equal(whole, parts), "encrypt: 7 != 3 + 4"
    assert torch.equal(two.view(COUNT, 2, n), full.view(COUNT, K, n)[:, :2]), "the limbs of a lower level are a prefix"
    plan.close()


def test_scratch_chunk_seam(hx, ctx, dev, orc):
    """n = 1024, n_limbs = 1: 4098 instances = the encode scratch's chunk (4096) + 2 in one call, against two calls split at an odd
    boundary; instances 0, chunk - 1, chunk and chunk + 1 against the model"""
    import torch
    n, kind, chunk = 1024, "seal", 4096
    count, cut = chunk + 2, 1237
    lm = limbs(orc, kind, n)
    plan = make_plan(hx, ctx, orc, n, lm.qs)
    look = (0, chunk - 1, chunk, chunk + 1)
    seed, stream, first = SEEDS[1], 6, 1000
    for what in (sm.TERNARY, sm.CBD21, sm.UNIFORM):
        whole, parts = minus_one(dev, count * n), minus_one(dev, count * n)
        plan.sample(whole, what, count, 1, seed=seed, stream=stream, first=first)
        plan.sample(parts[:cut * n], what, cut, 1, seed=seed, stream=stream, first=first)
        plan.sample(parts[cut * n:], what, count - cut, 1, seed=seed, stream=stream, first=first + cut)
        ctx.sync()
        assert torch.equal(whole, parts), f"kind {what}: one call != two calls"
        got = hx.to_u64(whole.view(count, n)[list(look)])
        want = [sm.sample(lm, what, seed, stream, first + b, 1, 1)[0] for b in look]
        assert_instances(got, want, len(look), NAMES, (1, n), f"kind {what} around the chunk seam")
    s = secret_of(lm, SEEDS[0], 1)
    pts = np.stack([orc.splitmix(n, 500 + b, lm.qs[0]) for b in range(4)])
    d_pt = up(hx, dev, pts)[(torch.arange(count, device=dev) % 4)[:, None] * n + torch.arange(n, device=dev)].reshape(-1).contiguous()
    d_s = up(hx, dev, s)
    whole, parts = minus_one(dev, count * 2 * n), minus_one(dev, count * 2 * n)
    plan.rlwe_encrypt(whole, d_s, count, 1, pt=d_pt, pt_batch=count, seed=seed, stream=stream, first=first)
    plan.rlwe_encrypt(parts[:cut * 2 * n], d_s, cut, 1, pt=d_pt[:cut * n], pt_batch=cut, seed=seed, stream=stream, first=first)
    plan.rlwe_encrypt(parts[cut * 2 * n:], d_s, count - cut, 1, pt=d_pt[cut * n:], pt_batch=count - cut, seed=seed, stream=stream, first=first + cut)
    ctx.sync()
    assert torch.equal(whole, parts), "encrypt: one call != two calls"
    got = hx.to_u64(whole.view(count, 2 * n)[list(look)])
    want = [sm.encrypt(lm, seed, stream, first + b, 1, s, pts[b % 4][None]) for b in look]
    assert_instances(got, want, len(look), ("component",) + NAMES, (2, 1, n), "encrypt around the chunk seam")
    plan.close()


def compose_encrypt(hx, plan, dev, lm, d_s, d_pt, pt_batch, seed, stream, first, count, n_limbs):
    """the composition hexl_rlwe_encrypt fuses: two samples, a * s by hexl_multiply_plain, e - a s (+ pt) by hexl_ct_lincomb"""
    import torch
    n = lm.n
    a, e, prod, c0 = (minus_one(dev, count * n_limbs * n) for _ in range(4))
    plan.sample(a, sm.UNIFORM, count, n_limbs, seed=seed, stream=stream, first=first)
    plan.sample(e, sm.CBD21, count, n_limbs, seed=seed, stream=stream, first=first)
    plan.multiply_plain(prod, a, d_s, count, 1, n_limbs, 1)
    plan.ct_lincomb(c0, [e, prod], count, 1, n_limbs, weights=[[1] * n_limbs, [q - 1 for q in lm.qs[:n_limbs]]], pt=d_pt, pt_batch=pt_batch)
    return torch.stack([c0.view(count, n_limbs, n), a.view(count, n_limbs, n)], dim=1).reshape(-1)


@pytest.mark.parametrize("kind", KINDS)
def test_encrypt_is_the_model_and_the_composition(hx, ctx, dev, orc, kind):
    """d_pt NULL, pt_batch 1 and count; n_limbs 1, 3 (a secret of K rows) and K; plaintexts of uniform and of extreme words"""
    import torch
    n = 1024
    lm = limbs(orc, kind, n)
    plan = make_plan(hx, ctx, orc, n, lm.qs)
    s = secret_of(lm, SEEDS[1], K)
    d_s = up(hx, dev, s)
    uni = np.array([[orc.splitmix(n, 300 + 7 * b + i, lm.qs[i]) for i in range(K)] for b in range(COUNT)])
    ext = np.array([extreme_ciphertext(lm_case(lm), b, 1, limbs=K, salt=2).reshape(K, n) for b in range(COUNT)])
    c = 0
    for n_limbs in (1, 3, K):
        for mode in ("null", "one", "each"):
            pts = (uni, ext)[c % 2][:, :n_limbs]
            seed, stream, first = SEEDS[c % 2], STREAMS[(c // 2) % 2] + c, FIRSTS[c % 3]
            c += 1
            host_pt = None if mode == "null" else np.ascontiguousarray(pts[:1] if mode == "one" else pts)
            d_pt = None if host_pt is None else up(hx, dev, host_pt)
            pt_batch = COUNT if mode == "each" else 1
            out = minus_one(dev, COUNT * 2 * n_limbs * n)
            plan.rlwe_encrypt(out, d_s, COUNT, n_limbs, pt=d_pt, pt_batch=pt_batch, seed=seed, stream=stream, first=first)
            ctx.sync()
            want = [sm.encrypt(lm, seed, stream, first + b, n_limbs, s, None if host_pt is None else host_pt[b if mode == "each" else 0])
                    for b in range(COUNT)]
            label = f"{kind}: encrypt n_limbs={n_limbs} pt={mode} first={first}"
            assert_instances(hx.to_u64(out), want, COUNT, ("component",) + NAMES, (2, n_limbs, n), label)
            composed = compose_encrypt(hx, plan, dev, lm, d_s, d_pt, pt_batch, seed, stream, first, COUNT, n_limbs)
            ctx.sync()
            assert torch.equal(out, composed), f"{label}: not the composition"
            assert np.array_equal(hx.to_u64(d_s), s.reshape(-1)), f"{label}: the secret was written"
    plan.close()


class lm_case:
    """what ks_util.extreme_ciphertext reads of a case"""

    def __init__(self, lm):
        self.n, self.moduli, self.L = lm.n, lm.qs, len(lm.qs)


@pytest.mark.parametrize("kind", KINDS)
def test_decrypt_is_the_model_on_extreme_words(hx, ctx, dev, orc, kind):
    n = 1024
    lm = limbs(orc, kind, n)
    plan = make_plan(hx, ctx, orc, n, lm.qs)
    tern = secret_of(lm, SEEDS[0], K)
    ext_s = np.stack([extreme_ciphertext(lm_case(lm), 1, 1, limbs=K, salt=4).reshape(K, n)[i] for i in range(K)])
    for c, (ncomp, n_limbs) in enumerate([(2, 1), (3, 1), (2, 3), (3, 3), (2, K), (3, K)]):
        s = (tern, ext_s)[c % 2]
        cts = [extreme_ciphertext(lm_case(lm), b, ncomp, limbs=n_limbs, salt=c) for b in range(COUNT)]
        out = minus_one(dev, COUNT * n_limbs * n)
        plan.rlwe_decrypt(out, up(hx, dev, np.stack(cts)), up(hx, dev, s), COUNT, ncomp, n_limbs)
        ctx.sync()
        want = [sm.decrypt(lm.qs, n, ct, s, ncomp, n_limbs) for ct in cts]
        assert_instances(hx.to_u64(out), want, COUNT, NAMES, (n_limbs, n), f"{kind}: decrypt components={ncomp} n_limbs={n_limbs}")
    plan.close()


@pytest.mark.parametrize("kind", ["strict", "seal"])
def test_decrypt_of_encrypt_leaves_exactly_the_error(hx, ctx, dev, orc, kind):
    """hexl_rns_ntt_inv(decrypt(encrypt(pt)) - pt) is the model's CBD21 polynomial, the same integers in every limb"""
    n = 1024
    lm = limbs(orc, kind, n)
    plan = make_plan(hx, ctx, orc, n, lm.qs)
    d_s = up(hx, dev, secret_of(lm, SEEDS[0], K))
    pt = np.array([[orc.splitmix(n, 800 + 7 * b + i, lm.qs[i]) for i in range(K)] for b in range(COUNT)])
    d_pt = up(hx, dev, pt)
    seed, stream, first = SEEDS[1], 12, (1 << 40) - 3
    ct, dec, diff = minus_one(dev, COUNT * 2 * K * n), minus_one(dev, COUNT * K * n), minus_one(dev, COUNT * K * n)
    plan.rlwe_encrypt(ct, d_s, COUNT, K, pt=d_pt, pt_batch=COUNT, seed=seed, stream=stream, first=first)
    plan.rlwe_decrypt(dec, ct, d_s, COUNT, 2, K)
    plan.ct_lincomb(diff, [dec, d_pt], COUNT, 1, K, weights=[[1] * K, [q - 1 for q in lm.qs]])
    plan.rns_ntt_inv(diff, diff, COUNT, K)
    ctx.sync()
    want = []
    for b in range(COUNT):
        ev = sm.small(seed, stream, sm.CBD21, first + b, n)
        assert np.abs(ev).max() <= 21
        want.append(np.stack([np.array([int(v) % q for v in ev], dtype=np.uint64) for q in lm.qs]))
    assert_instances(hx.to_u64(diff), want, COUNT, NAMES, (K, n), f"{kind}: the error of a fresh ciphertext")
    plan.close()


def test_refusals_write_nothing(hx, ctx, dev, orc):
    import torch
    n, n_limbs = 1024, 3
    lm = limbs(orc, "seal", n)
    plan = make_plan(hx, ctx, orc, n, lm.qs)
    per = n_limbs * n
    buf = minus_one(dev, COUNT * 3 * per + n)
    out, ct_out = buf[:COUNT * per], buf[:COUNT * 2 * per]
    s = torch.zeros(K * n, dtype=torch.int64, device=dev)
    pt = torch.zeros(COUNT * per, dtype=torch.int64, device=dev)
    ct = torch.zeros(COUNT * 3 * per, dtype=torch.int64, device=dev)
    seed = SEEDS[0]
    top = 1 << 40
    bad = [
        lambda: plan.sample(out, 0, COUNT, n_limbs, seed=seed),                                             # unknown kinds
        lambda: plan.sample(out, 4, COUNT, n_limbs, seed=seed),
        lambda: plan.sample(out, -1, COUNT, n_limbs, seed=seed),
        lambda: plan.sample(out, sm.UNIFORM, COUNT, 0, seed=seed),                                          # 1 <= n_limbs <= K
        lambda: plan.sample(out, sm.CBD21, COUNT, K + 1, seed=seed),
        lambda: plan.sample(out, sm.UNIFORM, COUNT, n_limbs, seed=seed, first=top - COUNT + 1),             # first + count > 2^40
        lambda: plan.sample(out, sm.TERNARY, 1, n_limbs, seed=seed, first=top),
        lambda: plan.sample(out, sm.UNIFORM, 0, n_limbs, seed=seed, first=top + 1),
        lambda: plan.sample(out, sm.UNIFORM, 1, n_limbs, seed=seed, first=(1 << 64) - 1),
        lambda: plan.sample(out, sm.UNIFORM, 1 << 40, n_limbs, seed=seed),                                  # a grid that overflows
        lambda: plan.rlwe_encrypt(ct_out, s, COUNT, 0, seed=seed),
        lambda: plan.rlwe_encrypt(ct_out, s, COUNT, K + 1, seed=seed),
        lambda: plan.rlwe_encrypt(ct_out, s, COUNT, n_limbs, pt=pt, pt_batch=2, seed=seed),                 # pt_batch is 1 or count
        lambda: plan.rlwe_encrypt(ct_out, s, COUNT, n_limbs, pt=pt, pt_batch=0, seed=seed),
        lambda: plan.rlwe_encrypt(ct_out, s, COUNT, n_limbs, seed=seed, first=top - 2),
        lambda: plan.rlwe_encrypt(ct_out, buf[COUNT * 2 * per - 8:COUNT * 2 * per - 8 + per], COUNT, n_limbs, seed=seed),   # out over the secret
        lambda: plan.rlwe_encrypt(ct_out, s, COUNT, n_limbs, pt=buf[n:n + per], pt_batch=1, seed=seed),      # out over the plaintext
        lambda: plan.rlwe_encrypt(ct_out, s, COUNT, n_limbs, pt=ct_out[:COUNT * per], pt_batch=COUNT, seed=seed),
        lambda: plan.rlwe_decrypt(out, ct, s, COUNT, 1, n_limbs),                                           # n_components is 2 or 3
        lambda: plan.rlwe_decrypt(out, ct, s, COUNT, 4, n_limbs),
        lambda: plan.rlwe_decrypt(out, ct, s, COUNT, 2, 0),
        lambda: plan.rlwe_decrypt(out, ct, s, COUNT, 2, K + 1),
        lambda: plan.rlwe_decrypt(out, buf[:COUNT * 2 * per], s, COUNT, 2, n_limbs),                        # in place is not offered
        lambda: plan.rlwe_decrypt(out, buf[n:n + COUNT * 3 * per], s, COUNT, 3, n_limbs),
        lambda: plan.rlwe_decrypt(out, ct, buf[COUNT * per - 8:COUNT * per - 8 + per], COUNT, 2, n_limbs),  # out over the secret
    ]
    for k, f in enumerate(bad):
        with pytest.raises(hx.HexlError, match="status -1"):
            f()
        ctx.sync()
        assert bool((buf == -1).all()), f"refusal {k} wrote to the output"
        assert not bool(s.any()) and not bool(pt.any()) and not bool(ct.any()), f"refusal {k} wrote to an input"
    case = KsCase(orc, n, 2, 3, seed=1, bits=55)                   # a plan on the integer kernels (moduli >= 2^52): out of scope
    integer = hx.KeySwitchPlan(ctx, n, 2, 3, 3, 2, case.moduli, case.modswitch)
    assert integer.tiers()[0][0] == -1
    for f in (lambda: integer.sample(out, sm.UNIFORM, COUNT, 2, seed=seed), lambda: integer.rlwe_encrypt(ct_out, s, COUNT, 2, seed=seed),
              lambda: integer.rlwe_decrypt(out, ct, s, COUNT, 2, 2)):
        with pytest.raises(hx.HexlError, match="status -1"):
            f()
    ctx.sync()
    assert bool((buf == -1).all())
    integer.close()
    # accepted: nothing to do; pt_batch ignored without a plaintext; adjacent buffers
    plan.sample(out, sm.CBD21, 0, n_limbs, seed=seed, first=top)
    plan.rlwe_encrypt(ct_out, s, 0, n_limbs, pt=pt, pt_batch=0, seed=seed)
    plan.rlwe_decrypt(out, ct, s, 0, 3, n_limbs)
    ctx.sync()
    assert bool((buf == -1).all())
    plan.rlwe_encrypt(ct_out, s, COUNT, n_limbs, pt_batch=7, seed=seed)
    plan.rlwe_decrypt(buf[COUNT * 2 * per:COUNT * 3 * per], ct_out, s, COUNT, 2, n_limbs)
    ctx.sync()
    assert bool((buf[COUNT * 3 * per:] == -1).all()) and not bool((buf[:COUNT * 3 * per] == -1).any())
    plan.close()


def test_encrypt_and_decrypt_are_ordered_on_a_caller_stream(hx, dev, orc, fill, closing):
    """behind a filler on a side stream set by hexl_ctx_set_stream: the secret and the plaintext are poison until copies queued on that
    stream replace them, the outputs are cloned on that stream, and the stream is the only thing waited for (test_gpu_streams.py, part A)"""
    n, kind, n_limbs = 1024, "seal", 3
    side, s = side_context(hx, closing)
    lm = limbs(orc, kind, n)
    plan = make_plan(hx, side, orc, n, lm.qs)
    closing.append(plan)
    sec = secret_of(lm, SEEDS[0], n_limbs)
    pts = np.array([[orc.splitmix(n, 600 + 7 * b + i, lm.qs[i]) for i in range(n_limbs)] for b in range(COUNT)])
    d_s, real_s = dev_pair(hx, dev, [sec])
    d_pt, real_pt = dev_pair(hx, dev, list(pts), COUNT)
    ct = minus_one(dev, COUNT * 2 * n_limbs * n)
    dec = minus_one(dev, COUNT * n_limbs * n)
    seed, stream, first = SEEDS[1], 21, 40
    want_ct = [sm.encrypt(lm, seed, stream, first + b, n_limbs, sec, pts[b]) for b in range(COUNT)]
    want_dec = [sm.decrypt(lm.qs, n, w, sec, 2, n_limbs) for w in want_ct]
    label = "hexl_rlwe_encrypt -> hexl_rlwe_decrypt on a side stream"

    def call():
        plan.rlwe_encrypt(ct, d_s, COUNT, n_limbs, pt=d_pt, pt_batch=COUNT, seed=seed, stream=stream, first=first)
        plan.rlwe_decrypt(dec, ct, d_s, COUNT, 2, n_limbs)

    def check(c):
        assert_every(hx, c[0], want_ct, COUNT, ("component",) + NAMES, (2, n_limbs, n), label)
        assert_every(hx, c[1], want_dec, COUNT, NAMES, (n_limbs, n), label)

    first_then_warm(Op(label, [(d_s, real_s), (d_pt, real_pt)], [ct, dec], [ct, dec], call, check), s, fill)


def test_square_end_to_end_on_the_device(hx, ctx, dev, orc):
    """z -> z^2 with every key and every ciphertext made on the device, n = 1024, L = 3, K = 4, four 40-bit primes, scale D = q_2:
    secret = hexl_sample(TERNARY) at K limbs; s^2 = hexl_multiply_plain; pt[d] = [i == d] (P mod q_i) s^2 by L hexl_ct_lincomb calls with
    per-limb weights; ONE key-shaped hexl_rlwe_encrypt; the key downloaded once for hexl_ks_set_keys; then hexl_ckks_encode ->
    hexl_rlwe_encrypt -> hexl_multiply_relinearize -> hexl_rescale -> hexl_rlwe_decrypt (secret of K rows at two limbs) -> hexl_ckks_decode.

    The bound, derived before any run. Units: one integer step of a coefficient; an error of at most h in every coefficient reaches a slot
    with at most n h (a slot is sum_j e_j zeta^(j 5^k)). ||s||_1 <= n. F = 16 log2(n) 2^-53 is the FFT bound of DESIGN.md 4.6.4.
      encode      slots D z + eps, |eps| <= E = n/2 + sqrt(n) F D (rounding 1/2 per coefficient, the FFT's 2-norm bound; |z| <= 1)
      fresh noise |e_j| <= 21 (CBD21) -> at most 21 n in a slot: the ciphertext decrypts to D z + d, |d| <= N1 = E + 21 n
      product     (D z + d)^2 = D^2 z^2 + 2 D z d + d^2, exactly, under (1, s, s^2): error 2 D N1 + N1^2 before the rescale
      key switch  c2 s^2 is replaced by (sum_d [c2]_(q_d) key_d) / P rounded: the key's errors e_d (|.| <= 21) meet digits below q_d, so a
                  coefficient of sum_d [c2]_d e_d is at most L n 21 max(q_d), divided by P; the rounding of the division is 1/2 in
                  component 0 and 1/2 in component 1, which meets s: (1 + n)/2. Per coefficient L n 21 max(q_d)/P + (n + 1)/2, times n
                  in a slot: KS
      rescale     the same rounding, (n + 1)/2 per coefficient -> n (n + 1)/2 in a slot, AFTER the division by q_2 = D
    Slot error of the result at scale D: (2 D N1 + N1^2 + KS) / D + n (n + 1) / 2; divided by D by decode, whose FFT adds at most
    F ||result||_2; the numpy reference is good to 2^-50. With n = 1024 and D ~ 2^40: 2 N1 / D ~ 4e-8, KS / D^2 ~ 1e-16,
    n (n + 1) / (2 D) ~ 4.8e-7: about 5.2e-7 in all."""
    import torch
    n, Kc, L, count = 1024, 4, 3, 2
    qs = [int(q) for q in orc.primes(Kc, 40, n)]
    P = qs[Kc - 1]
    case = KsCase(orc, n, L, Kc, seed=5, moduli=qs)
    plan = hx.KeySwitchPlan(ctx, n, L, Kc, Kc, 2, case.moduli, case.modswitch)
    seed = SEEDS[1]
    # 1. the secret, at K limbs
    s = minus_one(dev, Kc * n)
    plan.sample(s, sm.TERNARY, 1, Kc, seed=seed, stream=1)
    # 2. s^2   3. the L plaintexts of the relinearisation key
    s2 = minus_one(dev, Kc * n)
    plan.multiply_plain(s2, s, s, 1, 1, Kc, 1)
    pts = minus_one(dev, L * Kc * n)
    for d in range(L):
        plan.ct_lincomb(pts[d * Kc * n:(d + 1) * Kc * n], [s2], 1, 1, Kc, weights=[[P % qs[i] if i == d else 0 for i in range(Kc)]])
    # 4. one key-shaped encryption   5. one download
    key = minus_one(dev, L * 2 * Kc * n)
    plan.rlwe_encrypt(key, s, L, Kc, pt=pts, pt_batch=L, seed=seed, stream=2)
    ctx.sync()
    plan.set_keys(list(hx.to_u64(key).reshape(L, 2 * Kc * n)))
    # 6. encode, encrypt, square, rescale, decrypt, decode
    D = float(qs[2])
    assert int(D) == qs[2]
    rng = np.random.default_rng(23)
    z = np.sqrt(rng.random((count, n // 2))) * np.exp(2j * np.pi * rng.random((count, n // 2)))            # uniform in the unit disc
    z[:, 0], z[:, 1], z[:, 2] = 1.0, -1.0, 1j
    assert np.abs(z).max() <= 1.0 + 1e-15
    d_z = torch.from_numpy(np.ascontiguousarray(np.stack([z.real, z.imag], axis=-1))).to(dev)
    enc = minus_one(dev, count * L * n)
    plan.ckks_encode(enc, d_z, count, L, D)
    ct = minus_one(dev, count * 2 * L * n)
    plan.rlwe_encrypt(ct, s, count, L, pt=enc, pt_batch=count, seed=seed, stream=3)
    sq = minus_one(dev, count * 2 * L * n)
    plan.multiply_relinearize(sq, ct, ct, count)
    sq2 = minus_one(dev, count * 2 * 2 * n)
    plan.rescale(sq2, sq, count, L, 2)
    dec = minus_one(dev, count * 2 * n)
    plan.rlwe_decrypt(dec, sq2, s, count, 2, 2)
    d_out = torch.full((count, n // 2, 2), float("nan"), dtype=torch.float64, device=dev)
    plan.ckks_decode(d_out, dec, count, 2, D)
    ctx.sync()
    assert plan.range_check()
    o = d_out.cpu().numpy()
    got, want = o[..., 0] + 1j * o[..., 1], z * z
    # the ciphertext hides the plaintext: component 0 alone decodes to noise of the modulus' size, not to z
    F = 16 * math.log2(n) * 2.0 ** -53
    E = n / 2 + math.sqrt(n) * F * D
    N1 = E + 21 * n
    KS = n * (L * n * 21 * max(qs[:L]) / P + (n + 1) / 2)
    for b in range(count):
        tol = ((2 * D * N1 + N1 * N1 + KS) / D + n * (n + 1) / 2) / D + F * float(np.linalg.norm(want[b])) + 2.0 ** -50
        err = float(np.abs(got[b] - want[b]).max())
        print(f"[rlwe] z^2 end to end on the device, instance {b}: max |error| = {err:.3e}, bound {tol:.3e}")
        assert err <= tol, f"instance {b}: {err:.3e} > {tol:.3e}"
    plan.close()
