"""GPU: hexl_pk_encrypt bit-exact against the host model (tests/pk_model.py: Python integers on sample_model's streams and the oracle's
transforms) AND against its normative four-call composition on the device (hexl_sample x 2, hexl_multiply_plain on a replicated key,
hexl_ct_lincomb), every word of every instance; the first wrong word is named. Ring sizes 1024 (one 1024-word piece per polynomial),
2048 (two) and one case at 16384; the chains strict / period3_top / period12 / seal at K = 5, as test_gpu_rlwe.py builds them. Outputs
are pre-filled with -1 and followed by a guard row."""
import itertools
import math

import numpy as np
import pytest

import pk_model as pm
import sample_model as sm
from ks_util import KsCase, extreme_ciphertext
from rns_model import assert_instances
from test_gpu_rlwe import K, SEEDS, STREAMS, limbs, lm_case, make_plan, minus_one, secret_of, up
from test_gpu_streams import Op, assert_every, closing, dev_pair, fill, first_then_warm, side_context  # noqa: F401  (closing, fill: fixtures)

pytestmark = pytest.mark.gpu

COUNT = 3
KINDS = ["strict", "period3_top", "period12", "seal"]
FIRSTS = [0, 5, (1 << 39) - 3]
NAMES = ("component", "limb", "coefficient")
PK_SEED = bytes((97 * k + 5) & 0xFF for k in range(32))


def model_key(lm, rows=K, c=0):
    """(pk0, pk1) = (e - a s, a) at `rows` limbs from the model, and the secret's words"""
    s = secret_of(lm, PK_SEED, rows)
    return pm.public_key(lm, PK_SEED, 3, c, rows, s), s


def compose(hx, plan, dev, lm, d_pk, pk_limbs, d_pt, pt_batch, seed, stream, first, count, n_limbs):
    """the normative definition: U, E, T = (replicated key) . U, out = T + E (+ pt on component 0)"""
    n = lm.n
    per = n_limbs * n
    U, E, T, out = minus_one(dev, count * per), minus_one(dev, 2 * count * per), minus_one(dev, 2 * count * per), minus_one(dev, 2 * count * per)
    plan.sample(U, sm.TERNARY, count, n_limbs, seed=seed, stream=stream, first=first)
    plan.sample(E, sm.CBD21, 2 * count, n_limbs, seed=seed, stream=stream, first=2 * first)
    rep = d_pk.view(2, pk_limbs, n)[:, :n_limbs].unsqueeze(0).expand(count, 2, n_limbs, n).contiguous().view(-1)
    plan.multiply_plain(T, rep, U, count, 2, n_limbs, count)
    plan.ct_lincomb(out, [T, E], count, 2, n_limbs, pt=d_pt, pt_batch=pt_batch)
    return out


def run_and_check(hx, ctx, dev, plan, lm, pk, pk_limbs, host_pt, mode, seed, stream, first, count, n_limbs, label, composed=True):
    """one call into a -1 buffer with a guard row behind it, against the model and (composed) the four-call composition"""
    import torch
    n = lm.n
    words = count * 2 * n_limbs * n
    d_pk = up(hx, dev, pk[:, :pk_limbs])
    d_pt = None if host_pt is None else up(hx, dev, host_pt)
    pt_batch = count if mode == "each" else 1
    buf = minus_one(dev, words + n)
    plan.pk_encrypt(buf[:words], d_pk, count, n_limbs, pk_limbs=pk_limbs, pt=d_pt, pt_batch=pt_batch, seed=seed, stream=stream, first=first)
    ctx.sync()
    got = hx.to_u64(buf)
    want = [pm.pk_encrypt(lm, seed, stream, first + b, n_limbs, pk, None if host_pt is None else host_pt[b if mode == "each" else 0])
            for b in range(count)]
    assert_instances(got[:words], want, count, NAMES, (2, n_limbs, n), label)
    assert (got[words:] == np.uint64(0xFFFFFFFFFFFFFFFF)).all(), f"{label}: wrote behind the output"
    assert np.array_equal(hx.to_u64(d_pk), np.ascontiguousarray(pk[:, :pk_limbs]).reshape(-1)), f"{label}: the key was written"
    if composed:
        ref = compose(hx, plan, dev, lm, d_pk, pk_limbs, d_pt, pt_batch, seed, stream, first, count, n_limbs)
        ctx.sync()
        assert torch.equal(buf[:words], ref), f"{label}: not the composition"


@pytest.mark.parametrize("kind", KINDS)
def test_bit_exact_matrix(hx, ctx, dev, orc, kind):
    """n = 1024, K = 5: n_limbs {1, 3, K} x pk_limbs {n_limbs, K} x pt {NULL, one, per instance} x first {0, 5, 2^39 - 3} x two seeds x
    two streams, count 3; uniform / extreme plaintext words and a real / an extreme-word key alternate through the 180 calls"""
    n = 1024
    lm = limbs(orc, kind, n)
    plan = make_plan(hx, ctx, orc, n, lm.qs)
    real_key, _ = model_key(lm)
    ext_key = extreme_ciphertext(lm_case(lm), 1, 2, limbs=K, salt=7).reshape(2, K, n)
    uni = np.array([[orc.splitmix(n, 300 + 7 * b + i, lm.qs[i]) for i in range(K)] for b in range(COUNT)])
    ext = np.array([extreme_ciphertext(lm_case(lm), b, 1, limbs=K, salt=2).reshape(K, n) for b in range(COUNT)])
    combos = list(itertools.product(FIRSTS, SEEDS, STREAMS))
    c = 0
    for n_limbs in (1, 3, K):
        for pk_limbs in sorted({n_limbs, K}):
            for mode in ("null", "one", "each"):
                for first, seed, stream in combos:
                    pts = (uni, ext)[c % 3 == 1][:, :n_limbs]     # periods 3 and 5 against the 12 combinations: every first, seed and
                    pk = (real_key, ext_key)[(c % 5) % 2]         # stream meets both families of words and both keys
                    c += 1
                    host_pt = None if mode == "null" else np.ascontiguousarray(pts[:1] if mode == "one" else pts)
                    label = f"{kind}: pk_encrypt n_limbs={n_limbs} pk_limbs={pk_limbs} pt={mode} first={first} stream={stream:#x}"
                    run_and_check(hx, ctx, dev, plan, lm, pk, pk_limbs, host_pt, mode, seed, stream, first, COUNT, n_limbs, label)
    assert c == 15 * len(combos)
    plan.close()


@pytest.mark.parametrize("kind", ["strict", "seal"])
def test_two_pieces_per_polynomial(hx, ctx, dev, orc, kind):
    """n = 2048: two 1024-word pieces per polynomial, n_limbs = 2, both key strides"""
    n, n_limbs = 2048, 2
    lm = limbs(orc, kind, n)
    plan = make_plan(hx, ctx, orc, n, lm.qs)
    pk, _ = model_key(lm)
    pts = np.array([[orc.splitmix(n, 400 + 7 * b + i, lm.qs[i]) for i in range(n_limbs)] for b in range(COUNT)])
    run_and_check(hx, ctx, dev, plan, lm, pk, K, pts, "each", SEEDS[1], STREAMS[1], 5, COUNT, n_limbs, f"{kind}: n=2048 pk_limbs=K")
    run_and_check(hx, ctx, dev, plan, lm, pk, n_limbs, None, "null", SEEDS[0], 1, (1 << 39) - 3, COUNT, n_limbs, f"{kind}: n=2048 pk_limbs=2")
    plan.close()


def test_at_16384(hx, ctx, dev, orc):
    n, kind, n_limbs, count = 16384, "seal", 2, 2
    lm = limbs(orc, kind, n)
    plan = make_plan(hx, ctx, orc, n, lm.qs)
    pk, _ = model_key(lm, rows=3)
    pt = np.stack([orc.splitmix(n, 41 + i, lm.qs[i]) for i in range(n_limbs)])[None]
    run_and_check(hx, ctx, dev, plan, lm, pk, 3, pt, "one", SEEDS[1], 9, 6, count, n_limbs, "pk_encrypt at 16384")
    plan.close()


def test_scratch_chunk_seam(hx, ctx, dev, orc):
    """n = 1024, n_limbs = 1: 1367 instances = the call's chunk (floor(4096 / 3) = 1365) + 2 in one call, against the same range split
    at instance 700 into two calls; instances 0, chunk - 1, chunk and chunk + 1 against the model"""
    import torch
    n, kind, chunk = 1024, "seal", 1365
    count, cut = chunk + 2, 700
    lm = limbs(orc, kind, n)
    plan = make_plan(hx, ctx, orc, n, lm.qs)
    look = (0, chunk - 1, chunk, chunk + 1)
    seed, stream, first = SEEDS[1], 6, 1000
    pk, _ = model_key(lm, rows=1)
    d_pk = up(hx, dev, pk)
    pts = np.stack([orc.splitmix(n, 500 + b, lm.qs[0]) for b in range(4)])
    d_pt = up(hx, dev, pts)[(torch.arange(count, device=dev) % 4)[:, None] * n + torch.arange(n, device=dev)].reshape(-1).contiguous()
    whole, parts = minus_one(dev, count * 2 * n), minus_one(dev, count * 2 * n)
    plan.pk_encrypt(whole, d_pk, count, 1, pt=d_pt, pt_batch=count, seed=seed, stream=stream, first=first)
    plan.pk_encrypt(parts[:cut * 2 * n], d_pk, cut, 1, pt=d_pt[:cut * n], pt_batch=cut, seed=seed, stream=stream, first=first)
    plan.pk_encrypt(parts[cut * 2 * n:], d_pk, count - cut, 1, pt=d_pt[cut * n:], pt_batch=count - cut, seed=seed, stream=stream, first=first + cut)
    ctx.sync()
    assert torch.equal(whole, parts), "one call != two calls"
    got = hx.to_u64(whole.view(count, 2 * n)[list(look)])
    want = [pm.pk_encrypt(lm, seed, stream, first + b, 1, pk, pts[b % 4][None]) for b in look]
    assert_instances(got, want, len(look), NAMES, (2, 1, n), "pk_encrypt around the chunk seam")
    plan.close()


@pytest.mark.parametrize("kind", ["strict", "seal"])
def test_decrypt_leaves_exactly_the_model_noise(hx, ctx, dev, orc, kind):
    """hexl_rns_ntt_inv(decrypt(pk_encrypt(pt)) - pt) is the integer polynomial e_pk u + e0 + e1 s of the model, the same integers in
    every limb; secret and key are made on the device"""
    n = 1024
    lm = limbs(orc, kind, n)
    plan = make_plan(hx, ctx, orc, n, lm.qs)
    d_s, d_pk = minus_one(dev, K * n), minus_one(dev, 2 * K * n)
    plan.sample(d_s, sm.TERNARY, 1, K, seed=PK_SEED, stream=77, first=0)
    plan.gen_public_key(d_pk, d_s, seed=PK_SEED, stream=3, first=4)
    pt = np.array([[orc.splitmix(n, 800 + 7 * b + i, lm.qs[i]) for i in range(K)] for b in range(COUNT)])
    d_pt = up(hx, dev, pt)
    seed, stream, first = SEEDS[1], 12, (1 << 39) - 3
    ct, dec, diff = minus_one(dev, COUNT * 2 * K * n), minus_one(dev, COUNT * K * n), minus_one(dev, COUNT * K * n)
    plan.pk_encrypt(ct, d_pk, COUNT, K, pt=d_pt, pt_batch=COUNT, seed=seed, stream=stream, first=first)
    plan.rlwe_decrypt(dec, ct, d_s, COUNT, 2, K)
    plan.ct_lincomb(diff, [dec, d_pt], COUNT, 1, K, weights=[[1] * K, [q - 1 for q in lm.qs]])
    plan.rns_ntt_inv(diff, diff, COUNT, K)
    ctx.sync()
    s_int = sm.small(PK_SEED, 77, sm.TERNARY, 0, n)
    want = []
    for b in range(COUNT):
        ev = pm.noise(PK_SEED, 3, 4, s_int, seed, stream, first + b, n)
        assert 21 < np.abs(ev).max() <= (2 * n + 1) * 21
        want.append(np.stack([np.array([int(v) % q for v in ev], dtype=np.uint64) for q in lm.qs]))
    assert_instances(hx.to_u64(diff), want, COUNT, NAMES[1:], (K, n), f"{kind}: the noise of a fresh public-key ciphertext")
    plan.close()


def test_slots_end_to_end_on_the_device(hx, ctx, dev, orc):
    """Nothing but slots crosses the bus, n = 1024, three 40-bit primes, scale D = 2^40: secret = hexl_sample(TERNARY), the public key
    = gen_public_key (hexl_rlwe_encrypt of zero), hexl_ckks_encode -> hexl_pk_encrypt -> hexl_rlwe_decrypt -> hexl_ckks_decode.

    The bound, derived before any run. Units: one integer step of a coefficient; an error of at most h in every coefficient reaches a slot
    with at most n h (a slot is sum_j e_j zeta^(j 5^k)). F = 16 log2(n) 2^-53 is the FFT bound of DESIGN.md 4.6.4.
      encode   slots D z + eps, |eps| <= E = n/2 + sqrt(n) F D (rounding 1/2 per coefficient, the FFT's 2-norm bound; |z| <= 1)
      noise    c0 + c1 s = pt + e_pk u + e0 + e1 s: u and s ternary, the three errors CBD21 (|.| <= 21), so a coefficient of the noise
               is at most n 21 + 21 + n 21 = (2n + 1) 21, and a slot sees at most n (2n + 1) 21
    Slot error at scale D: E + n (2n + 1) 21, divided by D by decode, whose FFT adds at most F ||z||_2; the numpy comparison is good to
    2^-50. With n = 1024 and D = 2^40: n (2n + 1) 21 / D = 4.0e-5, E / D = 4.7e-10: about 4.0e-5 in all (the typical error is far
    smaller: the bound adds magnitudes, the noise adds in quadrature)."""
    import torch
    n, Kc, count = 1024, 3, 2
    qs = [int(q) for q in orc.primes(Kc, 40, n)]
    case = KsCase(orc, n, 2, Kc, seed=5, moduli=qs)
    plan = hx.KeySwitchPlan(ctx, n, 2, Kc, Kc, 2, case.moduli, case.modswitch)
    D = float(1 << 40)
    s, pk = minus_one(dev, Kc * n), minus_one(dev, 2 * Kc * n)
    plan.sample(s, sm.TERNARY, 1, Kc, seed=PK_SEED, stream=1)
    plan.gen_public_key(pk, s, seed=PK_SEED, stream=2)
    rng = np.random.default_rng(29)
    z = np.sqrt(rng.random((count, n // 2))) * np.exp(2j * np.pi * rng.random((count, n // 2)))            # uniform in the unit disc
    z[:, 0], z[:, 1], z[:, 2] = 1.0, -1.0, 1j
    assert np.abs(z).max() <= 1.0 + 1e-15
    d_z = torch.from_numpy(np.ascontiguousarray(np.stack([z.real, z.imag], axis=-1))).to(dev)
    enc, ct, dec = minus_one(dev, count * Kc * n), minus_one(dev, count * 2 * Kc * n), minus_one(dev, count * Kc * n)
    plan.ckks_encode(enc, d_z, count, Kc, D)
    plan.pk_encrypt(ct, pk, count, Kc, pt=enc, pt_batch=count, seed=SEEDS[1], stream=3)
    plan.rlwe_decrypt(dec, ct, s, count, 2, Kc)
    d_out = torch.full((count, n // 2, 2), float("nan"), dtype=torch.float64, device=dev)
    plan.ckks_decode(d_out, dec, count, Kc, D)
    ctx.sync()
    assert plan.range_check()
    o = d_out.cpu().numpy()
    got = o[..., 0] + 1j * o[..., 1]
    F = 16 * math.log2(n) * 2.0 ** -53
    E = n / 2 + math.sqrt(n) * F * D
    for b in range(count):
        tol = (E + n * (2 * n + 1) * 21) / D + F * float(np.linalg.norm(z[b])) + 2.0 ** -50
        err = float(np.abs(got[b] - z[b]).max())
        print(f"[pk_encrypt] slots end to end on the device, instance {b}: max |error| = {err:.3e}, bound {tol:.3e}")
        assert err <= tol, f"instance {b}: {err:.3e} > {tol:.3e}"
    plan.close()


def test_refusals_write_nothing(hx, ctx, dev, orc):
    import torch
    n, n_limbs = 1024, 3
    lm = limbs(orc, "seal", n)
    plan = make_plan(hx, ctx, orc, n, lm.qs)
    per = n_limbs * n
    words = COUNT * 2 * per
    buf = minus_one(dev, words + 2 * K * n)
    out = buf[:words]
    pk = torch.zeros(2 * K * n, dtype=torch.int64, device=dev)
    pt = torch.zeros(COUNT * per, dtype=torch.int64, device=dev)
    seed = SEEDS[0]
    top = 1 << 39
    call = lambda **kw: plan.pk_encrypt(**{**dict(out=out, pk=pk, count=COUNT, n_limbs=n_limbs, pk_limbs=K, seed=seed), **kw})
    bad = [
        lambda: call(n_limbs=0, pk_limbs=K),                                                  # 1 <= n_limbs <= K
        lambda: call(n_limbs=K + 1, pk_limbs=K + 1),
        lambda: call(pk_limbs=n_limbs - 1),                                                   # n_limbs <= pk_limbs <= K
        lambda: call(pk_limbs=0),
        lambda: call(pk_limbs=K + 1),
        lambda: call(pt=pt, pt_batch=2),                                                      # pt_batch is 1 or count
        lambda: call(pt=pt, pt_batch=0),
        lambda: call(first=top - COUNT + 1),                                                  # first + count > 2^39
        lambda: call(count=1, first=top),
        lambda: call(count=0, first=top + 1),
        lambda: call(count=1, first=(1 << 64) - 1),
        lambda: call(count=1 << 40),                                                          # a grid that overflows
        lambda: call(count=1 << 62),                                                          # a size that overflows
        lambda: call(pk=buf[words - 8:words - 8 + 2 * K * n]),                                # out over the head of the key
        lambda: call(out=buf[2 * K * n - 8:2 * K * n - 8 + words], pk=buf[:2 * K * n]),       # out over the last words of the key's FULL
                                                                                              # extent: a limb the call would not read
        lambda: call(pt=buf[n:n + per], pt_batch=1),                                          # out over the plaintext
        lambda: call(pt=out[:COUNT * per], pt_batch=COUNT),
    ]
    for k, f in enumerate(bad):
        with pytest.raises(hx.HexlError, match="status -1"):
            f()
        ctx.sync()
        assert bool((buf == -1).all()), f"refusal {k} wrote to the output"
        assert not bool(pk.any()) and not bool(pt.any()), f"refusal {k} wrote to an input"
    # null pointers, with and without instances
    lib, words8 = hx.lib(), hx.seed_words(seed)[0]
    for count in (COUNT, 0):
        for p_, o_, k_, s_ in ((None, out, pk, words8), (plan.h, None, pk, words8), (plan.h, out, None, words8), (plan.h, out, pk, None)):
            rc = lib.hexl_pk_encrypt(p_, None if o_ is None else o_.data_ptr(), None, 1, None if k_ is None else k_.data_ptr(), K, s_, 0, 0,
                                     count, n_limbs)
            assert rc == -1
    case = KsCase(orc, n, 2, 3, seed=1, bits=55)                   # a plan on the integer kernels (moduli >= 2^52): out of scope
    integer = hx.KeySwitchPlan(ctx, n, 2, 3, 3, 2, case.moduli, case.modswitch)
    assert integer.tiers()[0][0] == -1
    with pytest.raises(hx.HexlError, match="status -1"):
        integer.pk_encrypt(out, pk, COUNT, 2, pk_limbs=3, seed=seed)
    ctx.sync()
    assert bool((buf == -1).all())
    integer.close()
    # accepted: nothing to do; pt_batch ignored without a plaintext; the key adjacent to the output
    call(count=0, first=top)
    call(count=0, pt=pt, pt_batch=0)
    ctx.sync()
    assert bool((buf == -1).all())
    tail = buf[words:]
    tail.zero_()
    call(pk=tail, pt_batch=7, first=top - COUNT)
    ctx.sync()
    assert not bool((out == -1).any()) and not bool(tail.any())
    plan.close()


def test_ordered_on_a_caller_stream(hx, dev, orc, fill, closing):
    """behind a filler on a side stream set by hexl_ctx_set_stream: the key and the plaintext are poison until copies queued on that
    stream replace them, the output is cloned on that stream, and the stream is the only thing waited for (test_gpu_streams.py, part A)"""
    n, kind, n_limbs = 1024, "seal", 3
    side, s = side_context(hx, closing)
    lm = limbs(orc, kind, n)
    plan = make_plan(hx, side, orc, n, lm.qs)
    closing.append(plan)
    pk, _ = model_key(lm)
    pts = np.array([[orc.splitmix(n, 600 + 7 * b + i, lm.qs[i]) for i in range(n_limbs)] for b in range(COUNT)])
    d_pk, real_pk = dev_pair(hx, dev, [pk])
    d_pt, real_pt = dev_pair(hx, dev, list(pts), COUNT)
    ct = minus_one(dev, COUNT * 2 * n_limbs * n)
    seed, stream, first = SEEDS[1], 21, 40
    want = [pm.pk_encrypt(lm, seed, stream, first + b, n_limbs, pk, pts[b]) for b in range(COUNT)]
    label = "hexl_pk_encrypt on a side stream"

    def call():
        plan.pk_encrypt(ct, d_pk, COUNT, n_limbs, pk_limbs=K, pt=d_pt, pt_batch=COUNT, seed=seed, stream=stream, first=first)

    def check(c):
        assert_every(hx, c[0], want, COUNT, NAMES, (2, n_limbs, n), label)

    first_then_warm(Op(label, [(d_pk, real_pk), (d_pt, real_pt)], [ct], [ct], call, check), s, fill)
