"""GPU: hexl_rns_from_f64 / hexl_rns_to_f64 / hexl_ckks_encode / hexl_ckks_decode against the host model (tests/embed_model.py, pinned in
test_embed_model.py). Every comparison covers every instance of its launch; the instances cycle over two distinct ones. Word outputs
start as -1 and float outputs as NaN: the calls write them. The 2-norm bounds are derived, not measured: 0.5 sqrt(n) is
the rounding of n coefficients, 16 log2(n) 2^-53 is Higham's radix-2 bound (about 6.7 u per stage on correctly rounded twiddles) with a
factor of about two for the twist and the scale / (n/2) multiplies."""
import math

import numpy as np
import pytest

from ckks_model import Limbs
from embed_model import LD, as_double_slots, crt_lift, embed, embed_inverse, from_f64, ints_to_ld, ints_to_words
from rns_model import assert_instances, chain
from test_gpu_rotate_hoisted import cases_for, made, plans_for, uniform_ct  # noqa: F401  (made: a fixture)
from test_gpu_rns_ntt import make_plan

pytestmark = pytest.mark.gpu

RINGS = [1024, 2048, 16384, 32768]          # LOGE 4, LOGE 5, the full-LDS FFT, the split stage
KINDS = ["seal", "strict"]
K = 4
WORDS = ("limb", "coefficient")


def torch_():
    import torch
    return torch


@pytest.fixture(scope="module")
def setups(orc):
    """(n, kind) -> (moduli, Limbs), made once per module"""
    cache = {}

    def get(n, kind):
        if (n, kind) not in cache:
            qs = chain(orc, kind, K, n)
            cache[(n, kind)] = (qs, Limbs(orc, n, qs))
        return cache[(n, kind)]
    return get


def to_dev_f64(a, dev):
    return torch_().from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)


def tiled(distinct, count):
    return np.stack([distinct[c % len(distinct)] for c in range(count)])


def new_words(count, n_limbs, n, dev):
    return torch_().full((count * n_limbs * n,), -1, dtype=torch_().int64, device=dev)


def new_f64(shape, dev):
    return torch_().full(shape, float("nan"), dtype=torch_().float64, device=dev)


def value_families(qs, n, seed):
    """the host selftest's families spread over one polynomial: ties, the 2^52 / 2^53 / 2^62 edges, k q and k q +- 1, every binade"""
    rng = np.random.default_rng(seed)
    vals = []
    for v in (0.0, 0.5, 1.5, 2.5, 2.0 ** 52 - 0.5, 2.0 ** 53 + 2, 2.0 ** 62 - 1024):
        vals += [v, -v]
    for q in qs:
        for k in list(range(0, 6)) + [int(rng.integers(6, 1025)) for _ in range(6)] + [1024]:
            for d in (-1, 0, 1):
                v = k * q + d
                if int(float(v)) == v:
                    vals += [float(v), -float(v)]
    for e in range(-2, 62):
        m = rng.uniform(1.0, 2.0, 4) * 2.0 ** e
        vals += list(m[:2]) + list(-m[2:])
    vals = np.array(vals, dtype=np.float64)
    assert len(vals) <= n
    out = vals[np.arange(n) % len(vals)]
    return out[rng.permutation(n)]


def uniform_ints(n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(-(1 << 61) + 1, 1 << 61, n).astype(np.float64)


def exact_family(n, seed):
    """an integer polynomial with |a_j| <= 2^20 and its slots rounded to double: at scale 2^10 the device's unrounded coefficients are
    within about 2^-13 of the integers 2^10 a_j, so the rounding is unambiguous"""
    m = np.random.default_rng(seed).integers(-(1 << 20), (1 << 20) + 1, n)
    return m, as_double_slots(embed(m, n))


def rand_slots(n, seed):
    rng = np.random.default_rng(seed)
    z = rng.uniform(-1, 1, (n // 2, 2))
    return z


def as_complex(z):
    z = np.asarray(z)
    return z[..., 0].astype(LD) + 1j * z[..., 1].astype(LD)


def norm2(v):
    v = np.asarray(v)
    return float(np.sqrt((np.abs(v).astype(LD) ** 2).sum()))


def fft_bound(n):
    return 16 * math.log2(n) * 2.0 ** -53


# ---- rns_from_f64 ----
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", RINGS)
def test_from_f64_bit_exact(hx, ctx, dev, orc, setups, n, kind):
    qs, lm = setups(n, kind)
    plan = make_plan(hx, ctx, orc, n, qs)
    distinct = [value_families(qs, n, 11), uniform_ints(n, 12)]
    count = 4
    d_in = to_dev_f64(tiled(distinct, count), dev)
    for n_limbs in (1, 2, K):
        d_out = new_words(count, n_limbs, n, dev)
        plan.rns_from_f64(d_out, d_in, count, n_limbs)
        ctx.sync()
        want = [from_f64(lm, d, n_limbs) for d in distinct]
        assert_instances(hx.to_u64(d_out), want, count, WORDS, (n_limbs, n), f"{kind} n={n} n_limbs={n_limbs}")
    assert plan.range_check(), "in-range coefficients raised the range flag"
    plan.close()


def test_from_f64_flags_nan_and_two_to_the_63(hx, ctx, dev, orc, setups):
    n, n_limbs, count = 2048, 2, 4
    qs, lm = setups(n, "seal")
    plan = make_plan(hx, ctx, orc, n, qs)
    clean = uniform_ints(n, 21)
    dirty = clean.copy()
    dirty[5], dirty[n - 9] = float("nan"), 2.0 ** 63
    d_out = new_words(count, n_limbs, n, dev)
    plan.rns_from_f64(d_out, to_dev_f64(tiled([clean, dirty], count), dev), count, n_limbs)     # returns 0: no exception
    assert not plan.range_check(), "a NaN and 2^63 did not raise the range flag"
    got = hx.to_u64(d_out).reshape(count, -1)
    want = from_f64(lm, clean, n_limbs).reshape(-1)
    for c in (0, 2):                                               # the clean instances of the same launch are unaffected
        assert np.array_equal(got[c], want), f"clean instance {c} beside a flagged one"
    plan.rns_from_f64(d_out, to_dev_f64(tiled([clean], count), dev), count, n_limbs)
    assert plan.range_check(), "the next clean call raised the range flag"
    assert_instances(hx.to_u64(d_out), [want], count, WORDS, (n_limbs, n), "clean call after a flagged one")
    plan.close()


# ---- rns_to_f64 ----
def lift_inputs(qs, n, n_limbs, seed, small):
    """integer coefficients in (-Q/2, Q/2): below 2^53 of both signs (small) or up to Q/2; +-1, 0 and +-(Q - 1)/2 among them"""
    rng = np.random.default_rng(seed)
    Q = math.prod(qs[:n_limbs])
    top = min((Q - 1) // 2, (1 << 53) - 1) if small else (Q - 1) // 2
    bits = top.bit_length()
    x = []
    for j in range(n):
        b = int(rng.integers(1, bits + 1))                         # every magnitude
        v = int.from_bytes(rng.bytes((b + 7) // 8), "little") % (1 << b)
        x.append(min(v, top) * (1 if j & 1 else -1))
    x[:5] = [1, -1, 0, (Q - 1) // 2, -(Q - 1) // 2]
    if small:
        x[3], x[4] = top, -top
    return np.array(x, dtype=object)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", RINGS)
def test_to_f64_exact_below_2_53_and_within_2_50_above(hx, ctx, dev, orc, setups, n, kind):
    qs, lm = setups(n, kind)
    plan = make_plan(hx, ctx, orc, n, qs)
    count = 3
    for n_limbs, small in ((1, True), (2, True), (K, True), (K, False), (2, False)):
        xs = [lift_inputs(qs, n, n_limbs, 31 + s, small) for s in range(2)]
        words = tiled([ints_to_words(lm, x, n_limbs) for x in xs], count)
        d_out = new_f64((count, n), dev)
        plan.rns_to_f64(d_out, hx.as_i64(words.reshape(-1)).to(dev), count, n_limbs)
        ctx.sync()
        got = d_out.cpu().numpy()
        for c in range(count):
            x = xs[c % 2]
            assert np.isfinite(got[c]).all()
            g = [int(v) for v in got[c]]
            for j in range(n):
                exact = abs(x[j]) < 1 << 53
                ok = g[j] == x[j] if exact else abs(g[j] - x[j]) << 50 <= abs(x[j])
                assert ok, f"{kind} n={n} n_limbs={n_limbs} instance {c} coefficient {j}: got {g[j]}, want {x[j]}"
    plan.close()


# ---- ckks_encode ----
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", RINGS)
def test_encode_bit_exact_where_the_rounding_is_unambiguous(hx, ctx, dev, orc, setups, n, kind):
    qs, lm = setups(n, kind)
    plan = make_plan(hx, ctx, orc, n, qs)
    fam = [exact_family(n, 41 + s) for s in range(2)]
    count = 3
    d_z = to_dev_f64(tiled([z for _, z in fam], count), dev)
    for n_limbs in (1, 2, K):
        d_out = new_words(count, n_limbs, n, dev)
        plan.ckks_encode(d_out, d_z, count, n_limbs, 1024.0)
        ctx.sync()
        want = [ints_to_words(lm, m.astype(object) * 1024, n_limbs) for m, _ in fam]
        assert_instances(hx.to_u64(d_out), want, count, WORDS, (n_limbs, n), f"{kind} n={n} n_limbs={n_limbs}")
    assert plan.range_check()
    plan.close()


@pytest.mark.parametrize("n", RINGS)
def test_encode_at_working_magnitudes(hx, ctx, dev, orc, setups, n):
    qs, lm = setups(n, "seal")
    plan = make_plan(hx, ctx, orc, n, qs)
    n_limbs, count, scale = 2, 3, 2.0 ** 40
    zs = [rand_slots(n, 51 + s) for s in range(2)]
    d_out = new_words(count, n_limbs, n, dev)
    plan.ckks_encode(d_out, to_dev_f64(tiled(zs, count), dev), count, n_limbs, scale)
    ctx.sync()
    got = hx.to_u64(d_out).reshape(count, n_limbs, n)
    xs = [embed_inverse(as_complex(z), n) * LD(scale) for z in zs]
    for c in range(count):
        x = xs[c % 2]
        M = ints_to_ld(crt_lift(lm, got[c], n_limbs))
        err, bound = norm2(M - x), 0.5 * math.sqrt(n) + fft_bound(n) * norm2(x)
        rounding = norm2(np.rint(x) - x)
        print(f"encode n={n} instance {c}: |M - x| = {err:.4f}, bound {bound:.4f} (ratio {err / bound:.3f}), rounding alone {rounding:.4f}")
        assert err <= bound
    plan.close()


# ---- ckks_decode ----
@pytest.mark.parametrize("n", RINGS)
def test_decode_against_the_model(hx, ctx, dev, orc, setups, n):
    qs, lm = setups(n, "strict")
    plan = make_plan(hx, ctx, orc, n, qs)
    count, scale = 3, 2.0 ** 30
    for n_limbs, bits in ((3, 90), (1, 20)):
        rng = np.random.default_rng(61 + n_limbs)
        xs = []
        for s in range(2):
            mag = [int.from_bytes(rng.bytes(12), "little") % ((1 << bits) + 1) for _ in range(n)]
            xs.append(np.array([v if rng.integers(2) else -v for v in mag], dtype=object))
            xs[-1][:2] = [1 << bits, -(1 << bits)]
        words = tiled([ints_to_words(lm, x, n_limbs) for x in xs], count)
        d_z = new_f64((count, n // 2, 2), dev)
        plan.ckks_decode(d_z, hx.as_i64(words.reshape(-1)).to(dev), count, n_limbs, scale)
        ctx.sync()
        got = d_z.cpu().numpy()
        for c in range(count):
            z = embed(ints_to_ld(xs[c % 2]), n) / LD(scale)
            err, bound = norm2(as_complex(got[c]) - z), fft_bound(n) * norm2(z)
            print(f"decode n={n} n_limbs={n_limbs} instance {c}: |dz| / |z| = {err / norm2(z):.3e}, bound {fft_bound(n):.3e} (ratio {err / bound:.3f})")
            assert err <= bound
    plan.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", RINGS)
def test_round_trip_at_scale_2_40(hx, ctx, dev, orc, setups, n, kind):
    qs, lm = setups(n, kind)
    plan = make_plan(hx, ctx, orc, n, qs)
    n_limbs, count, scale = 2, 3, 2.0 ** 40
    z = tiled([rand_slots(n, 71 + s) for s in range(2)], count)
    d_w, d_back = new_words(count, n_limbs, n, dev), new_f64((count, n // 2, 2), dev)
    plan.ckks_encode(d_w, to_dev_f64(z, dev), count, n_limbs, scale)
    plan.ckks_decode(d_back, d_w, count, n_limbs, scale)
    ctx.sync()
    got = d_back.cpu().numpy()
    worst = float(np.abs(as_complex(got) - as_complex(z)).max())
    print(f"round trip {kind} n={n}: max |dz| = {worst:.3e}, bound {(n / 2 + 1) / scale:.3e}")
    assert np.isfinite(got).all() and worst <= (n / 2 + 1) / scale
    plan.close()


# ---- state ----
def test_one_instance_more_than_the_scratch_chunk(hx, ctx, dev, orc, setups):
    """n = 1024: a chunk is 4096 instances, so 4097 run as two; every instance against the model (encode) and against a two-instance
    call on another plan (decode), whose slots are checked against the model"""
    torch = torch_()
    n, n_limbs, count, scale = 1024, 2, 4097, 1024.0
    qs, lm = setups(n, "seal")
    fam = [exact_family(n, 81 + s) for s in range(2)]
    want = hx.as_i64(np.stack([ints_to_words(lm, m.astype(object) * 1024, n_limbs).reshape(-1) for m, _ in fam])).to(dev)
    small = make_plan(hx, ctx, orc, n, qs)
    d_ref = new_f64((2, n // 2, 2), dev)
    small.ckks_decode(d_ref, want.reshape(-1), 2, n_limbs, scale)
    ctx.sync()
    for c in range(2):
        z = as_complex(fam[c][1])
        assert norm2(as_complex(d_ref[c].cpu().numpy()) - z) <= 2 * fft_bound(n) * norm2(z)     # (the slots themselves were rounded to double)
    plan = make_plan(hx, ctx, orc, n, qs)
    idx = torch.arange(count, device=dev) % 2
    d_z = to_dev_f64(np.stack([z for _, z in fam]), dev)[idx].contiguous()
    d_w, d_back = new_words(count, n_limbs, n, dev), new_f64((count, n // 2, 2), dev)
    plan.ckks_encode(d_w, d_z, count, n_limbs, scale)
    plan.ckks_decode(d_back, d_w, count, n_limbs, scale)
    ctx.sync()
    bad = (d_w.view(count, -1) != want[idx]).any(dim=1)
    assert not bool(bad.any()), f"encode: {int(bad.sum())} of {count} instances wrong, the first is {int(torch.nonzero(bad)[0])}"
    bad = (d_back.view(count, -1) != d_ref.view(2, -1)[idx]).any(dim=1)
    assert not bool(bad.any()), f"decode: {int(bad.sum())} of {count} instances differ from the two-instance call, the first is {int(torch.nonzero(bad)[0])}"
    plan.close()
    small.close()


def test_a_larger_call_then_a_smaller_one_on_one_plan(hx, ctx, dev, orc, setups):
    n = 2048
    qs, lm = setups(n, "strict")
    plan = make_plan(hx, ctx, orc, n, qs)
    fam = [exact_family(n, 91 + s) for s in range(2)]
    for count, n_limbs in ((6, K), (2, 2), (5, 1)):
        d_z = to_dev_f64(tiled([z for _, z in fam], count), dev)
        d_w, d_c = new_words(count, n_limbs, n, dev), new_f64((count, n), dev)
        plan.ckks_encode(d_w, d_z, count, n_limbs, 1024.0)
        plan.rns_to_f64(d_c, d_w, count, n_limbs)
        ctx.sync()
        want = [ints_to_words(lm, m.astype(object) * 1024, n_limbs) for m, _ in fam]
        assert_instances(hx.to_u64(d_w), want, count, WORDS, (n_limbs, n), f"count={count} n_limbs={n_limbs}")
        got = d_c.cpu().numpy()
        for c in range(count):
            assert np.array_equal(got[c], fam[c % 2][0].astype(np.float64) * 1024), f"count={count}: coefficients of instance {c}"
    plan.close()


def test_encode_multiply_plain_decode_on_a_caller_stream(hx, ctx, dev, orc):
    """ct = (encode(a), encode(b)), pt = encode(w), all at scale 2^40; decode(ct . pt) at scale 2^80 is (a w, b w) slot by slot. An
    encoded slot is off by at most e = (n/2) / scale (n coefficients moved by at most 0.5 each), so a product of two is off by at most
    e (|a| + |w|) + e^2, and the decode adds far less than the remaining e: the bound is (n/2 + 1) / scale . (max|a| + max|w| + 1)."""
    torch = torch_()
    n, n_limbs, count, scale = 1024, 3, 3, 2.0 ** 40
    qs = chain(orc, "gen", K, n)
    plan = make_plan(hx, ctx, orc, n, qs)
    a = tiled([rand_slots(n, 101 + s) for s in range(2)], count * 2)              # [count][2 components]
    w = tiled([rand_slots(n, 111 + s) for s in range(2)], count)
    stream = torch.cuda.Stream(device=dev)
    d_a, d_wz = to_dev_f64(a, dev), to_dev_f64(w, dev)
    d_ct, d_pt = new_words(count * 2, n_limbs, n, dev), new_words(count, n_limbs, n, dev)
    d_out, d_back = new_words(count * 2, n_limbs, n, dev), new_f64((count * 2, n // 2, 2), dev)
    torch.cuda.synchronize()
    try:
        ctx.set_stream(stream.cuda_stream)
        plan.ckks_encode(d_ct, d_a, count * 2, n_limbs, scale)
        plan.ckks_encode(d_pt, d_wz, count, n_limbs, scale)
        plan.multiply_plain(d_out, d_ct, d_pt, count, 2, n_limbs, count)
        plan.ckks_decode(d_back, d_out, count * 2, n_limbs, scale * scale)
        stream.synchronize()
    finally:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    got = as_complex(d_back.cpu().numpy()).reshape(count, 2, n // 2)
    za, zw = as_complex(a).reshape(count, 2, n // 2), as_complex(w).reshape(count, 1, n // 2)
    bound = (n / 2 + 1) / scale * (float(np.abs(za).max()) + float(np.abs(zw).max()) + 1)
    worst = float(np.abs(got - za * zw).max())
    print(f"encode -> multiply_plain -> decode: max |dz| = {worst:.3e}, bound {bound:.3e}")
    assert worst <= bound
    assert plan.range_check()
    plan.close()


# ---- end to end with what exists ----
def test_encoded_rows_are_a_linear_transform_plaintext(hx, ctx, dev, orc, made):
    """n_limbs = K of an L = K - 1 plan: the encoder's [K][n] rows as d_pts[0] of hexl_linear_transform give, word for word, what the
    host-model-encoded plaintext gives -- the layout the header promises"""
    torch = torch_()
    n, L, Kp, nb = 1024, 2, 3, 4
    cases = cases_for(orc, n, L, Kp, 1)
    plans = plans_for(hx, ctx, cases, made)
    lm = Limbs(orc, n, [int(q) for q in cases[0].moduli])
    m, z = exact_family(n, 121)
    d_pt = new_words(1, Kp, n, dev)
    plans[0].ckks_encode(d_pt, to_dev_f64(z, dev), 1, Kp, 1024.0)
    want_pt = ints_to_words(lm, m.astype(object) * 1024, Kp).reshape(-1)
    d_ref_pt = hx.as_i64(want_pt).to(dev)
    cts = np.stack([uniform_ct(orc, cases[0], b) for b in range(2)])
    d_ct = hx.as_i64(cts).to(dev)[torch.arange(nb, device=dev) % 2].reshape(-1).contiguous()
    out_dev, out_ref = torch.full_like(d_ct, -1), torch.full_like(d_ct, -1)
    hx.linear_transform(plans, [5], [d_pt], out_dev, d_ct, nb)
    hx.linear_transform(plans, [5], [d_ref_pt], out_ref, d_ct, nb)
    ctx.sync()
    assert np.array_equal(hx.to_u64(d_pt), want_pt), "the encoded rows are not the model's"
    assert torch.equal(out_dev, out_ref) and not bool((out_dev == -1).all())
    assert plans[0].range_check()
